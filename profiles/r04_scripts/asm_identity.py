#!/usr/bin/env python3
"""Compare the device assembly of two builds kernel by kernel: body, .amdhsa descriptor, metadata entry.
usage: asm_identity.py DIR_A DIR_B   (directories of *.s files from `make audit`)"""
import os, re, sys

def norm(line):
    line = line.split(';', 1)[0].rstrip()
    line = re.sub(r'\.L(BB|JTI|func_end|func_begin|tmp)(\d+)', lambda m: '.L' + m.group(1), line)
    return line

def parse(path):
    lines = open(path).read().split('\n')
    kernels = {}
    names = [m.group(1) for l in lines for m in [re.match(r'\s*\.amdhsa_kernel (\S+)', l)] if m]
    idx = {l.split(':')[0]: n for n, l in enumerate(lines) if re.match(r'^[A-Za-z_][\w$.]*:', l)}
    for name in names:
        n = idx[name]
        body, desc, in_desc = [], [], False
        while not re.match(r'^\.Lfunc_end\d+:', lines[n]):
            l = lines[n]
            if re.match(r'\s*\.amdhsa_kernel ', l): in_desc = True
            if in_desc: desc.append(norm(l))
            else:
                t = norm(l)
                if t.strip(): body.append(t)
            if re.match(r'\s*\.end_amdhsa_kernel', l): in_desc = False
            n += 1
        kernels[name] = [body, desc, None]
    # metadata: entries of amdhsa.kernels, each starts with "  - .agpr_count" (keys are sorted)
    a = next(n for n, l in enumerate(lines) if l.strip() == '.amdgpu_metadata')
    b = next(n for n, l in enumerate(lines) if l.strip() == '.end_amdgpu_metadata')
    entry = None
    for l in lines[a:b] + ['amdhsa.end']:
        if l.startswith('  - ') or l.startswith('amdhsa.'):
            if entry:
                nm = next(re.match(r'\s*\.name:\s+(\S+)', e).group(1) for e in entry if re.match(r'\s*\.name:\s', e) and not e.startswith('      '))
                kernels[nm][2] = entry
            entry = [l] if l.startswith('  - .') else None
        elif entry is not None:
            entry.append(l)
    return kernels

def main(da, db):
    bad = 0
    for f in sorted(os.listdir(da)):
        if not f.endswith('.s'): continue
        ka, kb = parse(os.path.join(da, f)), parse(os.path.join(db, f))
        diffs = []
        if set(ka) != set(kb):
            diffs.append('symbol sets differ: only A %s, only B %s' % (sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))))
        for k in sorted(set(ka) & set(kb)):
            what = [w for w, x, y in zip(('body', 'descriptor', 'metadata'), ka[k], kb[k]) if x != y or x is None]
            if what: diffs.append('%s: %s differ' % (k, ', '.join(what)))
        print('%-20s %3d kernels  %s' % (f, len(ka), 'identical' if not diffs else 'DIFFERENT'))
        for d in diffs: print('    ' + d)
        bad += len(diffs)
    return 1 if bad else 0

if __name__ == '__main__':
    sys.exit(main(sys.argv[1], sys.argv[2]))
