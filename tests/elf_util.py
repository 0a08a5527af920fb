"""Readers of the built libraries: ELF64 sections and symbols, the gfx950 code objects inside .hip_fatbin, the kernels they hold and the
DT_NEEDED entries.  No external tool."""
import struct

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _sections(d):
    shoff = struct.unpack_from("<Q", d, 0x28)[0]
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", d, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", d, shoff + i * shentsize) for i in range(shnum)]
    stro = secs[shstrndx][4]
    return [(d[stro + s[0]:d.index(b"\0", stro + s[0])].decode(),) + s[1:] for s in secs]


def _symbols(d, sh_type):
    """names of the defined symbols of an ELF64 little-endian image's SHT_SYMTAB (2) or SHT_DYNSYM (11) sections"""
    secs = _sections(d)
    out = []
    for s in secs:
        if s[1] != sh_type:
            continue
        strtab = secs[s[6]][4]
        for i in range(0, s[5], 24):
            st_name, _, _, shndx, _, _ = struct.unpack_from("<IBBHQQ", d, s[4] + i)
            if st_name and shndx:
                o = strtab + st_name
                out.append(d[o:d.index(b"\0", o)].decode())
    return out


def _gfx950_code_objects(d):
    """The .hip_fatbin section holds one offload bundle per translation unit, each at a 4 KiB-aligned offset."""
    sec = [s for s in _sections(d) if s[0] == ".hip_fatbin"]
    assert sec, "the library has no .hip_fatbin section"
    fat = d[sec[0][4]:sec[0][4] + sec[0][5]]
    cos = []
    for off in range(0, len(fat), 4096):
        if fat[off:off + len(MAGIC)] != MAGIC:
            continue
        n = struct.unpack_from("<Q", fat, off + 24)[0]
        p = off + 32
        for _ in range(n):
            eo, es, ts = struct.unpack_from("<QQQ", fat, p)
            triple = fat[p + 24:p + 24 + ts].decode()
            p += 24 + ts
            if triple.endswith("gfx950") and es:
                co = fat[off + eo:off + eo + es]
                assert co[:4] == b"\x7fELF", f"bundle at {off}: {triple} is not an ELF code object (compressed?)"
                cos.append(co)
    return cos


def _kernels(path):
    """the mangled names of the kernels in the gfx950 code objects of the library at `path`"""
    kds = []
    for co in _gfx950_code_objects(open(path, "rb").read()):
        kds += [s[:-3] for s in _symbols(co, 2) if s.endswith(".kd")]
    return set(kds)


def _needed(path):
    """the DT_NEEDED entries of the library at `path`"""
    d = open(path, "rb").read()
    secs = _sections(d)
    dyn = [s for s in secs if s[0] == ".dynamic"][0]
    strtab = secs[dyn[6]][4]
    out = []
    for o in range(dyn[4], dyn[4] + dyn[5], 16):
        tag, val = struct.unpack_from("<qQ", d, o)
        if tag == 0:
            break
        if tag == 1:   # DT_NEEDED
            out.append(d[strtab + val:d.index(b"\0", strtab + val)].decode())
    return out
