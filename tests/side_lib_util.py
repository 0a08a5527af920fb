"""What the CPU tests of the side libraries (devio, gate, consistency, health, lookahead, sequence, score, bank, imm, adapt, stateio) share: building a
library that is missing, holding its exports to its header and its binding, the stale-EXEC audit and the kernel descriptors of the
generated assembly, and the stand-ins that let an entry point or DeviceIO be called without a GPU.  What a library expects -- its
names, kernel counts, families, bounds -- stays in its own test."""
import collections
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np

from elf_util import _symbols
from quadrotor_landing_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quadrotor_landing_amd", "csrc")


def _side(lib_module):
    """the SideLibrary of quadrotor_landing_amd/NAME.py: its NAME in capitals"""
    return getattr(lib_module, lib_module.__name__.rpartition(".")[2].upper())


def ensure_built(name):
    """-> the path of libqle_NAME.so, made first if it is missing"""
    path = _side(importlib.import_module("quadrotor_landing_amd." + name)).path
    if not os.path.exists(path):
        subprocess.run(["make", "-C", CSRC, f"../libqle_{name}.so"], check=True)
    return path


def declared_functions(header, prefix):
    """-> (the sorted names PREFIX_* followed by a parenthesis in the header, its text without comments)"""
    txt = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return sorted(set(re.findall(rf"\b({prefix}_[a-z0-9_]+)\s*\(", txt))), txt


def assert_exports_and_binds(lib_module, header, prefix, so, expected=None):
    """Every function the header declares is exported and bound, the binding names nothing else, and nothing else with the library's
    prefix is exported.  -> (names, the header's text without comments)"""
    names, txt = declared_functions(header, prefix)
    assert names and (expected is None or names == expected), names
    L = _side(lib_module).load()
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/{os.path.basename(header)} but not exported"
    assert sorted(lib_module.SYMBOLS) == names
    exported = {s for s in _symbols(open(so, "rb").read(), 11) if s.startswith(prefix + "_")}   # SHT_DYNSYM
    assert exported == set(names), sorted(exported ^ set(names))
    return names, txt


def run_audit(name):
    """make audit-NAME -> (the completed process, the path of the generated assembly it read)"""
    r = subprocess.run(["make", "-C", CSRC, "audit-" + name], capture_output=True, text=True, timeout=900)
    return r, os.path.join(CSRC, "build", "asm", name + "_capi.s")


def assert_audit_counts(result, name, n=None):
    """The audit passed over exactly n kernels (n = None: over at least one)."""
    assert result.returncode == 0, result.stdout[-3000:] + result.stderr[-2000:]
    m = re.search(rf"audit-{name}: no register copy under a stale EXEC in (\d+) kernels", result.stdout)
    assert m and (int(m.group(1)) >= 1 if n is None else int(m.group(1)) == n), result.stdout[-2000:]


Descriptor = collections.namedtuple("Descriptor", "scratch lds vgpr")


def kernel_descriptors(asm):
    """-> ({demangled kernel name: Descriptor(bytes of private segment, bytes of LDS, next free VGPR)} from the .amdhsa_kernel blocks of
    the assembly at `asm`, the .private_segment_fixed_size lines of its code object metadata)"""
    txt = open(asm).read()
    found = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, flags=re.S):
        get = lambda key: int(re.search(rf"\.amdhsa_{key} (\d+)", m.group(2)).group(1))   # noqa: E731
        found[_lib.demangle(m.group(1))] = Descriptor(get("private_segment_fixed_size"), get("group_segment_fixed_size"), get("next_free_vgpr"))
    return found, re.findall(r"\.private_segment_fixed_size:.*", txt)


def scratch_free(meta):
    """every .private_segment_fixed_size line of the metadata says 0"""
    return all(re.search(r"\.private_segment_fixed_size:\s+0\b", s) for s in meta)


# ---------------------------------------------------------------- stand-ins: no GPU call is reached
class FakeTensor:
    def __init__(self, shape, dtype="float32", device="cuda:0", contiguous=True, ptr=0x7F0000000000):
        self.shape, self.dtype, self.device, self._c, self._p = tuple(shape), dtype, device, contiguous, ptr

    def data_ptr(self):
        return self._p

    def is_contiguous(self):
        return self._c

    def numel(self):
        return int(np.prod(self.shape, dtype=np.int64))

    def __getitem__(self, idx):
        """A view: ints drop a dimension, slices shorten it; the storage stays the base's."""
        idx = idx if isinstance(idx, tuple) else (idx,)
        idx += (slice(None),) * (len(self.shape) - len(idx))
        shape = [len(range(*i.indices(d))) for d, i in zip(self.shape, idx) if isinstance(i, slice)]
        return type(self)(shape, self.dtype, self.device, ptr=self._p)

    def zero_(self):
        return self


class FakeEkf:
    """what DeviceIO reads of a handle"""
    batch, dtype, device, num_states = 100, _lib.QLE_F32, 0, 15
    _h = None


class _Reader:
    """takes consecutive pieces of a harness's int64 stream"""

    def __init__(self, a):
        self.a, self.p = a, 0

    def take(self, n):
        v = self.a[self.p:self.p + n]
        assert v.size == n
        self.p += n
        return v


def _view(batch=100, dtype=_lib.QLE_F32, n=15, compact=0):
    v = _lib.QleDeviceView()
    v.struct_size = C.sizeof(v); v.device = 0; v.dtype = dtype; v.num_states = n; v.batch = batch; v.padded_batch = -(-batch // 64) * 64
    v.state = 0x7F0000000000; v.state_words = 144; v.record_words = 64 if compact else 136; v.compact = compact
    return v


def _views(batch=100, dtype=_lib.QLE_F32, tag=True):
    iv = _lib.QleInputsView()
    iv.struct_size = C.sizeof(iv); iv.has_tag = int(tag); iv.u = 0x7F1000000000; iv.z = 0x7F2000000000 if tag else None
    return _view(batch, dtype), iv


def _params(**kw):
    p = _lib.QleParams()
    _lib.check(_lib.lib().qle_params_default(C.byref(p)))
    for k, val in kw.items():
        setattr(p, k, val)
    return p
