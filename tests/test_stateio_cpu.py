"""CPU tests of the device state I/O (include/qle_stateio.h, libqle_stateio.so, quadrotor_landing_amd/stateio.py, csrc/ekf_stateio.hpp):
the library builds, exports and binds what its header declares, its kernels are its own, its generated code passes the stale-EXEC audit
and uses no scratch memory, every refusal is made before any GPU call (without a GPU a HIP call would fail with another error class),
and the index and packing arithmetic of k_si_pack and k_si_copy -- compiled for the host with g++, once more as a stand-alone program
under AddressSanitizer and UBSan -- gives, bit for bit, the array a numpy restatement of off(w, i) gives: pack, identity copy, masked
copy, an index with duplicates, -1 and `batch`, with the untouched words (the ragged tail, the words >= record_words) compared too.

What the host build does not cover are the kernels' loads and stores themselves and the Python classes: tests/test_gpu_stateio.py.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import host_harness
import side_lib_util
import stateio_util as su
from elf_util import _kernels, _needed
from quadrotor_landing_amd import _lib, devio, stateio
from side_lib_util import (FakeTensor, _params, _view, assert_audit_counts, assert_exports_and_binds, ensure_built, kernel_descriptors,
                           run_audit, scratch_free)
from util import forbid_native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qle_stateio.h")
CLANGXX = "/opt/rocm/lib/llvm/bin/clang++"
N_COPY, N_PACK = 4, 12  # k_si_copy: dtype x record kind; k_si_pack: T x S x (15 full, 9 full, 9 compact)


@pytest.fixture(scope="module")
def sio_so():
    return ensure_built("stateio")


# ---------------------------------------------------------------- 1. header, exports, kernels
def test_library_exports_and_binds_every_declared_function(sio_so):
    _, txt = assert_exports_and_binds(stateio, HEADER, "qsi", sio_so,
                                      ["qsi_copy", "qsi_copy_host", "qsi_last_error", "qsi_launch_census_begin", "qsi_launch_census_end", "qsi_launch_count", "qsi_pack_state", "qsi_workspace_bytes"])
    assert re.search(r"#define QSI_F32 0\b", txt) and re.search(r"#define QSI_F64 1\b", txt)
    assert (stateio.QSI_F32, stateio.QSI_F64) == (devio.QDV_F32, devio.QDV_F64) == (0, 1)


def test_tick_library_declares_exports_and_binds_the_mark():
    txt = open(os.path.join(ROOT, "include", "qle_ekf.h")).read()
    assert re.search(r"\bint qle_mark_state_written\(qle_batch \*h\);", txt)
    assert "qle_mark_state_written" in _lib.SYMBOLS and hasattr(_lib.lib(), "qle_mark_state_written")
    assert _lib.lib().qle_mark_state_written(None) == _lib.QLE_ERR_INVALID   # a null handle is refused, not dereferenced


def test_kernels_are_the_librarys_own(sio_so):
    mine = {_lib.demangle(m) for m in _kernels(sio_so)}
    assert len(mine) == N_COPY + N_PACK, sorted(mine)
    assert all(re.match(r"void qsi::k_si_(copy|pack)<", k) for k in mine), sorted(mine)
    assert sum("k_si_copy<" in k for k in mine) == N_COPY
    for p in (_lib.LIB_PATH, devio.DEVIO_LIB_PATH):
        assert not any("k_si_" in _lib.demangle(m) for m in _kernels(p)), p
    needed = _needed(sio_so)
    assert any(n.startswith("libamdhip64") for n in needed) and not [n for n in needed if "qle_" in n], needed   # the HIP runtime only


# ---------------------------------------------------------------- 2. audit and resources
@pytest.fixture(scope="module")
def audit(sio_so):
    return run_audit("stateio")


def test_generated_device_code_passes_the_stale_exec_audit(audit):
    assert_audit_counts(audit[0], "stateio", N_COPY + N_PACK)


def test_no_kernel_uses_scratch_memory(audit):
    r, asm = audit
    assert r.returncode == 0
    found, meta = kernel_descriptors(asm)
    assert len(found) == N_COPY + N_PACK and all("k_si_" in k for k in found), sorted(found)
    for name, (scratch, lds, vgpr) in found.items():
        print(f"{name.split('(')[0]}: scratch {scratch} B, LDS {lds} B, registers {vgpr}")
        assert scratch == 0, (name, scratch)
        assert lds == 0 if "k_si_copy<" in name else 0 < lds <= 64 * 1024, (name, lds)
        assert vgpr <= 512, (name, vgpr)
    assert scratch_free(meta), meta


def test_copy_requests_a_records_loads_ahead_of_its_stores(audit):
    """In the generated code of k_si_copy every batch of dwordx4 loads (a whole fp32 record, half an fp64 record, the parameter record)
    stands in front of the stores of those rows: the sequence of runs is loads, the same number of stores, loads, ..."""
    txt = open(audit[1]).read()
    want = {(16, 36, 6): [16, 6], (34, 36, 6): [34, 6], (32, 72, 12): [32, 12], (68, 72, 12): [34, 34, 12]}
    seen = 0
    for m in re.finditer(r"^(_ZN3qsi9k_si_copyILi(\d+)ELi(\d+)ELi(\d+)E\w+):\s.*?s_endpgm", txt, flags=re.S | re.M):
        ops = re.findall(r"\b(global_load_dwordx4|global_store_dwordx4)\b", m.group(0))
        runs = []
        for op in ops:
            if runs and runs[-1][0] == op:
                runs[-1][1] += 1
            else:
                runs.append([op, 1])
        batches = want[tuple(int(g) for g in m.group(2, 3, 4))]
        assert [(o.split("_")[1], c) for o, c in runs] == [p for b in batches for p in (("load", b), ("store", b))], (m.group(1), runs)
        seen += 1
    assert seen == N_COPY


# ---------------------------------------------------------------- 3. refusals, before any GPU call
def test_library_refuses_before_any_gpu_call(sio_so):
    """No GPU here: a call that got as far as the HIP runtime would return QLE_ERR_HIP (or crash on the fake pointers), not these."""
    S = stateio.stateio_lib()
    B = C.byref
    INV = _lib.QLE_ERR_INVALID
    err = lambda: S.qsi_last_error()
    X, PP, MK, IDX, WR, WS, FP1, FP2 = (0x7F1000000000 + k * 0x1000000000 for k in range(8))

    def dst_of(v, state=WS, fp=None):
        d = _view(batch=v.batch, dtype=v.dtype, n=v.num_states, compact=v.compact)
        d.state, d.filter_params = state, fp
        return d

    v = _view()
    assert S.qsi_workspace_bytes(B(v)) == 128 * 144 * 4 and S.qsi_workspace_bytes(B(_view(dtype=_lib.QLE_F64, batch=64))) == 64 * 144 * 8
    pack = lambda v_=B(v), x=X, P=PP, dt=stateio.QSI_F32, m=MK: S.qsi_pack_state(v_, x, P, dt, m)
    copy = lambda s=v, d=None, idx=None, m=MK, wp=0, wr=WR, fn=S.qsi_copy: fn(B(s), B(dst_of(s) if d is None else d), idx, m, wp, wr)
    assert pack(v_=None) == INV and b"view" in err()
    for size in (0, C.sizeof(v) - 8, C.sizeof(v) + 8):                      # a wrong struct_size
        bad = _view(); bad.struct_size = size
        assert pack(v_=B(bad)) == INV and b"struct_size" in err()
        assert S.qsi_workspace_bytes(B(bad)) == INV
        assert copy(s=bad, d=dst_of(v)) == INV and b"struct_size" in err()
        bad_d = dst_of(v); bad_d.struct_size = size
        assert copy(d=bad_d) == INV and b"struct_size" in err()
    odd = _view(); odd.state = 0x7F0000000008                                # misaligned pointers
    assert pack(v_=B(odd)) == INV and b"aligned" in err()
    assert pack(x=X + 8) == INV and b"aligned" in err()
    assert pack(P=PP + 4) == INV and b"aligned" in err()
    assert copy(d=dst_of(v, state=WS + 8)) == INV and b"aligned" in err()
    assert copy(idx=IDX + 2) == INV and b"aligned" in err()
    assert copy(s=dst_of(v, v.state, FP1 + 8), d=dst_of(v, fp=FP2), wp=1) == INV and b"aligned" in err()
    for dt in (2, -1, 7):                                                     # a bad dtype: of the tensors, of a view
        assert pack(dt=dt) == INV and b"src_dtype" in err()
    assert pack(v_=B(_view(dtype=7))) == INV and copy(s=_view(dtype=7)) == INV
    assert pack(x=None, P=None) == INV and b"both null" in err()             # x and P both NULL
    for wrong in (dict(n=12), dict(batch=0), dict(n=15, compact=1)):
        assert pack(v_=B(_view(**wrong))) == INV
    rw = _view(); rw.record_words = 64                                        # full records of 64 words
    assert pack(v_=B(rw)) == INV and b"record_words" in err()
    # views that disagree
    f64 = dst_of(_view(dtype=_lib.QLE_F64))
    assert copy(d=f64) == INV and b"dtype" in err()
    assert copy(d=dst_of(_view(n=9))) == INV and b"num_states" in err()
    assert copy(s=_view(n=9), d=dst_of(_view(n=9, compact=1))) == INV and b"compact" in err()
    other = dst_of(v); other.device = 1
    assert copy(d=other) == INV and b"device" in err()
    assert copy(d=dst_of(_view(batch=70))) == INV and b"batch" in err()       # unequal batches without an index ...
    need = 128 * 144 * 4
    for state in (v.state, v.state + need - 16, v.state - need + 16, v.state + 16):   # an index with overlapping states
        assert copy(d=dst_of(v, state=state), idx=IDX) == INV and b"overlap" in err() and b"permutation" in err(), hex(state)
    assert copy(d=dst_of(v, state=v.state)) == INV and b"overlap" in err()    # ... and a copy onto itself
    assert copy(wp=1) == INV and b"filter_params" in err()                    # with_params without parameter records: neither,
    assert copy(s=dst_of(v, v.state, FP1), wp=1) == INV and b"dst has no" in err()   # the destination,
    assert copy(d=dst_of(v, fp=FP2), wp=1) == INV and b"src has no" in err()         # the source
    assert copy(s=dst_of(v, v.state, FP1), d=dst_of(v, fp=FP1), wp=1) == INV and b"overlap" in err()
    # the host entry refuses the same, before it allocates anything
    idx, m, wr = np.zeros(100, np.int32), np.ones(100, np.uint8), np.zeros(100, np.uint8)
    pi, pu = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    host = lambda s=v, d=None, i=idx.ctypes.data_as(pi), wp=0: S.qsi_copy_host(B(s), B(dst_of(s) if d is None else d), i, m.ctypes.data_as(pu), wp,
                                                                              wr.ctypes.data_as(pu))
    assert host(d=f64) == INV and host(d=dst_of(v, state=v.state)) == INV and host(wp=1) == INV
    assert host(d=dst_of(_view(batch=70)), i=None) == INV and b"batch" in err()
    assert S.qsi_launch_count() == 0


class FakeEkf(side_lib_util.FakeEkf):
    def __init__(self, dtype=_lib.QLE_F32, **kw):
        self.params = _params(**kw)
        self.dtype = dtype


def test_deviceio_refuses_before_any_gpu_call(monkeypatch):
    single, multirate, f64 = FakeEkf(), FakeEkf(multirate_ekf=1), FakeEkf(dtype=_lib.QLE_F64)   # parameters come from the tick library: made first
    forbid_native(monkeypatch)
    B = 100
    io, mr = devio.DeviceIO(single), devio.DeviceIO(multirate)
    x, P, m = FakeTensor((B, 16)), FakeTensor((B, 15, 15)), FakeTensor((B,), dtype="uint8")
    idx = FakeTensor((B,), dtype="int32")
    snap = stateio.Snapshot(io, _lib.QleDeviceView(), FakeTensor((128 * 144 * 4,), dtype="uint8"), None)
    # a masked write on a multirate handle: every entry that takes a mask
    for call in (lambda: mr.set_state(x, P, mask=m), lambda: mr.restore(stateio.Snapshot(mr, _lib.QleDeviceView(), None, None), mask=m),
                 lambda: mr.gather(idx, mask=m)):
        with pytest.raises(_lib.QleError, match="multirate_ekf") as e:
            call()
        assert e.value.code == _lib.QLE_ERR_STATE
    # a snapshot of another dtype, of another batch without an index, without parameter records
    with pytest.raises(ValueError, match="dtype"):
        devio.DeviceIO(f64).restore(snap)
    small = stateio.Snapshot(io, _lib.QleDeviceView(), None, None); small.batch = 70
    with pytest.raises(ValueError, match="index"):
        io.restore(small)
    with pytest.raises(ValueError, match="with_params"):
        io.restore(snap, with_params=True)
    with pytest.raises(ValueError, match="Snapshot"):
        io.restore(x)
    # tensors
    for bad in (dict(x=None, P=None), dict(x=FakeTensor((B, 15)), P=P), dict(x=x, P=FakeTensor((B, 9, 9))), dict(x=x, P=FakeTensor((B, 15, 15), dtype="float64")),
                dict(x=np.zeros((B, 16)), P=P), dict(x=FakeTensor((B, 16), device="cuda:1"), P=P), dict(x=x, P=P, mask=FakeTensor((B,), dtype="int32"))):
        with pytest.raises(ValueError):
            io.set_state(**bad)
    for bad_idx in (FakeTensor((B,), dtype="int64"), FakeTensor((B + 1,), dtype="int32"), np.zeros(B, np.int32), FakeTensor((B,), dtype="int32", ptr=0x7F0000000002)):
        with pytest.raises(ValueError):
            io.gather(bad_idx)
        with pytest.raises(ValueError):
            io.restore(snap, index=bad_idx)
    for kw in (dict(members=3), dict(members=0), dict(members=4, source=4), dict(members=4, source=-1), dict(members=2.5)):
        with pytest.raises(ValueError):
            io.fork(**kw)
    for good in (lambda: io.set_state(x, P, mask=m), lambda: io.set_state(x), lambda: mr.set_state(x, P), lambda: io.snapshot(),
                 lambda: io.restore(snap, mask=m, index=idx), lambda: io.gather(idx, mask=m), lambda: mr.gather(idx)):
        with pytest.raises(AssertionError, match="native library"):
            good()   # a good call is what reaches the libraries


# ---------------------------------------------------------------- 4. the arithmetic on the host, once more under the sanitizers
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/cpp/stateio_harness.cpp: the index and packing functions of ekf_stateio.hpp compiled for the host, once as they are and once
    as a stand-alone program under AddressSanitizer and UBSan.  By clang++, as the devio index harness: the layout header under them
    declares its 16-byte quads as vector types a host g++ does not have."""
    return host_harness.build("stateio_harness", tmp_path_factory, cxx=CLANGXX, flags=host_harness.FLAGS[:5] + ("-Wno-unused-variable", "-Wno-pass-failed"))


BATCHES = (1, 64, 65, 200)   # one filter, a whole tile, a tile and one lane, three tiles + 8
GRID = [(k, B) for k in su.KINDS for B in BATCHES]
GRID_IDS = [f"{k}-B{B}" for k, B in GRID]


def run_harness(exe, tmp, B, kind, mode, payload, src_f64=False, src_B=None, use_index=False, use_x=True, use_P=True):
    dtype, n, compact = su.KINDS[kind]
    hdr = [B, mode, dtype == "f64", src_f64, n, compact, B if src_B is None else src_B, use_index, use_x, use_P]
    o = host_harness.run(exe, tmp, hdr, payload, (su.padded(B) * su.SW + B,))
    return o[:su.padded(B) * su.SW].astype(su.NP_T[dtype]), o[su.padded(B) * su.SW:].astype(np.uint8)


@pytest.mark.parametrize("kind,B", GRID, ids=GRID_IDS)
def test_host_compiled_pack_gives_the_words_of_set_state(harness, tmp_path, kind, B):
    dtype, n, compact = su.KINDS[kind]
    prior = su.sentinel(B, dtype, seed=B)
    mask = np.ones(B, np.uint8); mask[1::3] = 0
    for src in ("f32", "f64"):
        x, P = su.random_state(B, n, seed=7 * B + n, dtype=src)
        assert B == 1 or not np.array_equal(P, P.transpose(0, 2, 1))          # the symmetrisation has something to do
        for exe in harness:
            for m, ux, uP in ((None, True, True), (mask, True, True), (None, True, False), (mask, False, True)):
                got, on = run_harness(exe, tmp_path, B, kind, 0, [x, P, np.ones(B) if m is None else m, prior], src_f64=src == "f64", use_x=ux, use_P=uP)
                want = su.expected_pack(prior, B, dtype, compact, x if ux else None, P if uP else None, m)
                assert su.same_bits(got, want), np.argwhere(su.bits(got) != su.bits(want)).ravel()[:8]
                assert np.array_equal(on, np.ones(B, np.uint8) if m is None else m)
    # what must not move did not: the lanes beyond B in the last tile and the words >= record_words of every filter
    tail = su.off(np.arange(su.SW)[None, :], np.arange(B, su.padded(B))[:, None], dtype).ravel()
    beyond = su.record_offsets(B, dtype, su.SW)[:, su.RECORD_WORDS[compact]:].ravel()
    assert su.same_bits(got[tail], prior[tail]) and su.same_bits(got[beyond], prior[beyond]) and beyond.size == B * (80 if compact else 8)


@pytest.mark.parametrize("kind,B", GRID, ids=GRID_IDS)
def test_host_compiled_copy_is_the_numpy_gather(harness, tmp_path, kind, B):
    dtype, n, compact = su.KINDS[kind]
    rng = np.random.default_rng(B)
    prior, src = su.sentinel(B, dtype, seed=B + 1), su.sentinel(B, dtype, seed=B + 2)
    mask = np.ones(B, np.uint8); mask[::2] = 0
    index = rng.integers(0, B, B); index[::5] = index[0]                      # duplicates; -1 and B where there is room
    if B > 2:
        index[1], index[B - 1] = -1, B
    cases = [(src, B, None, None), (src, B, None, mask), (src, B, index, None), (src, B, index, mask)]
    small_B = 70                                                              # a source of another batch size, through an index
    small = su.sentinel(small_B, dtype, seed=B + 3)
    cross = rng.integers(-1, small_B + 1, B)
    cases.append((small, small_B, cross, None))
    for s, sB, idx, m in cases:
        want, ok = su.expected_copy(s, prior, sB, B, dtype, compact, idx, m)
        for exe in harness:
            got, written = run_harness(exe, tmp_path, B, kind, 1, [np.zeros(B) if idx is None else idx, np.ones(B) if m is None else m, s, prior],
                                       src_B=sB, use_index=idx is not None)
            assert su.same_bits(got, want), np.argwhere(su.bits(got) != su.bits(want)).ravel()[:8]
            assert np.array_equal(written, ok)
        tail = su.off(np.arange(su.SW)[None, :], np.arange(B, su.padded(B))[:, None], dtype).ravel()
        beyond = su.record_offsets(B, dtype, su.SW)[:, su.RECORD_WORDS[compact]:].ravel()
        assert su.same_bits(got[tail], prior[tail]) and su.same_bits(got[beyond], prior[beyond])
        assert su.same_bits(got, prior) == (not ok.any())                     # and something did, wherever a filter was written
