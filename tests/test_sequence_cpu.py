"""CPU tests of the sequence boundary (include/qle_sequence.h, libqle_sequence.so, quadrotor_landing_amd/sequence.py,
csrc/sequence_kernels.hpp, sequence_index.hpp, sequence_plan.hpp): the library builds, exports and binds what its header declares,
`qsq_run_opts` has the layout the binding assumes, the generated code passes the stale-EXEC audit and uses no scratch memory, its
kernels are its own and all k_sq_pack, the staging walk of a misaligned span and the pack plan -- compiled for the host with g++ under
ASan/UBSan into a stand-alone program -- move every word exactly once and nothing else, and DeviceIO.sequence / run refuse bad
arguments before any GPU call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import host_harness
import side_lib_util
from elf_util import _kernels, _needed
from quadrotor_landing_amd import _lib, devio, sequence
from side_lib_util import (FakeTensor, _Reader, _view, assert_audit_counts, assert_exports_and_binds, ensure_built, kernel_descriptors,
                           run_audit, scratch_free)
from util import forbid_native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qle_sequence.h")


@pytest.fixture(scope="module")
def sequence_so():
    return ensure_built("sequence")


def test_library_exports_and_binds_every_declared_function(sequence_so):
    _, txt = assert_exports_and_binds(sequence, HEADER, "qsq", sequence_so, ["qsq_last_error", "qsq_launch_census_begin", "qsq_launch_census_end", "qsq_launch_count", "qsq_pack", "qsq_run"])
    assert sequence.CHUNK == int(re.search(r"#define QSQ_CHUNK (\d+)", txt).group(1)) == 32


def test_run_opts_layout_matches_the_header(tmp_path):
    fields = [n for n, _ in sequence.QsqRunOpts._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qle_sequence.h"\nint main(void) {\n  printf("%zu", sizeof(qsq_run_opts));\n'
                   + "".join(f'  printf(" %zu", offsetof(qsq_run_opts, {f}));\n' for f in fields) + '  printf("\\n"); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    O = sequence.QsqRunOpts
    assert got == [C.sizeof(O)] + [getattr(O, f).offset for f in fields]
    assert O.struct_size.offset == 0
    # every field of the header's struct is bound: the C program compiled with exactly these names, and the sizes agree
    body = re.search(r"typedef struct qsq_run_opts \{(.*?)\} qsq_run_opts;", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S), flags=re.S).group(1)
    declared = re.findall(r"(\w+)\s*;", body)
    assert declared == fields


@pytest.fixture(scope="module")
def audit(sequence_so):
    return run_audit("sequence")


def test_generated_device_code_passes_the_stale_exec_audit(audit):
    assert_audit_counts(audit[0], "sequence")


def test_no_kernel_uses_scratch_memory(audit):
    """The kernel descriptors and the code object metadata of the generated assembly: 0 bytes of private segment in each of the four
    (compute dtype, source dtype) instantiations of k_sq_pack, and the two LDS images of 64 x 7 words."""
    r, asm = audit
    assert r.returncode == 0
    found, meta = kernel_descriptors(asm)
    found = {name.split("(")[0]: d for name, d in found.items()}
    assert sorted(found) == [f"void qsq::k_sq_pack<{t}, {s}>" for t in ("double", "float") for s in ("double", "float")], sorted(found)
    for name, (scratch, lds, vgpr) in found.items():
        print(f"{name}: scratch {scratch} B, registers {vgpr}, LDS {lds} B")
        assert scratch == 0, (name, scratch)
        assert lds == 2 * 64 * 7 * (8 if "<double" in name else 4), (name, lds)
    assert len(meta) == 4 and scratch_free(meta), meta


def test_kernels_are_its_own_and_all_k_sq_pack(sequence_so):
    mine = _kernels(sequence_so)
    assert mine
    for other in (_lib.LIB_PATH, devio.DEVIO_LIB_PATH):
        theirs = _kernels(other)
        assert theirs and not mine & theirs, sorted(mine & theirs)
        assert not any("qsq::" in _lib.demangle(m) for m in theirs)
    ids = {_lib.demangle(m) for m in mine}
    assert all(i.startswith("void qsq::k_sq_pack<") for i in ids) and len(ids) == 4, sorted(ids)
    # the boundary library keeps exactly its three families: the record stores the two packs share are inlined helpers, not kernels
    fam = {_lib.demangle(m).split("<")[0].split("::")[1] for m in _kernels(devio.DEVIO_LIB_PATH)}
    assert fam == {"k_dv_pack", "k_dv_state", "k_dv_report"}, fam


def test_library_links_the_four_it_drives(sequence_so):
    needed = _needed(sequence_so)
    for lib in ("libqle_ekf.so", "libqle_devio.so", "libqle_gate.so", "libqle_consistency.so"):
        assert lib in needed, needed
    d = open(sequence_so, "rb").read()
    assert b"$ORIGIN" in d


# ---------------------------------------------------------------- the stand-alone harness: staging walk and plan
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/cpp/sequence_harness.cpp built with g++ under ASan + UBSan and run directly, nothing preloaded."""
    exe, = host_harness.build("sequence_harness", tmp_path_factory, plain=False, flags=("-Wall", "-Werror"))
    out = exe + ".bin"
    r = subprocess.run([exe, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]   # a sanitizer report ends the program with a non-zero status
    data = np.fromfile(out, dtype=np.int64)
    assert data.size == int(r.stdout.split()[0])
    return data


def test_staging_walk_moves_every_valid_word_once_and_nothing_else(harness):
    rd = _Reader(harness)
    # head words in front of the next 16-byte boundary
    np.testing.assert_array_equal(rd.take(8), [0, 3, 2, 1, 0, 3, 2, 1])
    np.testing.assert_array_equal(rd.take(4), [0, 1, 0, 1])
    cases = 0
    for V in (4, 2):
        for head in range(V):
            for W in (6, 7):
                for nv in (0, 1, 23, 63, 64):
                    valid = nv * W
                    cnt, fw = rd.take(valid), rd.take(valid)
                    vec, scalar, lo, hi, lds_max, misaligned = rd.take(6)
                    what = f"V={V} head={head} W={W} nv={nv}"
                    assert (cnt == 1).all(), what                                    # every word of [0, valid) exactly once
                    q = np.arange(valid)
                    np.testing.assert_array_equal(fw, (q // W) * 1000 + q % W, err_msg=what)   # to the right (filter, word)
                    assert lo == 0 and hi == valid - 1, what                          # no index below 0, none at or beyond valid
                    assert misaligned == 0 and vec * V + scalar == valid, what
                    # word by word: the head and the ragged tail only
                    body = max(valid - min(head, valid), 0)
                    assert scalar == min(head, valid) + body % V and vec == body // V, what
                    assert lds_max == (-1 if valid == 0 else (nv - 1) * 7 + W - 1) and lds_max < 64 * 7, what
                    cases += 1
    assert cases == (4 + 2) * 2 * 5


def test_plan_puts_every_tick_in_one_chunk_entry(harness):
    rd = _Reader(harness)
    rd.take(12 + sum(2 * nv * W + 6 for V in (4, 2) for _ in range(V) for W in (6, 7) for nv in (0, 1, 23, 63, 64)))
    tagged = {0, 3, 31, 32, 33, 64, 69}
    for n in (1, 31, 32, 33, 70):
        for t0 in (0, 5):
            for pat in range(3):
                has = (lambda t: False, lambda t: True, lambda t: t in tagged)[pat]
                chunks, chunks_fn, m = rd.take(3)
                assert chunks == chunks_fn == -(-n // 32)
                ticks, zs = [], []
                for c in range(chunks):
                    k0, count = rd.take(2)
                    assert k0 == 32 * c and count == min(32, n - 32 * c)
                    e = rd.take(2 * count).reshape(count, 2)
                    ticks += list(e[:, 0]); zs += list(e[:, 1])
                assert ticks == list(range(t0, t0 + n)), (n, t0, pat)          # every tick in exactly one entry, in order
                want, slot = [], 0
                for t in range(t0, t0 + n):
                    want.append(slot if has(t) else -1)
                    slot += bool(has(t))
                assert zs == want and m == slot, (n, t0, pat)
    assert rd.take(1)[0] == sequence.CHUNK
    assert rd.p == harness.size


# ---------------------------------------------------------------- DeviceIO.sequence / run argument checks (no GPU call is reached)
class FakeParams:
    multirate_ekf = 0


class FakeEkf(side_lib_util.FakeEkf):
    params = FakeParams()


def _fake_seq(io, K, ticks):
    s = sequence.DeviceSequence.__new__(sequence.DeviceSequence)
    s.io, s.n_ticks, s.meas_ticks, s.inputs = io, K, list(ticks), object()
    return s


def test_sequence_and_run_refuse_before_any_gpu_call(monkeypatch):
    boom = forbid_native(monkeypatch)
    monkeypatch.setattr(FakeEkf, "make_inputs", boom, raising=False)
    io = devio.DeviceIO(FakeEkf())
    B, K = 100, 40
    T = FakeTensor
    u = T((K, B, 6))
    z3, m3 = T((3, B, 7)), T((3, B), dtype="uint8")
    bad = [
        dict(u_seq=np.zeros((K, B, 6), np.float32)),                         # a host array
        dict(u_seq=T((B, 6))),                                               # one tick: not a sequence
        dict(u_seq=T((K, B, 7))),
        dict(u_seq=T((K, B + 1, 6))),
        dict(u_seq=T((K, B, 6), dtype="float16")),
        dict(u_seq=T((K, B, 6), device="cuda:1")),
        dict(u_seq=T((K, B, 6), contiguous=False)),
        dict(u_seq=T((K, B, 6), ptr=0x7F0000000008)),                        # base not 16-byte aligned
        dict(u_seq=u, z_seq=z3, meas_ticks=[5, 3, 9]),                       # unsorted
        dict(u_seq=u, z_seq=z3, meas_ticks=[3, 3, 9]),                       # not strictly increasing
        dict(u_seq=u, z_seq=z3, meas_ticks=[3, 9, K]),                       # out of range
        dict(u_seq=u, z_seq=z3, meas_ticks=[-1, 3, 9]),
        dict(u_seq=u, z_seq=z3, meas_ticks=[3, 9]),                          # M mismatch: z_seq holds 3
        dict(u_seq=u, z_seq=z3, meas_ticks=[1, 3, 9, 11]),
        dict(u_seq=u, meas_ticks=[3, 9]),                                    # tag ticks without z_seq
        dict(u_seq=u, z_seq=z3),                                             # z_seq without tag ticks
        dict(u_seq=u, mask_seq=m3, meas_ticks=[1, 3, 9]),                    # mask_seq without z_seq
        dict(u_seq=u, z_seq=z3, mask_seq=T((2, B), dtype="uint8"), meas_ticks=[1, 3, 9]),
        dict(u_seq=u, z_seq=z3, mask_seq=T((3, B), dtype="float32"), meas_ticks=[1, 3, 9]),
        dict(u_seq=u, z_seq=z3, mask_seq=T((3, B), dtype="bool", contiguous=False), meas_ticks=[1, 3, 9]),
        dict(u_seq=u, z_seq=T((3, B, 7), dtype="float64"), meas_ticks=[1, 3, 9]),   # u and z of different dtypes
        dict(u_seq=u, z_seq=T((3, B, 6)), meas_ticks=[1, 3, 9]),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            io.sequence(**kw)
    # a good call gets as far as creating the sequence
    with pytest.raises(AssertionError, match="native library"):
        io.sequence(u, z3, [1, 3, 9], m3)

    seq = _fake_seq(io, K, [1, 3, 9])
    # a refill checks the window: its own m, and the end of the sequence
    with pytest.raises(ValueError):
        seq.pack(T((10, B, 6)), T((3, B, 7)), t0=2)          # ticks [2, 12) hold two tag slots
    with pytest.raises(ValueError):
        seq.pack(T((10, B, 6)), T((2, B, 7)), t0=K - 5)      # beyond the end
    with pytest.raises(AssertionError, match="native library"):
        seq.pack(T((10, B, 6)), T((2, B, 7)), t0=2)
    x8 = T((8, B, 16))
    bad_run = [
        dict(seq=object()),
        dict(seq=_fake_seq(devio.DeviceIO(FakeEkf()), K, [])),               # another handle's sequence
        dict(seq=seq, t0=-1),
        dict(seq=seq, t0=10, n=K),
        dict(seq=seq, chi2_max=0.0),
        dict(seq=seq, chi2_max=-3.0),
        dict(seq=seq, chi2_max=float("nan")),
        dict(seq=seq, return_nis=True),                                      # without a gate
        dict(seq=seq, trace=("nees",)),                                      # trace kinds without trace_every
        dict(seq=seq, x_true_seq=x8),
        dict(seq=seq, trace_every=0),
        dict(seq=seq, trace_every=2.5),
        dict(seq=seq, trace_every=5, trace=("report", "state")),
        dict(seq=seq, trace_every=5, trace=()),
        dict(seq=seq, trace_every=5, trace=("nees",)),                       # no truth
        dict(seq=seq, trace_every=5, x_true_seq=x8),                         # a truth without "nees"
        dict(seq=seq, trace_every=5, trace=("nees",), x_true_seq=T((7, B, 16))),   # J = 40 // 5 = 8
        dict(seq=seq, trace_every=5, trace=("nees",), x_true_seq=T((8, B, 15))),
        dict(seq=seq, trace_every=5, trace=("nees",), x_true_seq=x8, blocks="nonsense"),
        dict(seq=seq, trace_every=5, trace=("nees",), x_true_seq=x8, chi2_hi=0.0),
        dict(seq=seq, trace_every=5, dtype="int32"),
    ]
    for kw in bad_run:
        with pytest.raises(ValueError):
            io.run(**kw)
    with pytest.raises(AssertionError, match="native library"):
        io.run(seq, trace_every=5, trace=("report", "nees"), x_true_seq=x8, chi2_max=16.81, return_nis=True)
    # the gate's own rule
    class MrEkf(FakeEkf):
        params = type("P", (), {"multirate_ekf": 1})()
    mio = devio.DeviceIO(MrEkf())
    with pytest.raises(_lib.QleError) as e:
        mio.run(_fake_seq(mio, K, [1]), chi2_max=16.81)
    assert e.value.code == _lib.QLE_ERR_STATE


def _opts(**kw):
    o = sequence.QsqRunOpts()
    o.struct_size = C.sizeof(o)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_native_entries_refuse_before_any_gpu_call(sequence_so):
    """Without a GPU a HIP call fails as QLE_ERR_HIP / QLE_ERR_NO_DEVICE: every refusal here is QLE_ERR_INVALID with its own message."""
    S = sequence.sequence_lib()
    v = _view()
    u = C.c_void_p(0x7F0000100000)
    assert S.qsq_pack(None, None, 0, 1, u, None, None, 0) == _lib.QLE_ERR_INVALID
    assert S.qsq_pack(C.byref(v), None, 0, 1, u, None, None, 0) == _lib.QLE_ERR_INVALID and b"inputs is null" in S.qsq_last_error()
    assert S.qsq_pack(C.byref(v), None, 0, 1, u, None, None, 7) == _lib.QLE_ERR_INVALID and b"src_dtype" in S.qsq_last_error()
    assert S.qsq_pack(C.byref(v), None, -1, 1, u, None, None, 0) == _lib.QLE_ERR_INVALID
    v.struct_size -= 8
    assert S.qsq_pack(C.byref(v), None, 0, 1, u, None, None, 0) == _lib.QLE_ERR_INVALID and b"struct_size" in S.qsq_last_error()
    assert S.qsq_run(None, None, 0, 1, None) == _lib.QLE_ERR_INVALID and b"handle is null" in S.qsq_last_error()
