"""CPU tests of the filter banks (include/qle_bank.h, libqle_bank.so, quadrotor_landing_amd/bank.py, csrc/ekf_bank.hpp): the library
builds, exports and binds what its header declares, its four kernels are its own, it needs no other library of the project, its generated
code passes the stale-EXEC audit and uses no scratch memory and no LDS, every refusal is made before any GPU call (without a GPU a HIP
call would fail with another error class), and the arithmetic of k_bank_fuse -- compiled for the host with g++, once plain and once as a
stand-alone program under AddressSanitizer and UBSan, with the butterfly restated as the same tree over an array -- agrees with the numpy
restatement `bank_util.fuse_ref`, which is itself pinned by an independent form.

What the host build covers: bank_member_valid, bank_weight_raw, bank_diff, bank_fuse_state, bank_cov_term and the word table.  What it
does not: the kernel's loads and stores, its shuffles and where a bank's record lands; tests/test_gpu_bank.py holds those.

Measured deviations of the host-compiled arithmetic from the truth (printed per case, `pytest -s`) and the stated tolerances:
tests/tolerances_bank.md.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import bank_util as bu
import host_harness
import side_lib_util
from elf_util import _kernels, _needed
from quadrotor_landing_amd import _lib, bank, devio
from side_lib_util import FakeTensor, assert_audit_counts, assert_exports_and_binds, ensure_built, kernel_descriptors, run_audit, scratch_free
from util import forbid_native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qle_bank.h")
N_KERNELS = 4   # k_bank_fuse: T x COMPACT


@pytest.fixture(scope="module")
def bank_so():
    return ensure_built("bank")


# ---------------------------------------------------------------- 1. header, exports, kernels, audit, resources
def test_library_exports_and_binds_every_declared_function(bank_so):
    _, txt = assert_exports_and_binds(bank, HEADER, "qbk", bank_so,
                                      ["qbk_fuse", "qbk_fuse_host", "qbk_last_error", "qbk_launch_census_begin", "qbk_launch_census_end", "qbk_launch_count", "qbk_workspace_bytes"])
    assert int(re.search(r"#define QBK_MAX_MEMBERS (\d+)", txt).group(1)) == bank.MAX_MEMBERS == 64


def test_kernels_are_its_own_and_exactly_four(bank_so):
    mine, main = _kernels(bank_so), _kernels(_lib.LIB_PATH)
    assert mine and main and not mine & main, sorted(mine & main)
    ids = {_lib.demangle(m) for m in mine}
    assert all(i.startswith("void qle::k_bank_fuse<") for i in ids), sorted(ids)
    assert len(ids) == N_KERNELS
    assert {re.match(r"void qle::k_bank_fuse<(\w+), (\w+)>", i).groups() for i in ids} == {(t, c) for t in ("float", "double") for c in ("true", "false")}
    assert not any("k_bank" in _lib.demangle(m) for m in main)


def test_library_links_the_hip_runtime_only(bank_so):
    needed = _needed(bank_so)
    assert any(n.startswith("libamdhip64") for n in needed), needed
    assert not any("qle_" in n for n in needed), needed
    assert not re.findall(rb"libqle_[a-z]+\.so", open(bank_so, "rb").read())


@pytest.fixture(scope="module")
def audit(bank_so):
    return run_audit("bank")


def test_generated_device_code_passes_the_stale_exec_audit(audit):
    assert_audit_counts(audit[0], "bank", N_KERNELS)


def test_no_kernel_uses_scratch_memory_or_lds(audit):
    """The kernel descriptors of the generated assembly: 0 bytes of private segment and no LDS for all four, and a register count that
    leaves room for at least two waves per SIMD (P is streamed: nowhere near the 240 registers of a resident fp64 covariance)."""
    r, asm = audit
    assert r.returncode == 0
    found, meta = kernel_descriptors(asm)
    assert len(found) == N_KERNELS and all("k_bank_fuse<" in k for k in found), sorted(found)
    for name, (scratch, lds, vgpr) in found.items():
        print(f"{name.split('(')[0]}: scratch {scratch} B, LDS {lds} B, registers {vgpr}")
        assert scratch == 0, (name, scratch)
        assert lds == 0, (name, lds)
        assert vgpr <= 256, (name, vgpr)
    assert scratch_free(meta), meta


# ---------------------------------------------------------------- 2. refusals, before any GPU call
_view = functools.partial(side_lib_util._view, batch=128)


def test_library_refuses_before_any_gpu_call(bank_so):
    """No GPU here: a call that got as far as the HIP runtime would return QLE_ERR_HIP (or crash on the fake pointers), not these."""
    K = bank.bank_lib()
    B = C.byref
    INV = _lib.QLE_ERR_INVALID
    v, fused = _view(), _lib.QleDeviceView()
    need = K.qbk_workspace_bytes(B(v), 4)
    assert need == 64 * 144 * 4                                               # 32 banks: one tile
    assert K.qbk_workspace_bytes(B(_view(batch=140, dtype=_lib.QLE_F64)), 2) == 128 * 144 * 8   # 70 banks: two tiles
    LW, WS, W, BEST, MK = 0x7F1000000000, 0x7F2000000000, 0x7F3000000000, 0x7F4000000000, 0x7F5000000000
    state_bytes = 128 * 144 * 4

    def call(v_=B(v), M=4, lw=LW, mask=MK, ws=WS, nb=need, fused_=B(fused), w=W, best=BEST):
        return K.qbk_fuse(v_, M, lw, mask, ws, nb, fused_, w, best)

    err = lambda: K.qbk_last_error()
    assert call(v_=None) == INV and b"view" in err()
    for size in (0, C.sizeof(v) - 8, C.sizeof(v) + 8):                      # a wrong struct_size
        bad = _view(); bad.struct_size = size
        assert call(v_=B(bad)) == INV and b"struct_size" in err()
        assert K.qbk_workspace_bytes(B(bad), 4) == INV
    for M in (0, 1, 3, 6, 12, 48, 128, -2, -64, 2 ** 31 - 1, -2 ** 31):      # members not a power of two in 2..64
        assert call(M=M) == INV and b"power of two" in err(), M
        assert K.qbk_workspace_bytes(B(v), M) == INV
    for batch, M in ((100, 8), (140, 64), (130, 4), (2, 4)):                  # batch % members != 0
        assert call(v_=B(_view(batch=batch)), M=M) == INV and b"multiple" in err(), (batch, M)
        assert K.qbk_workspace_bytes(B(_view(batch=batch)), M) == INV
    assert call(lw=None) == INV and b"logw is null" in err()                 # logw == NULL
    odd = _view(); odd.state = 0x7F0000000008                                # misaligned pointers
    assert call(v_=B(odd)) == INV and b"aligned" in err()
    assert call(lw=LW + 4) == INV and b"aligned" in err()
    assert call(w=W + 4) == INV and b"aligned" in err()
    assert call(best=BEST + 2) == INV and b"aligned" in err()
    assert call(ws=WS + 8) == INV and b"aligned" in err()
    assert call(nb=need - 1) == INV and b"too small" in err()                # a workspace that is too small
    assert call(nb=0) == INV and call(ws=None) == INV
    for ws in (v.state, v.state + state_bytes - 16, v.state - need + 16, v.state + 16):   # ... or overlaps view->state
        assert call(ws=ws) == INV and b"overlaps" in err(), hex(ws)
    assert call(ws=v.state - 4 * need, nb=4 * need + state_bytes + 16) == INV and b"overlaps" in err()   # a larger workspace around the state
    assert call(fused_=None) == INV and b"fused" in err()
    for wrong in (dict(dtype=7), dict(n=12), dict(batch=0), dict(n=15, compact=1)):
        assert call(v_=B(_view(**wrong))) == INV
    # the host entry refuses the same, before it allocates anything
    lw, w, best = np.zeros(128), np.zeros(128), np.zeros(32, np.int32)
    pl, pw, pb = lw.ctypes.data_as(C.POINTER(C.c_double)), w.ctypes.data_as(C.POINTER(C.c_double)), best.ctypes.data_as(C.POINTER(C.c_int32))
    host = lambda M=4, ws=WS, nb=need, lw_=pl, v_=B(v): K.qbk_fuse_host(v_, M, lw_, None, ws, nb, B(fused), pw, pb)
    assert host(M=3) == INV and host(M=128) == INV and host(nb=need - 1) == INV and host(ws=v.state) == INV and host(ws=WS + 4) == INV
    assert host(lw_=None) == INV and host(v_=B(_view(batch=100)), M=8) == INV and host(v_=None) == INV
    assert K.qbk_launch_count() == 0


class FakeEkf:
    batch, dtype, device, num_states = 128, _lib.QLE_F32, 0, 15
    _h = None


def test_python_refuses_a_bad_geometry_before_any_native_call(monkeypatch):
    forbid_native(monkeypatch)
    io = devio.DeviceIO(FakeEkf())
    for bad in (0, 1, 3, 6, 48, 128, -4, 2.5, 4.0 + 1e-9, True, "4", None):
        with pytest.raises(ValueError):
            io.bank(bad)
        with pytest.raises(ValueError):
            bank.Bank(io, bad)
        with pytest.raises(ValueError):
            bank.Fused(io, _lib.QleDeviceView(), None, bad, None, None)
    small = devio.DeviceIO(FakeEkf()); small.ekf.batch = 100                 # B % M
    for M in (8, 64):
        with pytest.raises(ValueError, match="multiple"):
            small.bank(M)
        with pytest.raises(ValueError, match="multiple"):
            bank.Fused(small, _lib.QleDeviceView(), None, M, None, None)
    b = io.bank(4)
    assert (b.members, b.banks) == (4, 32)
    lw, m = FakeTensor((128,), dtype="float64"), FakeTensor((128,), dtype="uint8")
    for bad_lw in (np.zeros(128), FakeTensor((128,), dtype="float32"), FakeTensor((127,), dtype="float64"), FakeTensor((128, 1), dtype="float64"),
                   FakeTensor((128,), dtype="float64", device="cuda:1"), FakeTensor((128,), dtype="float64", contiguous=False)):
        with pytest.raises(ValueError):
            b.fuse(bad_lw)
    for bad_m in (np.zeros(128, np.uint8), FakeTensor((128,), dtype="float32"), FakeTensor((32,), dtype="uint8")):
        with pytest.raises(ValueError):
            b.fuse(lw, mask=bad_m)
    with pytest.raises(AssertionError, match="native library"):
        b.fuse(lw, mask=m)   # a good call is what reaches the libraries
    assert not hasattr(bank.Fused, "lookahead")   # not offered: which Q a fused estimate coasts under is a modelling choice


# ---------------------------------------------------------------- 3. the truth, pinned by an independent form
@pytest.mark.parametrize("M,n", [(2, 15), (8, 9), (64, 15)])
def test_truth_is_the_mixture_covariance_where_members_share_a_quaternion(M, n):
    rng = np.random.default_rng(40 + M)
    G = 5
    x, P, logw, mask = bu.make_case(rng, M, G, n, "f64", empty_bank=False)
    qb = rng.normal(size=(G, 4)); qb /= np.linalg.norm(qb, axis=1, keepdims=True)
    has_state = x[:, 6:10].any(axis=1)
    x[has_state, 6:10] = qb.repeat(M, axis=0)[has_state]                      # one quaternion per bank (stateless members stay so)
    ref = bu.fuse_ref(x, P, logw, mask, M)
    worst = 0.0
    for g in range(G):
        s = slice(g * M, (g + 1) * M)
        v = ref.w[s] > 0
        cov, scale = bu.mixture_cov(x[s][v], P[s][v], ref.w[s][v])
        worst = max(worst, float((np.abs(ref.P[g] - cov) / scale).max()))
        q, qr = ref.x[g, 6:10], x[ref.best[g], 6:10]
        assert min(np.abs(q - qr).max(), np.abs(q + qr).max()) < 4e-16       # d_theta = 0: the shared attitude
        assert abs(ref.w[s].sum() - 1.0) < 4e-16
    print(f"M={M} n={n}: fuse_ref against the mixture covariance {worst:.2e} of the sum of absolute terms")
    assert worst < 8 * 2.0 ** -53, worst                                     # a few fp64 roundings


# ---------------------------------------------------------------- 4. the arithmetic on the host, once more under the sanitizers
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/cpp/bank_harness.cpp: the arithmetic of ekf_bank.hpp compiled by g++ (the HIP headers define the device decorators away),
    once as it is and once as a stand-alone program under AddressSanitizer and UBSan."""
    return host_harness.build("bank_harness", tmp_path_factory)


def run_harness(exe, tmp, dtype, compact, M, x, P, logw, mask):
    B, n = x.shape[0], P.shape[1]
    G = B // M
    per = np.concatenate([x, host_harness.full_P(P, compact), logw[:, None], mask[:, None].astype(np.float64)], axis=1)
    o = host_harness.run(exe, tmp, [B, int(dtype == "f64"), int(compact), M], [per], -1)
    w, bank_out = o[:B], o[B:].reshape(G, 242)
    Pf = bank_out[:, 17:].reshape(G, 15, 15)
    assert not Pf[:, n:, :].any() and not Pf[:, :, n:].any()
    return w, bank_out[:, 0].astype(np.int32), bank_out[:, 1:17], Pf[:, :n, :n].copy()


GRID = [(M, d, r) for M in (2, 8, 64) for d in ("f64", "f32") for r in bu.RECORDS]
G_CPU = {2: 70, 8: 11, 64: 3}   # the shapes of tests/test_gpu_bank.py: the worst deviation is taken over as many banks as the GPU test draws


@pytest.mark.parametrize("M,dtype,record", GRID, ids=[f"M{M}-{d}-{r}" for M, d, r in GRID])
def test_host_compiled_arithmetic_matches_the_truth(harness, tmp_path, M, dtype, record):
    n, compact = bu.RECORDS[record]
    rng = np.random.default_rng(1000 + M + n)
    x, P, logw, mask = bu.make_case(rng, M, G_CPU[M], n, dtype)
    ref = bu.fuse_ref(x, P, logw, mask, M)
    assert ref.best[-1] == -1 and (ref.best[:-1] >= 0).all()
    live = ref.w > 0
    assert ref.w[live].min() > 1e-3 / M                                      # no member is weighted away
    for exe in harness:
        w, best, xf, Pf = run_harness(exe, tmp_path, dtype, compact, M, x, P, logw, mask)
        np.testing.assert_array_equal(best, ref.best)                        # exact: best, the zero weights, the empty bank's record
        np.testing.assert_array_equal(w == 0, ref.w == 0)
        assert not xf[-1].any() and not Pf[-1].any() and not w[-M:].any()
        assert np.array_equal(Pf, Pf.transpose(0, 2, 1)) and np.isfinite(xf).all() and np.isfinite(Pf).all()
        dev = bu.deviations(w, xf, Pf, ref)
        tol = bu.TOL[dtype]
        print(f"BANK host M={M} {dtype} {record}: " + " ".join(f"{k} {v:.2e} ({v / tol[k]:.3f} of {tol[k]:.0e})" for k, v in dev.items()))
        assert all(dev[k] <= tol[k] for k in dev), (dev, tol)
        for g in range(len(best) - 1):
            assert abs(w[g * M:(g + 1) * M].sum() - 1.0) < 4e-16
