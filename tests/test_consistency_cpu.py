"""CPU tests of the consistency diagnostics (include/qle_consistency.h, libqle_consistency.so, quadrotor_landing_amd/consistency.py,
csrc/ekf_consistency.hpp): the library builds, exports and binds what its header declares, its kernels are its own (none shared with,
none added to, the three existing libraries), its generated code passes the stale-EXEC audit and uses no scratch memory, every refusal
is made before any GPU call (without a GPU a HIP call would fail with another error class), and the arithmetic of k_nees -- nees_eval,
compiled for the host with g++ -- agrees with numpy's dense solve on the sliced marginal for every block selection.

Reference and tolerance: consistency_util.py (|nees - ref| <= 16 n kappa(C_i) u ref per filter; err to 8 u of its block's norm, the
attitude block to 8 u pi).  What the host build does not cover are the kernel's loads and its batch summary: tests/test_gpu_consistency.py.

Measured worst deviation / tolerance of the host-compiled arithmetic (B = 300 per case, every block selection; must be <= 1):
  fp64: nees 0.065 (n = 15), 0.052 (n = 9, full and compact);  err 0.24 / 0.32
  fp32: nees 0.060 (n = 15), 0.21 (n = 9, full and compact);   err 0.14 / 0.16
(tests/tolerances_consistency.md holds the table).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import consistency_util as cu
import host_harness
from elf_util import _kernels
from quadrotor_landing_amd import _lib, consistency, devio, gate
from side_lib_util import FakeTensor, _params, _view, assert_audit_counts, assert_exports_and_binds, ensure_built, kernel_descriptors, run_audit, scratch_free
from util import forbid_native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qle_consistency.h")
AB_STATIC, WB_STATIC = np.array([0.2, -0.09, -0.03]), np.array([-0.02, -0.01, 0.003])


@pytest.fixture(scope="module")
def cons_so():
    return ensure_built("consistency")


def test_library_exports_and_binds_every_declared_function(cons_so):
    assert_exports_and_binds(consistency, HEADER, "qcs", cons_so, ["qcs_last_error", "qcs_launch_census_begin", "qcs_launch_census_end", "qcs_launch_count", "qcs_nees", "qcs_nees_host"])


def test_summary_struct_is_eight_doubles_in_the_header_order():
    txt = open(HEADER).read()
    body = re.search(r"typedef struct qcs_summary \{(.*?)\} qcs_summary;", txt, flags=re.S).group(1)
    fields = re.findall(r"double\s+([a-z_]+);", body)
    assert tuple(fields) == consistency.SUMMARY_FIELDS and C.sizeof(consistency.QcsSummary) == 64


def test_kernels_are_disjoint_from_the_three_existing_libraries(cons_so):
    mine = _kernels(cons_so)
    others = {p: _kernels(p) for p in (_lib.LIB_PATH, devio.DEVIO_LIB_PATH, gate.GATE_LIB_PATH)}
    assert mine and all(others.values())
    for p, k in others.items():
        assert not mine & k, (p, sorted(mine & k))
        assert not any("k_nees" in _lib.demangle(m) for m in k), p
    ids = {_lib.demangle(m) for m in mine}
    assert all(i.startswith("void qle::k_nees<") or i.startswith("qle::k_nees_reduce(") for i in ids), sorted(ids)
    assert len(ids) == 9   # k_nees: T x PFP x COMPACT, and k_nees_reduce


@pytest.fixture(scope="module")
def audit(cons_so):
    return run_audit("consistency")


def test_generated_device_code_passes_the_stale_exec_audit(audit):
    assert_audit_counts(audit[0], "consistency", 9)


def test_no_kernel_uses_scratch_memory(audit):
    """The kernel descriptors of the generated assembly: 0 bytes of private segment for every k_nees instantiation (and the reduce), and
    the register counts the launch bounds promise -- fp32 within the 256 registers that leave room for two waves per SIMD."""
    r, asm = audit
    assert r.returncode == 0
    found, meta = kernel_descriptors(asm)
    nees = {k: v for k, v in found.items() if "k_nees<" in k}
    assert len(nees) == 8 and len(found) == 9, sorted(found)
    for name, (scratch, _, vgpr) in found.items():
        print(f"{name.split('(')[0]}: scratch {scratch} B, registers {vgpr}")
        assert scratch == 0, (name, scratch)
        assert vgpr <= (256 if "k_nees<float" in name else 512), (name, vgpr)
    assert scratch_free(meta), meta


# ---------------------------------------------------------------- refusals, before any GPU call
def test_library_refuses_before_any_gpu_call(cons_so):
    """No GPU here: a call that got as far as the HIP runtime would return QLE_ERR_HIP (or crash on the fake pointers), not these."""
    K = consistency.consistency_lib()
    v, p = _view(), _params()
    xt, out = 0x7F1000000000, 0x7F3000000000
    B = C.byref
    INV = _lib.QLE_ERR_INVALID

    def call(v_=B(v), p_=B(p), xt_=xt, td=consistency.QCS_F32, blocks=31, chi2=25.0, nees=out, err=None, summ=out + 4096, dd=consistency.QCS_F32):
        return K.qcs_nees(v_, p_, xt_, td, None, blocks, chi2, nees, err, summ, dd)

    assert call(v_=None) == INV and b"view" in K.qcs_last_error()
    assert call(p_=None) == INV and call(xt_=None) == INV
    short = _view(); short.struct_size = C.sizeof(short) - 8
    assert call(v_=B(short)) == INV and b"struct_size" in K.qcs_last_error()
    for blocks in (0, 32, 63, 1 << 8):
        assert call(blocks=blocks) == INV and b"blocks" in K.qcs_last_error()
    nine_v, nine_p = _view(n=9), _params(est_bias=0)
    for blocks in (8, 16, 31, 1 | 8):
        assert call(v_=B(nine_v), p_=B(nine_p), blocks=blocks) == INV and b"bias block" in K.qcs_last_error()
    for bad in (0.0, -1.0, float("nan"), float("-inf")):
        assert call(chi2=bad) == INV and b"chi2_hi" in K.qcs_last_error()
    assert call(td=7) == INV and call(dd=7) == INV
    assert call(xt_=xt + 8) == INV and b"aligned" in K.qcs_last_error()
    assert call(nees=out + 2) == INV and call(err=out + 1) == INV and call(summ=out + 4) == INV
    assert call(nees=out + 4, dd=consistency.QCS_F64) == INV
    assert call(p_=B(nine_p)) == INV   # the view says 15 states
    # the host entry refuses the same, before it allocates anything
    hx = np.zeros((100, 16)); hn = np.zeros(100); s = consistency.QcsSummary()
    hp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    host = lambda v_, p_, blocks, chi2: K.qcs_nees_host(v_, p_, hp(hx), None, blocks, chi2, hp(hn), None, B(s))
    assert host(B(v), B(p), 0, 25.0) == INV and host(B(v), B(p), 31, 0.0) == INV and host(B(short), B(p), 31, 25.0) == INV
    assert host(B(nine_v), B(nine_p), 8, 25.0) == INV and host(None, B(p), 31, 25.0) == INV
    assert K.qcs_launch_count() == 0


class FakeEkf:
    batch, dtype, device = 100, _lib.QLE_F32, 0
    _h = None

    def __init__(self, num_states=15, **kw):
        self.num_states = num_states
        self.params = _params(**kw)


def test_deviceio_refuses_bad_nees_arguments_before_any_gpu_call(monkeypatch):
    ekf, ekf9 = FakeEkf(), FakeEkf(num_states=9, est_bias=0)   # their parameters come from the tick library: made first
    forbid_native(monkeypatch)
    B = 100
    io = devio.DeviceIO(ekf)
    xt = FakeTensor((B, 16))
    bad = [
        dict(x_true=np.zeros((B, 16))),                               # a host array
        dict(x_true=FakeTensor((B, 15))),
        dict(x_true=FakeTensor((B, 16), dtype="float16")),
        dict(x_true=FakeTensor((B, 16), device="cuda:1")),
        dict(x_true=FakeTensor((B, 16), contiguous=False)),
        dict(x_true=FakeTensor((B, 16), ptr=0x7F0000000008)),         # not 16-byte aligned
        dict(x_true=xt, mask=FakeTensor((B,), dtype="float32")),
        dict(x_true=xt, mask=FakeTensor((B, 1), dtype="uint8")),
        dict(x_true=xt, blocks=0),
        dict(x_true=xt, blocks=32),
        dict(x_true=xt, blocks=""),
        dict(x_true=xt, blocks="pose+yaw"),
        dict(x_true=xt, chi2_hi=0.0),
        dict(x_true=xt, chi2_hi=float("nan")),
        dict(x_true=xt, dtype="int32"),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            io.nees(**kw)
    nine = devio.DeviceIO(ekf9)
    for blocks in ("ab", "r+wb", 8, 31):
        with pytest.raises(ValueError, match="bias block"):
            nine.nees(xt, blocks=blocks)
    with pytest.raises(AssertionError, match="native library"):
        io.nees(xt, blocks="pose", chi2_hi=12.6)   # a good call is what reaches the libraries
    with pytest.raises(AssertionError, match="native library"):
        nine.nees(xt)                              # "all" means the blocks the handle has


def test_block_names():
    bm = consistency.block_mask
    assert bm("all") == 31 and bm("all", 9) == 7 and bm("pose") == 5 and bm("r") == 1 and bm("theta") == 4 and bm("th") == 4
    assert bm("r+theta+ab+wb") == 29 and bm("r, v") == 3 and bm(("r", "wb")) == 17 and bm(29) == 29 and bm("bias") == 24
    assert {k: bm(k) for k in cu.NAMED_BLOCKS} == cu.NAMED_BLOCKS


# ---------------------------------------------------------------- the arithmetic on the host
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/cpp/consistency_harness.cpp: ekf_consistency.hpp's nees_eval compiled by g++ (the HIP headers define the device decorators away),
    once as it is and once as a stand-alone program under AddressSanitizer and UBSan."""
    return host_harness.build("consistency_harness", tmp_path_factory)


def run_harness(exe, tmp, dtype, compact, blocks, x, P, xt, ab, wb):
    B, n = x.shape[0], P.shape[1]
    per = np.concatenate([x, host_harness.full_P(P), xt, np.broadcast_to(ab, (B, 3)), np.broadcast_to(wb, (B, 3))], axis=1)
    o = host_harness.run(exe, tmp, [B, int(dtype == "f64"), int(compact), blocks], [per], (B, 17))
    return o[:, 0], o[:, 1] != 0, o[:, 2:2 + n]


CASES = [("f64", 15, False), ("f64", 9, False), ("f64", 9, True), ("f32", 15, False), ("f32", 9, False), ("f32", 9, True)]


@pytest.fixture(scope="module")
def cases():
    """One construction per (dtype, n), shared by every block selection and left unchanged."""
    out = {}
    for dtype in ("f64", "f32"):
        for n in (15, 9):
            rng = np.random.default_rng(1200 + n + (dtype == "f32"))
            r32 = (lambda a: a.astype(np.float32).astype(np.float64)) if dtype == "f32" else (lambda a: a)
            ab = r32(AB_STATIC + 0.05 * rng.normal(size=(300, 3))); wb = r32(WB_STATIC + 0.005 * rng.normal(size=(300, 3)))
            x, P, xt = cu.make_case(rng, 300, n, dtype, ab, wb)
            kap = cu.kappa_scaled(P)
            assert kap.max() <= cu.KAPPA_MAX and kap.max() > 30.0   # the construction reaches the conditioning it promises
            out[dtype, n] = (x, P, xt, ab, wb, cu.err_ref(x, xt, ab, wb, n))
    return out


@pytest.mark.parametrize("dtype,n,compact", CASES, ids=[f"{d}-n{n}-{'compact' if c else 'full'}" for d, n, c in CASES])
def test_host_compiled_arithmetic_matches_the_dense_solve_on_every_marginal(harness, cases, tmp_path, dtype, n, compact):
    x, P, xt, ab, wb, eref = cases[dtype, n]
    big, neg = np.arange(300) % 8 == 3, np.arange(300) % 8 == 5
    ang = np.degrees(np.linalg.norm(eref[:, 6:9], axis=1))
    assert ang[big].max() > 160.0 and (xt[neg, 9] < 0).all()
    worst_n = worst_e = 0.0
    for blocks in range(1, 32 if n == 15 else 8):
        ref = cu.nees_ref(P, eref, blocks)
        for exe in harness:                  # the plain build, then the same file under ASan + UBSan
            nees, pd, err = run_harness(exe, tmp_path, dtype, compact, blocks, x, P, xt, ab, wb)
            assert pd.all() and np.isfinite(nees).all()
            rn, re_ = cu.nees_ratio(nees, ref, P, dtype), cu.err_ratio(err, eref, dtype)
            worst_n, worst_e = max(worst_n, rn), max(worst_e, re_)
            assert rn <= 1.0, (blocks, rn)       # every filter of every selection: nothing is left out
            assert re_ <= 1.0, (blocks, re_)
    print(f"{dtype} n={n} compact={compact}: worst |nees - ref| / tol {worst_n:.3g}, worst err deviation / bar {worst_e:.3g}")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_indefinite_covariance_gives_nan_and_is_flagged(harness, cases, tmp_path, dtype):
    x, P, xt, ab, wb, eref = (a[:8].copy() for a in cases[dtype, 15])
    P0 = P.copy()
    P[3, 4, 4] = -P[3, 4, 4]     # a negative diagonal entry in the velocity block
    for exe in harness:
        nees, pd, _ = run_harness(exe, tmp_path, dtype, False, 31, x, P, xt, ab, wb)
        assert np.isnan(nees[3]) and np.isfinite(np.delete(nees, 3)).all()
        assert (~pd).sum() == 1 and not pd[3]                                  # n_not_pd = 1
        # the marginal that leaves the bad block out is positive definite again
        nees, pd, _ = run_harness(exe, tmp_path, dtype, False, 31 & ~2, x, P, xt, ab, wb)
        assert pd.all() and cu.nees_ratio(nees, cu.nees_ref(P, eref, 29), P0, dtype) <= 1.0
