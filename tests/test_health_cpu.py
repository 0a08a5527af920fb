"""CPU tests of the filter lifecycle (include/qle_health.h, libqle_health.so, quadrotor_landing_amd/health.py, csrc/ekf_health.hpp, and
qle_initialize_state_slot of the tick library): the library builds, exports and binds what its header declares, its kernels are its own
(none shared with, none added to, the four existing libraries), its generated code passes the stale-EXEC audit and uses no scratch
memory, every refusal is made before any GPU call (without a GPU a HIP call would fail with another error class), and the per-filter
classification of k_health -- health_classify, compiled for the host with g++ -- gives the status bytes of a numpy restatement.

Reference: health_util.py.  Every comparison is exact: a status byte is right or wrong.  What the host build does not cover are the
kernel's loads, its masks and its batch summary: tests/test_gpu_lifecycle.py.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import health_util as hu
import host_harness
from elf_util import _kernels, _needed
from quadrotor_landing_amd import _lib, consistency, devio, gate, health
from side_lib_util import (FakeEkf, FakeTensor, _view, assert_audit_counts, assert_exports_and_binds, ensure_built, kernel_descriptors, run_audit,
                           scratch_free)
from util import forbid_native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qle_health.h")
N_KERNELS = 10   # k_health: T x {compact, full n = 9, full n = 15}; k_health_reduce; k_retire: T; k_and_masks


@pytest.fixture(scope="module")
def health_so():
    return ensure_built("health")


def test_library_exports_and_binds_every_declared_function(health_so):
    assert_exports_and_binds(health, HEADER, "qhl", health_so,
                             ["qhl_and_masks", "qhl_health", "qhl_health_host", "qhl_last_error", "qhl_launch_census_begin", "qhl_launch_census_end", "qhl_launch_count", "qhl_retire"])


def test_seed_from_a_slot_is_exported_from_the_tick_library():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qle_ekf.h")).read(), flags=re.S)
    assert re.search(r"int qle_initialize_state_slot\(qle_batch \*h, const qle_inputs \*in, int64_t t, int32_t reinit_bias\);", txt)
    L = C.CDLL(_lib.LIB_PATH)
    assert hasattr(L, "qle_initialize_state_slot") and "qle_initialize_state_slot" in _lib.SYMBOLS
    # refusals that need no GPU: a null handle, and (before any launch) nothing else can be reached without one
    fn = _lib.lib().qle_initialize_state_slot
    assert fn(None, None, 0, 0) == _lib.QLE_ERR_INVALID


def test_summary_struct_is_nine_doubles_in_the_header_order():
    txt = open(HEADER).read()
    body = re.search(r"typedef struct qhl_summary \{(.*?)\} qhl_summary;", txt, flags=re.S).group(1)
    fields = re.findall(r"double\s+([a-z_]+);", body)
    assert tuple(fields) == health.SUMMARY_FIELDS and len(fields) == 9 and C.sizeof(health.QhlSummary) == 72
    body = re.search(r"typedef struct qhl_limits \{(.*?)\} qhl_limits;", txt, flags=re.S).group(1)
    assert re.findall(r"(?:uint32_t|double)\s+([a-z_]+);", body) == [n for n, _ in health.QhlLimits._fields_]
    for name, bit in health.BITS.items():
        assert re.search(rf"#define QHL_{name.upper()} {bit}u", txt), name
    assert health.ALL == sum(health.BITS.values()) == 63
    assert (hu.NONFINITE, hu.NOT_PD, hu.QNORM, hu.SIGMA_R, hu.SIGMA_V, hu.SIGMA_THETA) == tuple(health.BITS.values())


def test_kernels_are_disjoint_from_the_four_existing_libraries(health_so):
    mine = _kernels(health_so)
    others = {p: _kernels(p) for p in (_lib.LIB_PATH, devio.DEVIO_LIB_PATH, gate.GATE_LIB_PATH, consistency.CONSISTENCY_LIB_PATH)}
    assert mine and all(others.values())
    fams = ("k_health", "k_retire", "k_and_masks")
    for p, k in others.items():
        assert not mine & k, (p, sorted(mine & k))
        assert not any(f in _lib.demangle(m) for m in k for f in fams), p
    ids = {_lib.demangle(m) for m in mine}
    assert all(i.startswith(("void qle::k_health<", "qle::k_health_reduce(", "void qle::k_retire<", "qle::k_and_masks(")) for i in ids), sorted(ids)
    assert len(ids) == N_KERNELS


def test_library_links_the_hip_runtime_only(health_so):
    needed = _needed(health_so)
    assert any(n.startswith("libamdhip64") for n in needed), needed
    assert not any("qle_" in n or "oracle" in n for n in needed), needed


@pytest.fixture(scope="module")
def audit(health_so):
    return run_audit("health")


def test_generated_device_code_passes_the_stale_exec_audit(audit):
    assert_audit_counts(audit[0], "health", N_KERNELS)


def test_no_kernel_uses_scratch_memory(audit):
    """The kernel descriptors of the generated assembly: 0 bytes of private segment for every kernel, no LDS for the per-filter part
    (k_health_reduce alone keeps its 2 KiB of slices there), and the register counts the launch bounds promise -- fp32 within the 256
    registers that leave room for two waves per SIMD."""
    r, asm = audit
    assert r.returncode == 0
    found, meta = kernel_descriptors(asm)
    assert len([k for k in found if "k_health<" in k]) == 6 and len(found) == N_KERNELS, sorted(found)
    for name, (scratch, lds, vgpr) in found.items():
        print(f"{name.split('(')[0]}: scratch {scratch} B, LDS {lds} B, registers {vgpr}")
        assert scratch == 0, (name, scratch)
        assert lds == (2048 if "k_health_reduce" in name else 0), (name, lds)
        assert vgpr <= (256 if "k_health<float" in name else 512), (name, vgpr)
    assert scratch_free(meta), meta


# ---------------------------------------------------------------- refusals, before any GPU call
def test_library_refuses_before_any_gpu_call(health_so):
    """No GPU here: a call that got as far as the HIP runtime would return QLE_ERR_HIP (or crash on the fake pointers), not these."""
    H = health.health_lib()
    v, lim = _view(), health.make_limits()
    out = 0x7F3000000000
    B = C.byref
    INV = _lib.QLE_ERR_INVALID

    def call(v_=B(v), l_=B(lim), mask=None, status=out, flagged=out + 4096, summ=out + 8192):
        return H.qhl_health(v_, l_, mask, status, flagged, summ)

    assert call(v_=None) == INV and b"view" in H.qhl_last_error()
    assert call(l_=None) == INV and b"limits" in H.qhl_last_error()
    short = _view(); short.struct_size = C.sizeof(short) - 8
    assert call(v_=B(short)) == INV and b"struct_size" in H.qhl_last_error()
    for size in (0, C.sizeof(lim) - 8, C.sizeof(lim) + 8):
        bad = health.make_limits(); bad.struct_size = size
        assert call(l_=B(bad)) == INV and b"struct_size" in H.qhl_last_error()
    for select in (0, 64, 127, 1 << 8):
        bad = health.make_limits(); bad.select = select
        assert call(l_=B(bad)) == INV and b"select" in H.qhl_last_error()
    for field in ("sigma_r_max", "sigma_v_max", "sigma_theta_max", "qnorm_tol"):
        for val in (0.0, -1.0, float("nan"), float("-inf")):
            bad = health.make_limits(); setattr(bad, field, val)
            assert call(l_=B(bad)) == INV and field.encode() in H.qhl_last_error(), (field, val)
    assert call(summ=out + 4) == INV and b"aligned" in H.qhl_last_error()
    odd = _view(); odd.state = 0x7F0000000008
    assert call(v_=B(odd)) == INV and b"aligned" in H.qhl_last_error()
    for wrong in (dict(dtype=7), dict(n=12), dict(batch=0)):
        assert call(v_=B(_view(**wrong))) == INV
    # retire and the mask product
    assert H.qhl_retire(None, out) == INV and H.qhl_retire(B(short), out) == INV
    assert H.qhl_retire(B(v), None) == INV and b"mask" in H.qhl_last_error()
    assert H.qhl_and_masks(B(v), None, out, out) == INV and H.qhl_and_masks(B(v), out, None, out) == INV
    assert H.qhl_and_masks(B(v), out, out, None) == INV and H.qhl_and_masks(B(short), out, out, out) == INV
    # the host entry refuses the same, before it allocates anything
    st = np.zeros(100, np.uint8); s = health.QhlSummary()
    p8 = st.ctypes.data_as(C.POINTER(C.c_uint8))
    bad = health.make_limits(); bad.select = 0
    assert H.qhl_health_host(B(v), B(bad), None, p8, None, B(s)) == INV and H.qhl_health_host(B(short), B(lim), None, p8, None, B(s)) == INV
    assert H.qhl_health_host(None, B(lim), None, p8, None, B(s)) == INV
    assert H.qhl_launch_count() == 0


def test_deviceio_refuses_bad_lifecycle_arguments_before_any_gpu_call(monkeypatch):
    forbid_native(monkeypatch)
    B = 100
    io = devio.DeviceIO(FakeEkf())
    z, m = FakeTensor((B, 7)), FakeTensor((B,), dtype="uint8")
    bad_z = [np.zeros((B, 7)), FakeTensor((B, 6)), FakeTensor((B, 7), dtype="float16"), FakeTensor((B, 7), device="cuda:1"),
             FakeTensor((B, 7), device="cpu"), FakeTensor((B, 7), contiguous=False), FakeTensor((B, 7), ptr=0x7F0000000008)]
    bad_m = [np.zeros(B, np.uint8), FakeTensor((B,), dtype="float32"), FakeTensor((B, 1), dtype="uint8"), FakeTensor((B,), dtype="uint8", device="cuda:1"),
             FakeTensor((B,), dtype="bool", contiguous=False)]
    for t in bad_z:
        with pytest.raises(ValueError):
            io.seed(t)
        with pytest.raises(ValueError):
            io.reseed(t, m)
    for t in bad_m:
        with pytest.raises(ValueError):
            io.seed(z, t)
        with pytest.raises(ValueError):
            io.health(mask=t)
        with pytest.raises(ValueError):
            io.retire(t)
        with pytest.raises(ValueError):
            io.reseed(z, t)
    with pytest.raises((ValueError, AttributeError, TypeError)):
        io.retire(None)
    for kw in (dict(sigma_r_max=0.0), dict(sigma_v_max=-1.0), dict(sigma_theta_max=float("nan")), dict(qnorm_tol=0.0), dict(select=0),
               dict(select=64), dict(select=""), dict(select="nonfinite+broken")):
        with pytest.raises(ValueError):
            io.health(**kw)
        with pytest.raises(ValueError):
            io.reseed(z, m, **kw)
    with pytest.raises(ValueError, match="unknown limits"):
        io.reseed(z, m, chi2_max=3.0)
    for good in (lambda: io.seed(z, m), lambda: io.health(mask=m, sigma_r_max=2.0, select="nonfinite+not_pd"), lambda: io.retire(m),
                 lambda: io.reseed(z, m, sigma_theta_max=0.5)):
        with pytest.raises(AssertionError, match="native library"):
            good()   # a good call is what reaches the libraries


def test_select_names():
    sm = health.select_mask
    assert sm(None) == 63 and sm("all") == 63 and sm("nonfinite") == 1 and sm("nonfinite+not_pd") == 3 and sm(("qnorm", "sigma_r")) == 12
    assert sm("sigma_v, sigma_theta") == 48 and sm(5) == 5
    lim = health.make_limits(sigma_r_max=2.0, select="not_pd")
    assert (lim.struct_size, lim.select, lim.sigma_r_max, lim.sigma_v_max, lim.qnorm_tol) == (C.sizeof(lim), 2, 2.0, float("inf"), 1e-3)


# ---------------------------------------------------------------- the classification on the host
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/cpp/health_harness.cpp: ekf_health.hpp's health_classify compiled by g++ (the HIP headers define the device decorators
    away), once as it is and once as a stand-alone program under AddressSanitizer and UBSan."""
    return host_harness.build("health_harness", tmp_path_factory)


def run_harness(exe, tmp, dtype, n, compact, x, P, limits, select=63):
    B = x.shape[0]
    hdr = [B, int(dtype == "f64"), int(compact), n, limits["sigma_r_max"], limits["sigma_v_max"], limits["sigma_theta_max"], limits["qnorm_tol"], select]
    o = host_harness.run(exe, tmp, hdr, [np.concatenate([x, host_harness.full_P(P, compact)], axis=1)], (B, 2))
    return o[:, 0].astype(np.uint8), o[:, 1] != 0


CASES = [("f64", 15, False), ("f64", 9, False), ("f64", 9, True), ("f32", 15, False), ("f32", 9, False), ("f32", 9, True)]


@pytest.mark.parametrize("dtype,n,compact", CASES, ids=[f"{d}-n{n}-{'compact' if c else 'full'}" for d, n, c in CASES])
def test_host_compiled_classification_matches_numpy(harness, tmp_path, dtype, n, compact):
    x, P = hu.case_list(dtype, n)
    ref, margin = hu.classify(x, P, **hu.LIMITS)
    assert margin >= 0.5                                       # rounding cannot flip a positive-definite verdict
    want = dict(zip(hu.CASE_NAMES, ref))
    assert want == dict(healthy=0, nan_in_x=hu.NONFINITE, inf_in_P=hu.NONFINITE, indefinite=hu.NOT_PD, q_scaled=hu.QNORM, at_limit=0,
                        above_limit=hu.SIGMA_R, no_state=0), want   # the list holds what it says
    for exe in harness:                                        # the plain build, then the same file under ASan + UBSan
        st, no_state = run_harness(exe, tmp_path, dtype, n, compact, x, P, hu.LIMITS)
        print(f"{dtype} n={n} compact={compact}: status {list(st)} expected {list(ref)}")
        assert np.array_equal(st, ref), (list(st), list(ref))
        assert list(no_state) == [False] * 7 + [True]
    # every bit at once, and limits that are off
    x2, P2 = x.copy(), P.copy()
    P2[3, 1, 1] = 5.0; P2[3, 4, 4] = 30.0; P2[3, 7, 7] = 10.0; x2[3, 6:10] = x[4, 6:10]
    lims = dict(sigma_r_max=2.0, sigma_v_max=5.0, sigma_theta_max=3.0, qnorm_tol=1e-3)
    ref2, margin2 = hu.classify(x2, P2, **lims)
    assert margin2 >= 0.5 and ref2[3] == 62
    st2, _ = run_harness(harness[0], tmp_path, dtype, n, compact, x2, P2, lims)
    assert np.array_equal(st2, ref2), (list(st2), list(ref2))
    off = dict(sigma_r_max=np.inf, sigma_v_max=np.inf, sigma_theta_max=np.inf, qnorm_tol=1e-3)
    st3, _ = run_harness(harness[0], tmp_path, dtype, n, compact, x2, P2, off)
    assert np.array_equal(st3, hu.classify(x2, P2, **off)[0]) and st3[3] == hu.NOT_PD | hu.QNORM and st3[6] == 0
