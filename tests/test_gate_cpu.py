"""CPU tests of the chi-square gate in front of the fused tick (include/qle_gate.h, libqle_gate.so, quadrotor_landing_amd/gate.py,
csrc/ekf_pregate.hpp): the library builds, exports and binds what its header declares, its kernels are its own (none shared with, none
added to, libqle_ekf.so and libqle_devio.so), its generated code passes the stale-EXEC audit, the arithmetic of k_pregate -- compiled
for the host with g++ -- agrees with the dense oracle's predict followed by the numpy restatement of the innovation, and every refusal
is made before any GPU call (without a GPU a HIP call would fail with another error class).

What the host build covers: the arithmetic of pregate_eval and the set of covariance words it reads (tests/cpp/pregate_harness.cpp fills
every word outside pregate_needs with NaN).  What it does not cover: the kernel's own loads -- which 16-byte quads it fetches
(load_P_rows of ekf_layout.hpp over pregate_needs or the pose block) and the record loads (load_rec).  Those run only on the GPU and are
held by tests/test_gpu_gate.py; here only their word counts are checked, by the static_asserts of ekf_pregate.hpp at compile time.

Measured deviations of the host-compiled arithmetic from the reference (worst over the grid, B = 300, innovations up to 170 degrees;
bars in gate_util.TOL):
  fp64: nu 2.2e-14, S 2.4e-15, NIS 3.5e-14 (bar 1e-12)
  fp32: nu 1.5e-5, S 1.6e-6, NIS 2.0e-5 (bars 3e-5, 3e-5, 1e-4)
The fp32 nu figure is within a factor of 3 of its bar, with and without the predict step in front (1.48e-5 / 1.48e-5): it is the
attitude innovation near 170 degrees, where the logarithm divides by a quaternion scalar part of ~0.09 held to fp32 (the same figure
test_gpu_innovation.py records for k_innov, 1.06e-5, on its own seeds); the predict step adds nothing visible.
"""
import ctypes as C
import os

import numpy as np
import pytest

import host_harness
import oracle
import side_lib_util
from elf_util import _kernels
from gate_util import HW, TOL, clear_of_threshold, displaced_tag_poses, predict_then_innovation, rel
from innovation_util import CHI2_6_099
from oracle import ekf_np
from quadrotor_landing_amd import _lib, devio, gate
from side_lib_util import FakeTensor, _params, _views, assert_audit_counts, assert_exports_and_binds, ensure_built, run_audit
from util import forbid_native, meas_near, rand_imu, rand_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qle_gate.h")


@pytest.fixture(scope="module")
def gate_so():
    return ensure_built("gate")


def test_library_exports_and_binds_every_declared_function(gate_so):
    names, _ = assert_exports_and_binds(gate, HEADER, "qgt", gate_so)
    assert len(names) >= 3


def test_kernels_are_disjoint_from_the_tick_and_boundary_libraries(gate_so):
    mine, main, dv = _kernels(gate_so), _kernels(_lib.LIB_PATH), _kernels(devio.DEVIO_LIB_PATH)
    assert mine and main and dv
    assert not mine & main, sorted(mine & main)
    assert not mine & dv, sorted(mine & dv)
    ids = {_lib.demangle(m) for m in mine}
    assert all(i.startswith("void qle::k_pregate<") for i in ids), sorted(ids)
    assert len(ids) == 32   # T x DIRECT x PFP x COMPACT x PREDICT
    assert not any("k_pregate" in _lib.demangle(m) for m in main | dv)


def test_generated_device_code_passes_the_stale_exec_audit(gate_so):
    assert_audit_counts(run_audit("gate")[0], "gate")


# ---------------------------------------------------------------- the arithmetic on the host
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/cpp/pregate_harness.cpp: ekf_pregate.hpp's pregate_eval compiled by g++ (the HIP headers define the device decorators away),
    once as it is and once as a stand-alone program under AddressSanitizer and UBSan."""
    return host_harness.build("pregate_harness", tmp_path_factory)


def run_harness(exe, tmp, po, dtype, predict, x, P, u, z, pfp):
    B = x.shape[0]
    hdr = [B, po.direct_orien_method, int(predict), int(pfp is not None), int(dtype == "f64"), *host_harness.params_header(po)]
    per = np.concatenate([x, host_harness.full_P(P), u, z, np.zeros((B, 24)) if pfp is None else pfp], axis=1)
    o = host_harness.run(exe, tmp, hdr, [per], (B, 43))
    return o[:, 1:7], o[:, 7:].reshape(B, 6, 6), o[:, 0]


GRID = [(d, o, e, f) for d in ("f64", "f32") for o in (1, 0) for e in (1, 0) for f in (False, True)]
GRID_IDS = [f"{d}-direct{o}-bias{e}-{'pfp' if f else 'shared'}" for d, o, e, f in GRID]


def make_case(dtype, direct, est_bias, use_pfp, B=300, seed=5):
    kw = dict(update_freq=400.0, direct_orien_method=direct, est_bias=est_bias, **HW)
    po = oracle.make_params(**kw)
    n = po.num_states
    rng = np.random.default_rng(seed + 7 * direct + 3 * est_bias + int(use_pfp))
    x, P = rand_states(rng, B, n, cov_scale=0.3)
    if n == 9:
        x[:, 10:16] = 0.0
    z = meas_near(rng, po, x, ang=np.deg2rad(170.0), pos=0.1)
    u = rand_imu(rng, B)
    pfp = None
    if use_pfp:
        pfp = np.zeros((B, 24))
        pfp[:, 0:12] = np.array(list(po.Q)) * 10 ** rng.uniform(-0.5, 0.5, size=(B, 12))
        pfp[:, 12:15] = HW["ab_static"]; pfp[:, 15:18] = HW["wb_static"]
        pfp[:, 18:24] = np.array(list(po.R)) * rng.uniform(0.3, 3.0, size=(B, 6))
        if n == 9:
            pfp[:, 6:12] = 0.0
    if dtype == "f32":   # the values an fp32 handle holds
        r32 = lambda a: None if a is None else a.astype(np.float32).astype(np.float64)
        x, P, z, u, pfp = r32(x), r32(P), r32(z), r32(u), r32(pfp)
    return po, ekf_np.Params.from_orc(po), rng, x, P, u, z, pfp


@pytest.mark.parametrize("predict", [True, False], ids=["predict", "stored"])
@pytest.mark.parametrize("dtype,direct,est_bias,use_pfp", GRID, ids=GRID_IDS)
def test_host_compiled_arithmetic_matches_oracle_predict_then_restatement(harness, tmp_path, dtype, direct, est_bias, use_pfp, predict):
    po, p, rng, x, P, u, z, pfp = make_case(dtype, direct, est_bias, use_pfp)
    nur, Sr, nisr, _, _ = predict_then_innovation(po, p, x, P, u, z, pfp, predict=predict)
    tol = TOL[dtype]
    for exe in harness:                                        # the plain build, then the same file under ASan + UBSan
        nu, S, nis = run_harness(exe, tmp_path, po, dtype, predict, x, P, u, z, pfp)
        e_nu, e_S, e_nis = rel(nu, nur), rel(S, Sr), float(np.abs(nis / nisr - 1).max())
        print(f"{dtype} predict={predict}: worst relative nu {e_nu:.2e} S {e_S:.2e} nis {e_nis:.2e}; NIS range {nisr.min():.3g} .. {nisr.max():.3g}")
        assert np.isfinite(nis).all() and np.array_equal(S, S.transpose(0, 2, 1))
        assert e_nu < tol["nu"] and e_S < tol["S"] and e_nis < tol["nis"], (e_nu, e_S, e_nis)


def test_not_positive_definite_S_gives_nan(harness, tmp_path):
    po, p, rng, x, P, u, z, pfp = make_case("f64", 1, 1, False, B=8)
    P[3] = -P[3]
    for exe in harness:
        _, _, nis = run_harness(exe, tmp_path, po, "f64", False, x, P, u, z, None)
        assert np.isnan(nis[3]) and np.isfinite(np.delete(nis, 3)).all()


@pytest.mark.parametrize("dtype,direct,est_bias,use_pfp", GRID, ids=GRID_IDS)
def test_displaced_tag_poses_stay_clear_of_the_threshold(harness, tmp_path, dtype, direct, est_bias, use_pfp):
    """The rejection case of test_gpu_gate.py (same seeds, same batch): by the oracle alone at most 1 % of the filters come within 1e-4 of
    the threshold, the displaced poses are rejected and the others accepted; the host-compiled arithmetic decides every clear filter as
    the oracle does."""
    B = 2391
    kw = dict(update_freq=400.0, direct_orien_method=direct, est_bias=est_bias, **HW)
    po = oracle.make_params(**kw)
    p = ekf_np.Params.from_orc(po)
    rng = np.random.default_rng(41 + 7 * direct + 3 * est_bias + int(use_pfp))
    x, P = rand_states(rng, B, po.num_states, cov_scale=0.05)
    if po.num_states == 9:
        x[:, 10:16] = 0.0
    u = rand_imu(rng, B)
    xp, _ = oracle.run_batch(po, x, P, u[None])
    z, out = displaced_tag_poses(rng, po, xp)
    if dtype == "f32":
        x, P, u, z = (a.astype(np.float32).astype(np.float64) for a in (x, P, u, z))
    _, _, nisr, _, _ = predict_then_innovation(po, p, x, P, u, z)
    clear = clear_of_threshold(nisr)
    assert (~clear).mean() <= 0.01
    acc_ref = nisr <= CHI2_6_099
    assert acc_ref[~out].mean() > 0.9 and acc_ref[out].mean() < 0.1
    for exe in harness:
        _, _, nis = run_harness(exe, tmp_path, po, dtype, True, x, P, u, z, None)
        assert np.array_equal((nis <= CHI2_6_099)[clear], acc_ref[clear])


# ---------------------------------------------------------------- refusals, before any GPU call
def test_library_refuses_before_any_gpu_call(gate_so):
    """No GPU here: a call that got as far as the HIP runtime would return QLE_ERR_HIP (or crash on the fake pointers), not these."""
    G = gate.gate_lib()
    v, iv = _views()
    p = _params()
    out = 0x7F3000000000
    tick = lambda v_, iv_, p_, chi2: G.qgt_gate_tick(v_, iv_, p_, chi2, out, out, None, None, gate.QGT_F32)
    inno = lambda v_, iv_, p_: G.qgt_innovation(v_, iv_, p_, out, None, None, gate.QGT_F32)
    B = C.byref
    assert tick(None, B(iv), B(p), 16.81) == _lib.QLE_ERR_INVALID and b"view" in G.qgt_last_error()
    assert tick(B(v), None, B(p), 16.81) == _lib.QLE_ERR_INVALID
    assert tick(B(v), B(iv), None, 16.81) == _lib.QLE_ERR_INVALID
    short, _ = _views(); short.struct_size = C.sizeof(short) - 8
    assert tick(B(short), B(iv), B(p), 16.81) == _lib.QLE_ERR_INVALID and inno(B(short), B(iv), B(p)) == _lib.QLE_ERR_INVALID
    _, ishort = _views(); ishort.struct_size = 8
    assert tick(B(v), B(ishort), B(p), 16.81) == _lib.QLE_ERR_INVALID
    mr = _params(multirate_ekf=1)
    assert tick(B(v), B(iv), B(mr), 16.81) == _lib.QLE_ERR_STATE and b"multirate" in G.qgt_last_error()
    assert inno(B(v), B(iv), B(mr)) == _lib.QLE_ERR_STATE
    _, notag = _views(tag=False)
    assert tick(B(v), B(notag), B(p), 16.81) == _lib.QLE_ERR_INVALID and b"tag slot" in G.qgt_last_error()
    assert inno(B(v), B(notag), B(p)) == _lib.QLE_ERR_INVALID
    for bad in (0.0, -1.0, float("nan"), float("-inf")):
        assert tick(B(v), B(iv), B(p), bad) == _lib.QLE_ERR_INVALID and b"chi2_max" in G.qgt_last_error()
    assert G.qgt_gate_tick(B(v), B(iv), B(p), 16.81, out, out, None, None, 7) == _lib.QLE_ERR_INVALID
    nine = _params(est_bias=0)
    assert tick(B(v), B(iv), B(nine), 16.81) == _lib.QLE_ERR_INVALID   # the view says 15 states
    assert G.qgt_launch_count() == 0


class FakeEkf(side_lib_util.FakeEkf):
    def __init__(self, **kw):
        self.params = _params(**kw)


def test_deviceio_refuses_bad_gate_arguments_before_any_gpu_call(monkeypatch):
    ekf, ekf_mr = FakeEkf(), FakeEkf(multirate_ekf=1)   # their parameters come from the tick library: made first
    forbid_native(monkeypatch)
    B = 100
    io = devio.DeviceIO(ekf)
    u, z = FakeTensor((B, 6)), FakeTensor((B, 7))
    bad = [
        dict(u=u, chi2_max=16.81),                                   # a tick without tag poses
        dict(u=u, z=z, chi2_max=0.0),
        dict(u=u, z=z, chi2_max=-3.0),
        dict(u=u, z=z, chi2_max=float("nan")),
        dict(u=u, z=z, return_nis=True),                             # nothing to return without a gate
        dict(u=u, z=FakeTensor((B, 6)), chi2_max=16.81),
        dict(u=u, z=z, mask=FakeTensor((B,), dtype="float32"), chi2_max=16.81),
        dict(u=FakeTensor((B, 6), device="cpu"), z=z, chi2_max=16.81),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            io.tick(**kw)
    for kw in (dict(z=FakeTensor((B, 6))), dict(z=z, mask=FakeTensor((B, 1), dtype="uint8")), dict(z=z, dtype="int32"),
               dict(z=FakeTensor((B, 7), ptr=0x7F0000000008)), dict(z=np.zeros((B, 7)))):
        with pytest.raises(ValueError):
            io.innovation(**kw)
    mr = devio.DeviceIO(ekf_mr)
    for call in (lambda: mr.tick(u, z, chi2_max=16.81), lambda: mr.innovation(z)):
        with pytest.raises(_lib.QleError) as e:
            call()
        assert e.value.code == _lib.QLE_ERR_STATE
    with pytest.raises(AssertionError, match="native library"):
        io.tick(u, z, chi2_max=16.81)   # a good call is what reaches the libraries
