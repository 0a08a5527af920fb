"""Innovation diagnostics (qle_innovation) and the chi-square outlier gate (qle_update_gated, qle_step_gated) on the device.

Reference: innovation_ref (innovation_util.py), the numpy restatement of the first half of correction_step
(relative_pose_EKF.cpp:417-475), evaluated on the values the device holds (the state read back, tag poses and per-filter noise rounded
to the compute dtype).  Every case runs in both dtypes, both orientation methods, full and compact records (est_bias 1 / 0), with and
without per-filter parameters and in the three kernel families of test_gpu_isolation.py (QLE_QUAD unset / 0 / 3: the gated tick's
predict launch follows the policy).

Tolerances against the fp64 restatement, relative to the largest element of each output (NIS: to itself):
  fp64: 1e-12 (measured worst over the grid: nu 2.2e-14, S 1.1e-14, NIS 1.4e-14).
  fp32: 3e-5 (nu, S) and 1e-4 (NIS, which squares the innovation).  Measured worst over the grid on MI355X: nu 1.06e-5, S 1.12e-5,
  NIS 8.4e-6 -- the device also rounds C_vc, r_v_cv and R to fp32, which the fp64 restatement does not, and the innovations reach
  170 degrees.
"""
import numpy as np
import pytest

import oracle
import quadrotor_landing_amd as qla
from quadrotor_landing_amd._lib import QLE_ERR_INVALID, QLE_ERR_STATE
import test_gpu_parity as tp
from oracle import ekf_np
from innovation_util import CHI2_6_099, innovation_ref_batch
from util import assert_state_close, meas_near, qmul, rand_imu, rand_states

pytestmark = pytest.mark.gpu

TOL = {"f64": dict(nu=1e-12, S=1e-12, nis=1e-12), "f32": dict(nu=3e-5, S=3e-5, nis=1e-4)}

B = 64 * 4 + 17
BIG = np.deg2rad(170.0)


@pytest.fixture(autouse=True, params=["default", "lanes-only", "coop-forced"])
def kernel_family(request, monkeypatch):
    """As in test_gpu_isolation: the default policy, the one-lane kernels only (QLE_QUAD=0) and the cooperative kernel forced for every
    single-rate tick (QLE_QUAD=3); QLE_QUAD is read at handle creation."""
    if request.param == "lanes-only":
        monkeypatch.setenv("QLE_QUAD", "0")
    elif request.param == "coop-forced":
        monkeypatch.setenv("QLE_QUAD", "3")
    else:
        monkeypatch.delenv("QLE_QUAD", raising=False)
    return request.param


GRID = [(d, o, e, f) for d in ("f64", "f32") for o in (1, 0) for e in (1, 0) for f in (False, True)]
GRID_IDS = [f"{d}-direct{o}-bias{e}-{'pfp' if f else 'shared'}" for d, o, e, f in GRID]
grid = pytest.mark.parametrize("dtype,direct,est_bias,use_pfp", GRID, ids=GRID_IDS)


def _rot_z(z, ang, rng):
    """Tag records rotated by `ang` rad about random axes (attitude innovation of about that angle)."""
    z = z.copy()
    ax = rng.normal(size=(z.shape[0], 3)); ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    dq = np.concatenate([ax * np.sin(ang / 2), np.full((z.shape[0], 1), np.cos(ang / 2))], axis=1)
    z[:, 3:7] = qmul(z[:, 3:7], dq)
    return z


class Case:
    """A handle with random states, tag poses (innovations up to ~170 degrees) and optionally per-filter parameters."""

    def __init__(self, dtype, direct, est_bias, use_pfp, seed=5, batch=B, cov_scale=0.3):
        self.dtype = dtype
        self.kw = dict(update_freq=400.0, direct_orien_method=direct, est_bias=est_bias, **tp.HW)
        self.po = oracle.make_params(**self.kw)
        self.p = ekf_np.Params.from_orc(self.po)
        self.n = self.po.num_states
        self.B = batch
        rng = np.random.default_rng(seed + 7 * direct + 3 * est_bias + int(use_pfp))
        self.rng = rng
        self.x, self.P = rand_states(rng, batch, self.n, cov_scale=cov_scale)
        if self.n == 9:
            self.x[:, 10:16] = 0.0
        self.z = meas_near(rng, self.po, self.x, ang=BIG, pos=0.1)
        self.u = rand_imu(rng, batch)
        self.ekf = qla.BatchedRelativePoseEKF(batch, dtype, params=qla.make_params(**self.kw))
        self.pfp = None
        if use_pfp:
            pfp = np.zeros((batch, 24))
            pfp[:, 0:12] = np.array(list(self.po.Q)) * 10 ** rng.uniform(-0.5, 0.5, size=(batch, 12))
            pfp[:, 12:15] = self.kw["ab_static"]; pfp[:, 15:18] = self.kw["wb_static"]
            pfp[:, 18:24] = np.array(list(self.po.R)) * rng.uniform(0.3, 3.0, size=(batch, 6))
            if self.n == 9:
                pfp[:, 6:12] = 0.0
            self.ekf.set_filter_params(pfp)
            self.pfp = self.ekf.get_filter_params()   # as the device holds them
        self.reset()

    def reset(self, x=None, P=None):
        self.ekf.set_state(self.x if x is None else x, self.P if P is None else P)

    def dev_z(self, z):
        return z.astype(np.float32).astype(np.float64) if self.dtype == "f32" else z

    def ref(self, z, mask=None):
        """innovation_ref on the values the device holds."""
        xd, Pd = self.ekf.get_state()
        R = None if self.pfp is None else self.pfp[:, 18:24]
        return innovation_ref_batch(self.p, xd, Pd, self.dev_z(z), R=R, mask=mask)

    def close(self):
        self.ekf.close()


def _rel(a, b):
    scale = np.abs(b).max(axis=tuple(range(1, b.ndim)), keepdims=True)
    return float((np.abs(a - b) / np.maximum(scale, 1e-300)).max())


def _same(a, b):
    """bit for bit (float64 arrays compared as their bit patterns, so NaN == NaN and -0 != 0)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float64 and b.dtype == np.float64:
        return np.array_equal(a.view(np.uint64), b.view(np.uint64))
    return np.array_equal(a, b)


@grid
def test_innovation_matches_restatement(dtype, direct, est_bias, use_pfp):
    c = Case(dtype, direct, est_bias, use_pfp)
    nu, S, nis = c.ekf.innovation(c.z)
    nur, Sr, nisr = c.ref(c.z)
    tol = TOL[dtype]
    e_nu, e_S = _rel(nu, nur), _rel(S, Sr)
    e_nis = float(np.abs(nis / nisr - 1).max())
    print(f"{dtype}: worst relative nu {e_nu:.2e} S {e_S:.2e} nis {e_nis:.2e}; NIS range {nisr.min():.3g} .. {nisr.max():.3g}")
    assert np.isfinite(nis).all()
    assert np.array_equal(S, S.transpose(0, 2, 1))
    assert e_nu < tol["nu"] and e_S < tol["S"] and e_nis < tol["nis"], (e_nu, e_S, e_nis)
    c.close()


@grid
def test_innovation_leaves_state_unchanged(dtype, direct, est_bias, use_pfp):
    c = Case(dtype, direct, est_bias, use_pfp)
    x0, P0 = c.ekf.get_state()
    mask = (c.rng.uniform(size=c.B) < 0.7).astype(np.uint8)
    c.ekf.innovation(c.z, mask)
    c.ekf.innovation(c.z)
    x1, P1 = c.ekf.get_state()
    assert _same(x0, x1) and _same(P0, P1)
    c.close()


@grid
def test_update_gated_infinite_threshold_is_update(dtype, direct, est_bias, use_pfp):
    c = Case(dtype, direct, est_bias, use_pfp)
    mask = (c.rng.uniform(size=c.B) < 0.8).astype(np.uint8)
    c.ekf.update(c.z, mask)
    xu, Pu = c.ekf.get_state()
    c.reset()
    acc, nis = c.ekf.update_gated(c.z, np.inf, mask)
    xg, Pg = c.ekf.get_state()
    assert np.array_equal(acc, mask.astype(bool) & np.isfinite(nis))
    assert np.isfinite(nis[mask != 0]).all() and np.isnan(nis[mask == 0]).all()
    assert _same(xu, xg) and _same(Pu, Pg)
    c.close()


@grid
def test_gate_rejects_displaced_tag_poses(dtype, direct, est_bias, use_pfp):
    """A known subset of tag poses displaced by ~1 m and 30 degrees, gated at the 0.99 quantile (16.81)."""
    c = Case(dtype, direct, est_bias, use_pfp, cov_scale=0.05)
    z = meas_near(c.rng, c.po, c.x, ang=0.05, pos=0.02)
    out = c.rng.uniform(size=c.B) < 0.3
    d = c.rng.normal(size=(c.B, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    z[out, 0:3] += d[out]
    z[out] = _rot_z(z[out], np.deg2rad(30.0), c.rng)
    _, _, nisr = c.ref(z)
    x0, P0 = c.ekf.get_state()
    acc, nis = c.ekf.update_gated(z, CHI2_6_099)
    xg, Pg = c.ekf.get_state()
    clear = np.abs(nisr / CHI2_6_099 - 1) > 1e-4
    assert np.array_equal(acc[clear], (nisr <= CHI2_6_099)[clear])
    assert acc[~out].mean() > 0.9 and acc[out].mean() < 0.1
    rej = ~acc
    assert _same(xg[rej], x0[rej]) and _same(Pg[rej], P0[rej])
    c.reset()
    c.ekf.update(z, acc.astype(np.uint8))
    xu, Pu = c.ekf.get_state()
    assert _same(xu, xg) and _same(Pu, Pg)
    c.close()


@grid
def test_step_gated_is_predict_then_update_gated(dtype, direct, est_bias, use_pfp):
    c = Case(dtype, direct, est_bias, use_pfp)
    chi2 = 40.0
    acc, nis = c.ekf.step_gated(c.u, c.z, chi2)
    xs, Ps = c.ekf.get_state()
    c.reset()
    c.ekf.predict(c.u)
    acc2, nis2 = c.ekf.update_gated(c.z, chi2)
    x2, P2 = c.ekf.get_state()
    assert np.array_equal(acc, acc2) and _same(nis, nis2)
    assert _same(xs, x2) and _same(Ps, P2)
    assert acc.any() and (~acc).any()
    # and the fused tick with the accepted filters as its mask, within the fused-versus-split tolerances
    c.reset()
    c.ekf.step(c.u, c.z, acc.astype(np.uint8))
    xf, Pf = c.ekf.get_state()
    assert_state_close(xs, Ps, xf, Pf, **tp.UPD[dtype])
    c.close()


@grid
def test_masked_and_uninitialised_filters(dtype, direct, est_bias, use_pfp):
    c = Case(dtype, direct, est_bias, use_pfp)
    seeded = (c.rng.uniform(size=c.B) < 0.7).astype(np.uint8)
    seeded[:64] = 1
    c.ekf.set_state(np.zeros((c.B, 16)), np.zeros((c.B, c.n, c.n)))
    c.ekf.initialize_state(c.z, mask=seeded)
    assert np.array_equal(c.ekf.state_initialized(), seeded)
    zm = meas_near(c.rng, c.po, c.ekf.get_state()[0], ang=0.1, pos=0.05)
    mask = (c.rng.uniform(size=c.B) < 0.6).astype(np.uint8)
    live = (mask != 0) & (seeded != 0)
    x0, P0 = c.ekf.get_state()
    nu, S, nis = c.ekf.innovation(zm, mask)
    assert np.isnan(nis[~live]).all() and np.isfinite(nis[live]).all()
    assert (nu[~live] == 0).all() and (S[~live] == 0).all()
    acc, nis_g = c.ekf.update_gated(zm, CHI2_6_099 * 1e6, mask)
    assert not acc[~live].any() and acc[live].all()
    assert _same(nis, nis_g)
    x1, P1 = c.ekf.get_state()
    assert _same(x1[~live], x0[~live]) and _same(P1[~live], P0[~live])
    acc, _ = c.ekf.step_gated(c.u, zm, np.inf, mask)
    assert not acc[~live].any()
    x2, P2 = c.ekf.get_state()
    assert _same(x2[seeded == 0], x0[seeded == 0]) and _same(P2[seeded == 0], P0[seeded == 0])
    c.close()


# ---- wave independence (test_gpu_isolation.py style)
BW = 64 * 6 + 23                                                # six waves and a ragged tail
DIST = np.array([0, 63, 64 + 32, 2 * 64 + 15, 64 * 6 + 9])      # lane 0, lane 63, mid-wave, 16th filter of a workgroup, ragged tail
HEALTHY = np.setdiff1d(np.arange(BW), DIST)
DISTURBERS = ["state_nan", "state_inf", "uninit", "corr170", "zero_tag"]


@pytest.mark.parametrize("kind", DISTURBERS)
@grid
def test_filters_independent_of_wave_neighbours(dtype, direct, est_bias, use_pfp, kind):
    c = Case(dtype, direct, est_bias, use_pfp, batch=BW)
    z = meas_near(c.rng, c.po, c.x, ang=0.3, pos=0.05)
    xd, Pd, zd = c.x.copy(), c.P.copy(), z.copy()
    if kind == "state_nan":
        xd[DIST] = np.nan; Pd[DIST] = np.nan
    elif kind == "state_inf":
        xd[DIST, 0:3] = np.inf; Pd[DIST, 0, 0] = np.inf
    elif kind == "uninit":
        xd[DIST] = 0.0
    elif kind == "corr170":
        Pd[DIST] *= 10.0
        zd[DIST] = _rot_z(meas_near(c.rng, c.po, c.x[DIST], ang=0.0, pos=0.05), BIG, c.rng)
    elif kind == "zero_tag":
        zd[DIST] = 0.0

    def run(x, P, zz):
        c.reset(x, P)
        nu, S, nis = c.ekf.innovation(zz)
        acc, nis_g = c.ekf.update_gated(zz, CHI2_6_099)
        xs, Ps = c.ekf.get_state()
        c.reset(x, P)
        acc_s, nis_s = c.ekf.step_gated(c.u, zz, CHI2_6_099)
        xt, Pt = c.ekf.get_state()
        return dict(nu=nu, S=S, nis=nis, acc=acc, nis_g=nis_g, x=xs, P=Ps, acc_s=acc_s, nis_s=nis_s, xt=xt, Pt=Pt)

    base = run(c.x, c.P, z)
    dist = run(xd, Pd, zd)
    for k in base:
        assert _same(base[k][HEALTHY], dist[k][HEALTHY]), (kind, k)
    for a, n in (("acc", "nis_g"), ("acc_s", "nis_s")):
        ok = np.isfinite(dist[n][DIST]) & (dist[n][DIST] <= CHI2_6_099)
        assert not (dist[a][DIST] & ~ok).any(), (kind, a)
    if kind in ("state_nan", "uninit", "zero_tag"):
        assert not dist["acc"][DIST].any() and np.isnan(dist["nis"][DIST]).all()
    c.close()


def test_gated_calls_refuse_multirate_device_gating_and_bad_thresholds():
    kw = dict(update_freq=100.0, direct_orien_method=1)
    rng = np.random.default_rng(3)
    x, P = rand_states(rng, 70, 15, cov_scale=0.3)
    po = oracle.make_params(**kw)
    z = meas_near(rng, po, x)
    u = rand_imu(rng, 70)
    for dtype in ("f64", "f32"):
        ekf = qla.BatchedRelativePoseEKF(70, dtype, params=qla.make_params(**kw))
        ekf.set_state(x, P)
        for bad in (np.nan, 0.0, -1.0, -np.inf):
            for call in (lambda t: ekf.update_gated(z, t), lambda t: ekf.step_gated(u, z, t)):
                with pytest.raises(qla.QleError) as e:
                    call(bad)
                assert e.value.code == QLE_ERR_INVALID
        ekf.enable_gating(True)
        for call in (lambda: ekf.update_gated(z, CHI2_6_099), lambda: ekf.step_gated(u, z, CHI2_6_099)):
            with pytest.raises(qla.QleError) as e:
                call()
            assert e.value.code == QLE_ERR_STATE
        ekf.enable_gating(False)
        ekf.update_gated(z, CHI2_6_099)   # allowed again
        ekf.close()
        mr = qla.BatchedRelativePoseEKF(70, dtype, params=qla.make_params(multirate_ekf=1, measurement_delay=0.03, **kw))
        mr.set_state(x, P)
        for call in (lambda: mr.update_gated(z, CHI2_6_099), lambda: mr.step_gated(u, z, CHI2_6_099)):
            with pytest.raises(qla.QleError) as e:
                call()
            assert e.value.code == QLE_ERR_STATE
        nu, S, nis = mr.innovation(z)     # diagnostics against the current state stay available
        assert np.isfinite(nis).all()
        mr.close()
