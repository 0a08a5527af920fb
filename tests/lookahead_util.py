"""Shared by the look-ahead tests (test_lookahead_cpu.py, test_gpu_lookahead.py): the cases, the reference and the bars.

Reference: the dense fp64 oracle's prediction_step (oracle.run_batch, one predict-only tick at a time) applied h times with the IMU
sample held, from exactly the values the code under test holds.  `ticks_to_limit` is restated in numpy on a covariance trajectory.

Bars.  tests/tolerances.md states what ONE predict of the engine is held to against the oracle (test_predict_teacher_forced):
fp32 state 5e-7, quaternion 1e-6, covariance 3e-6; fp64 1e-12, 1e-11, 5e-11, in the metrics of util.py (state_dev, quat_err, cov_dev).
h predicts in a row are held to h times that: each tick adds its own rounding to what it was handed, and the predict does not amplify
what it was handed by more than 1 + O(dT) per tick (F = I + O(dT)), so the sum over h <= 64 ticks is the bar and no constant is
fitted.  h = 0 is held to equality of bits.  On the GPU the bar is the one the issue sets: twice the larger of the existing path's own
measured deviation (h launches of `predict(u)`) and h times the per-step tolerance -- unless the forecast has that path's bits.

The coast budget compares integers.  A filter whose reference variance comes within 1e-3 (relative) of a limit at any tick 0..h may
fall either way in fp32 and is excluded; at most 5 % of the filters may be.
"""
import numpy as np

import oracle
from util import cov_dev, quat_err, rand_quat, state_dev

STEP_TOL = {"f32": dict(state=5e-7, quat=1e-6, cov=3e-6), "f64": dict(state=1e-12, quat=1e-11, cov=5e-11)}
HW = dict(r_v_cv=[0.06036412, -0.00145196, -0.04439579], q_vc=[-0.7035177, 0.7106742, 0.0014521, -0.0017207],
          ab_static=[0.2, -0.09, -0.03], wb_static=[-0.02, -0.01, 0.003])
KW = dict(update_freq=400.0, measurement_freq=30.0, direct_orien_method=1, Q_a=[0.0005] * 3, Q_w=[0.00005] * 3, **HW)
RECORDS = {"full15": (15, False), "full9": (9, False), "compact9": (9, True)}
HORIZONS = (0, 1, 2, 17, 64)
MARGIN, MAX_EXCLUDED = 1e-3, 0.05


def held(dtype, a):
    """a as a handle of `dtype` holds it"""
    return None if a is None else (a.astype(np.float32).astype(np.float64) if dtype == "f32" else np.array(a, dtype=np.float64))


def make_pfp(rng, po, B, n):
    """Per-filter [Q 12, ab_static 3, wb_static 3, R 6]: noise within half a decade of the shared values, static biases jittered."""
    pfp = np.zeros((B, 24))
    pfp[:, 0:12] = np.array(list(po.Q)) * 10 ** rng.uniform(-0.5, 0.5, size=(B, 12))
    pfp[:, 12:15] = np.array(HW["ab_static"]) + 0.01 * rng.normal(size=(B, 3))
    pfp[:, 15:18] = np.array(HW["wb_static"]) + 0.001 * rng.normal(size=(B, 3))
    pfp[:, 18:24] = np.array(list(po.R)) * rng.uniform(0.3, 3.0, size=(B, 6))
    if n == 9:
        pfp[:, 6:12] = 0.0
    return pfp


def make_case(dtype, n, use_pfp, B, seed):
    """(po, x, P, u, pfp) as a handle of `dtype` holds them.  Gyro: filter 0 turns at exactly zero rate (the sample equals its biases
    in the held values), filter 1 below small_ang_tol (dT * |w| = 5e-11 < 1e-10), filter 2 at a few rad/s, the rest ~0.4 rad/s."""
    po = oracle.make_params(**dict(KW, est_bias=int(n == 15)))
    rng = np.random.default_rng(seed)
    x = np.zeros((B, 16))
    x[:, 0:3] = rng.uniform([-1, -1, 1], [1, 1, 4], size=(B, 3))
    x[:, 3:6] = rng.normal(size=(B, 3)) * 0.5
    x[:, 6:10] = rand_quat(rng, B)
    if n == 15:
        x[:, 10:13] = rng.normal(size=(B, 3)) * 0.1
        x[:, 13:16] = rng.normal(size=(B, 3)) * 0.01
    A = rng.normal(size=(B, n, n)) * 0.1
    P = A @ A.transpose(0, 2, 1) + np.eye(n) * rng.uniform(0.01, 0.2, size=(B, n, 1))
    P = 0.5 * (P + P.transpose(0, 2, 1))
    u = np.zeros((B, 6))
    u[:, 0:3] = rng.normal(size=(B, 3)) * 1.5 + np.array([0, 0, 9.8])
    u[:, 3:6] = rng.normal(size=(B, 3)) * 0.4
    pfp = make_pfp(rng, po, B, n) if use_pfp else None
    x, P, u, pfp = held(dtype, x), held(dtype, P), held(dtype, u), held(dtype, pfp)
    P = 0.5 * (P + P.transpose(0, 2, 1))
    # the special rates, on the held values: filters 0 and 1 carry no gyro bias of their own, so u - x[13:16] - wb_static is exact
    wb = np.tile(held(dtype, np.array(HW["wb_static"])), (B, 1)) if pfp is None else pfp[:, 15:18]
    if B >= 3:
        x[0:2, 13:16] = 0.0
        u[0, 3:6] = wb[0]
        u[1, 3:6] = wb[1] + np.array([0.0, 0.0, 2e-8])
        u[2, 3:6] = [3.0, -2.0, 2.5]
        u = held(dtype, u)
    return po, x, P, u, pfp


def oracle_trajectory(po, x, P, u, h, pfp=None):
    """([h+1, B, 16], [h+1, B, n, n]): the state after k = 0..h oracle predicts with u held."""
    xs, Ps = [np.array(x, dtype=np.float64)], [np.array(P, dtype=np.float64)]
    for _ in range(h):
        xk, Pk = oracle.run_batch(po, xs[-1], Ps[-1], u[None], per_filter_params=pfp)
        xs.append(xk); Ps.append(Pk)
    return np.stack(xs), np.stack(Ps)


def deviations(x, P, xr, Pr):
    """(state, quat, cov) deviation in the metrics of util.py"""
    return dict(state=float(state_dev(x, xr)), quat=float(quat_err(x[:, 6:10], xr[:, 6:10])), cov=float(cov_dev(P, Pr)))


def block_max(Ps):
    """([..., B], [..., B]): the largest diagonal entry of P(r,r) and of P(theta,theta)"""
    d = np.einsum("...ii->...i", Ps)
    return d[..., 0:3].max(axis=-1), d[..., 6:9].max(axis=-1)


def ticks_rule(Ps, sigma_r_max, sigma_theta_max, skipped=None):
    """ticks_to_limit of include/qle_lookahead.h restated on a covariance trajectory Ps [h+1, B, n, n] (doubles): the smallest k at
    which a diagonal entry of P(r,r) exceeds sigma_r_max^2 or one of P(theta,theta) exceeds sigma_theta_max^2, else -1."""
    mr, mt = block_max(Ps)
    over = (mr > float(sigma_r_max) * float(sigma_r_max)) | (mt > float(sigma_theta_max) * float(sigma_theta_max))
    t = np.where(over.any(axis=0), over.argmax(axis=0), -1).astype(np.int32)
    if skipped is not None:
        t[skipped] = -1
    return t


def limit_margin(Ps, sigma_r_max, sigma_theta_max):
    """[B]: the smallest relative distance of a block's largest variance from its limit squared over the ticks of the trajectory"""
    mr, mt = block_max(Ps)
    m = np.full(Ps.shape[1], np.inf)
    for v, s in ((mr, sigma_r_max), (mt, sigma_theta_max)):
        if np.isfinite(s):
            m = np.minimum(m, np.abs(v / (float(s) * float(s)) - 1.0).min(axis=0))
    return m


def coast_case(dtype, n, use_pfp, B, h, seed):
    """A case whose crossings spread over k = 0, inside the horizon and never, and the two limits of the call.
    The priors are scaled per filter: position variances of ~1e-7 (every fourth filter: ~1e-3, above the limit at k = 0) under
    velocity variances of 0.2 x 10^U(-1.3, 1) (every fourth filter: 1e-4 of that, never), so that P(r,r) grows by dT^2 k^2 P(v,v) --
    several per cent per tick near the crossing; attitude variances of U(0, 30) Q_w under a growth of Q_w per tick.
    The limits are fixed per call and come from the oracle's trajectory of one reference filter (filter 1 for r, the filter at the
    80th percentile of the attitude priors for theta), midway between its values at two consecutive ticks in the middle of the horizon.
    -> (po, x, P, u, pfp, sigma_r_max, sigma_theta_max, Ps_oracle)"""
    po, x, P, u, pfp = make_case(dtype, n, use_pfp, B, seed)
    rng = np.random.default_rng(seed + 1)
    cls = np.arange(B) % 4
    s = np.ones((B, n))
    s[:, 0:3] = np.where(cls == 0, 1e-1, 1e-3)[:, None]
    vs = 10 ** rng.uniform(-1.3, 1.0, size=B)
    vs[1] = 1.0
    s[:, 3:6] = np.sqrt(np.where(cls == 3, 1e-4, 1.0) * vs)[:, None]
    qw = float(po.Q[3])
    th = rng.uniform(0.0, 30.0, size=B) * qw
    th[cls == 3] = rng.uniform(0.0, 5.0, size=int((cls == 3).sum())) * qw
    s[:, 6:9] = np.sqrt(th / np.einsum("bii->bi", P)[:, 6:9].max(axis=1))[:, None]
    if n == 15:
        s[:, 9:12] = 1e-2
        s[:, 12:15] = 1e-4
    P = held(dtype, P * s[:, :, None] * s[:, None, :])
    P = 0.5 * (P + P.transpose(0, 2, 1))
    _, Ps = oracle_trajectory(po, x, P, u, h, pfp)
    mr, mt = block_max(Ps)
    k = max(1, h // 2)
    sigma_r = float(np.sqrt(0.5 * (mr[k - 1, 1] + mr[k, 1])))
    j = int(np.argsort(mt[0])[(4 * B) // 5])
    sigma_t = float(np.sqrt(0.5 * (mt[k - 1, j] + mt[k, j])))
    return po, x, P, u, pfp, sigma_r, sigma_t, Ps
