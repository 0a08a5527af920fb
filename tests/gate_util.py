"""Shared by test_gate_cpu.py and test_gpu_gate.py: the reference of the gate in front of the fused tick -- the dense oracle's
prediction_step followed by the numpy restatement of the innovation (innovation_util.innovation_ref) -- and the displaced tag
poses of the rejection case."""
import numpy as np

import oracle
from innovation_util import CHI2_6_099, innovation_ref_batch
from util import meas_near, qmul

# tolerances against the fp64 reference, relative to the largest element of each output (NIS: to itself): the project's own for the
# innovation diagnostics (test_gpu_innovation.py); the predict step in front adds 5e-7 in fp32 (tests/tolerances.md), well inside
HW = dict(r_v_cv=[0.06036412, -0.00145196, -0.04439579], q_vc=[-0.7035177, 0.7106742, 0.0014521, -0.0017207],
          ab_static=[0.2, -0.09, -0.03], wb_static=[-0.02, -0.01, 0.003])
TOL = {"f64": dict(nu=1e-12, S=1e-12, nis=1e-12), "f32": dict(nu=3e-5, S=3e-5, nis=1e-4)}


def rel(a, b):
    scale = np.abs(b).max(axis=tuple(range(1, b.ndim)), keepdims=True)
    return float((np.abs(a - b) / np.maximum(scale, 1e-300)).max())


def predict_then_innovation(po, p, x, P, u, z, pfp=None, mask=None, predict=True):
    """(nu, S, nis, x_pred, P_pred): oracle.run_batch for one predict-only tick (per-filter Q and static biases when pfp is given),
    then innovation_ref on the predicted state (per-filter R)."""
    if predict:
        x, P = oracle.run_batch(po, x, P, u[None], per_filter_params=pfp)
    R = None if pfp is None else pfp[:, 18:24]
    nu, S, nis = innovation_ref_batch(p, x, P, z, R=R, mask=mask)
    return nu, S, nis, x, P


def rot_z(z, ang, rng):
    """Tag records rotated by `ang` rad about random axes (test_gpu_innovation._rot_z)."""
    z = z.copy()
    ax = rng.normal(size=(z.shape[0], 3)); ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    dq = np.concatenate([ax * np.sin(ang / 2), np.full((z.shape[0], 1), np.cos(ang / 2))], axis=1)
    z[:, 3:7] = qmul(z[:, 3:7], dq)
    return z


def displaced_tag_poses(rng, po, x_pred, frac=0.3):
    """The rejection case of test_gate_rejects_displaced_tag_poses, built around the PREDICTED state: tag poses near it (0.02 m, 0.05 rad),
    a known subset displaced by 1 m and 30 degrees.  -> (z, displaced [B] bool)"""
    B = x_pred.shape[0]
    z = meas_near(rng, po, x_pred, ang=0.05, pos=0.02)
    out = rng.uniform(size=B) < frac
    d = rng.normal(size=(B, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    z[out, 0:3] += d[out]
    z[out] = rot_z(z[out], np.deg2rad(30.0), rng)
    return z, out


def clear_of_threshold(nis, chi2=CHI2_6_099):
    """The "clear of the threshold" rule: a filter whose reference NIS is within 1e-4 (relative) of the threshold may fall either way."""
    return np.abs(nis / chi2 - 1) > 1e-4
