"""Shared helpers for the parity tests (oracle <-> engine)."""
import json
import math
import os
import re

import numpy as np

import oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def forbid_native(monkeypatch):
    """Make every native library unreachable, for the "refuses before any GPU call" tests: the side-library loader, `_lib.lib`, and
    every name a module of the package binds either under (`<x>_lib`, `lib`).  Whatever reaches one raises AssertionError; returns the function that
    raises it, for what else counts as native in a test (a fake handle's `make_inputs`)."""
    import sys

    from quadrotor_landing_amd import _lib

    def boom(*a, **k):
        raise AssertionError("a native library was reached")
    loader, tick = _lib.SideLibrary.load, _lib.lib
    for name, mod in list(sys.modules.items()):
        if mod is None or not name.startswith("quadrotor_landing_amd"):
            continue
        for attr, v in list(vars(mod).items()):
            if v is tick or (getattr(v, "__func__", None) is loader and isinstance(getattr(v, "__self__", None), _lib.SideLibrary)):
                monkeypatch.setattr(mod, attr, boom)
    monkeypatch.setattr(_lib.SideLibrary, "load", boom)
    return boom


def param_sets():
    return json.load(open(os.path.join(GOLDEN, "param_sets.json")))


def golden_kwargs(ps, **over):
    """Keyword set valid for both oracle.make_params and quadrotor_landing_amd.make_params."""
    s = param_sets()[ps]
    q = s["Q"]
    kw = dict(update_freq=s["update_freq"], est_bias=int(s["est_bias"]), direct_orien_method=1,
              Q_a=q[0:3], Q_w=q[3:6], R_r=s["R"][0:3], R_ang=s["R"][3:6], r_v_cv=s["r_v_cv"], q_vc=s["q_vc"])
    if s["est_bias"]:
        kw.update(Q_ab=q[6:9], Q_wb=q[9:12])
    kw.update(over)
    return kw


def rand_quat(rng, n, max_angle=None):
    if max_angle is None:
        q = rng.normal(size=(n, 4))
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        q[q[:, 3] < 0] *= -1
        return q
    ax = rng.normal(size=(n, 3)); ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    ang = rng.uniform(0, max_angle, size=(n, 1))
    return np.concatenate([ax * np.sin(ang / 2), np.cos(ang / 2)], axis=1)


def rand_states(rng, B, n, cov_scale=1.0):
    x = np.zeros((B, 16))
    x[:, 0:3] = rng.uniform([-1, -1, 1], [1, 1, 4], size=(B, 3))
    x[:, 3:6] = rng.normal(size=(B, 3)) * 0.5
    x[:, 6:10] = rand_quat(rng, B)
    if n == 15:
        x[:, 10:13] = rng.normal(size=(B, 3)) * 0.1
        x[:, 13:16] = rng.normal(size=(B, 3)) * 0.01
    A = rng.normal(size=(B, n, n)) * 0.1
    P = A @ A.transpose(0, 2, 1) + np.eye(n) * rng.uniform(0.01, 0.2, size=(B, n, 1))
    P = 0.5 * (P + P.transpose(0, 2, 1)) * cov_scale
    return x, P


def rand_imu(rng, B):
    u = np.zeros((B, 6))
    u[:, 0:3] = rng.normal(size=(B, 3)) * 1.5 + np.array([0, 0, 9.8])
    u[:, 3:6] = rng.normal(size=(B, 3)) * 0.4
    return u


def qmul(a, b):
    av, aw, bv, bw = a[..., :3], a[..., 3:4], b[..., :3], b[..., 3:4]
    return np.concatenate([aw * bv + bw * av + np.cross(av, bv), aw * bw - np.sum(av * bv, axis=-1, keepdims=True)], axis=-1)


def qconj(q):
    return q * np.array([-1, -1, -1, 1.0])


def rot(q):
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([
        np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
        np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
        np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def meas_near(rng, orc_p, x, ang=0.8, pos=0.1):
    """Tag poses whose implied pose is near state x (inverse of EKF.cpp:431-438)."""
    B = x.shape[0]
    q_vc = np.array(list(orc_p.q_vc)); C_vc = np.array(list(orc_p.C_vc)).reshape(3, 3); r_v_cv = np.array(list(orc_p.r_v_cv))
    q_true = qmul(x[:, 6:10], rand_quat(rng, B, ang))
    r_true = x[:, 0:3] + rng.normal(size=(B, 3)) * pos
    q_ct = qmul(qconj(q_vc)[None], qconj(q_true))
    t = -np.einsum("bji,bj->bi", rot(q_true), r_true) - r_v_cv
    r_c = t @ C_vc  # C_vc^T t
    return np.concatenate([r_c, q_ct], axis=1)


def oracle_predict_batch(p, x, P, u):
    xo = np.empty_like(x); Po = np.empty_like(P); acc = np.empty((x.shape[0], 3))
    for i in range(x.shape[0]):
        xo[i], Po[i], acc[i] = oracle.prediction_step(p, x[i], P[i], u[i])
    return xo, Po, acc


def oracle_update_batch(p, x, P, z, mask=None):
    xo = x.copy(); Po = P.copy()
    obs = np.zeros((x.shape[0], 7))
    for i in range(x.shape[0]):
        if mask is None or mask[i]:
            xo[i], Po[i], obs[i, :3], obs[i, 3:] = oracle.correction_step(p, x[i], P[i], z[i, :3], z[i, 3:])
    return xo, Po, obs


def quat_err(a, b):
    """max over batch of min(|a-b|, |a+b|) per quaternion (sign-insensitive)."""
    return np.minimum(np.abs(a - b).max(axis=-1), np.abs(a + b).max(axis=-1)).max()


# Every engine-vs-reference comparison goes through note(): with QLE_TOL_RECORD=<path> the measured deviation is written next
# to the tolerance it was held against, per test, so that the stated tolerances can be audited (and re-derived) from a GPU run:
# tests/tolerances.md is that table.  A tolerance more than ~10x its measured deviation hides regressions.
_REC = []
_TIGHT = {}
_tight_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tolerances_tight.json")
if os.path.exists(_tight_path) and not os.environ.get("QLE_TOL_STATED"):   # QLE_TOL_STATED=1: the stated tolerances only (to re-derive the table)
    _TIGHT = json.load(open(_tight_path))


def _test_key():
    t = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]
    t = t.split("::", 1)[1] if "::" in t else t
    return re.sub(r"\[(default|lanes-only|coop-forced)-?", "[", t).replace("[]", "")


def note(kind, value, tol):
    """Every engine-vs-reference comparison passes through here.  The deviation is held against the smaller of the tolerance the test
    states and the entry of tests/tolerances_tight.json (50 x the deviation an MI355X run measured, for comparisons whose stated
    tolerance was more than 100 x that measurement: tests/make_tolerances.py), and recorded when QLE_TOL_RECORD is set."""
    value = float(value)
    eff = min(float(tol), _TIGHT.get(f"{_test_key()}|{kind}|{float(tol):.3e}", float(tol)))
    if os.environ.get("QLE_TOL_RECORD"):
        _REC.append((os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0], kind, value, eff, float(tol)))
    assert value <= eff or not (value == value), f"{kind}: deviation {value:.3e} above the tolerance in force {eff:.3e} (stated {float(tol):.3e})"
    return value


def _dump_rec():
    path = os.environ.get("QLE_TOL_RECORD")
    if path and _REC:
        agg = {}
        for test, kind, v, tol, stated in _REC:
            k = (test, kind, tol, stated)
            agg[k] = max(agg.get(k, 0.0), v)
        with open(path, "a") as fh:
            for (test, kind, tol, stated), v in sorted(agg.items()):
                fh.write(json.dumps(dict(test=test, kind=kind, measured=v, tol=tol, stated=stated)) + "\n")


import atexit  # noqa: E402
atexit.register(_dump_rec)


def state_dev(x, xr):
    """max |x - xr| / (1 + |xr|) over the non-quaternion state words: the single number `tol` of assert_state_close bounds
    (|x - xr| <= tol (1 + |xr|) is numpy's allclose with atol = rtol = tol)."""
    keep = [i for i in range(16) if not 6 <= i < 10]
    return (np.abs(x[..., keep] - xr[..., keep]) / (1.0 + np.abs(xr[..., keep]))).max()


def cov_dev(P, Pr):
    """max |P_ij - Pr_ij| / sqrt(Pr_ii Pr_jj): entries near zero are sums of O(diag) terms, so the scale is the matrix's own."""
    scale = np.sqrt(np.einsum("...ii->...i", Pr)[..., :, None] * np.einsum("...ii->...i", Pr)[..., None, :])
    return (np.abs(P - Pr) / (scale + 1e-300)).max()


def assert_state_close(x, P, xr, Pr, rtol, atol=None, qtol=None, ptol=None):
    """State words within rtol/atol, quaternion (up to sign) within qtol, covariance entries within ptol x sqrt(P_ii P_jj).
    ptol is its own argument: fp64 callers that leave it out get 50 rtol (5e-11 for the per-step 1e-12), fp32 callers state it."""
    atol = rtol if atol is None else atol
    qtol = qtol if qtol is not None else max(atol, rtol) * 10
    ptol = ptol if ptol is not None else rtol * 50
    dq = note("quat", quat_err(x[:, 6:10], xr[:, 6:10]), qtol)
    assert dq <= qtol, (dq, qtol)
    keep = [i for i in range(16) if not 6 <= i < 10]
    note("state", state_dev(x, xr), max(rtol, atol))
    np.testing.assert_allclose(x[:, keep], xr[:, keep], rtol=rtol, atol=atol)
    err = note("cov", cov_dev(P, Pr), ptol)
    assert err <= ptol, (err, ptol)


def orc_params_from_qle(qp):
    """oracle parameter block from an engine parameter block (field-for-field; used with load_yaml)."""
    kw = {}
    orc_fields = {n for n, _ in oracle.OrcParams._fields_}
    derived = {"dT_nom", "upd_per_meas", "num_states", "measurement_step_delay", "Q", "R", "cov_init", "C_vc"}
    for name, _ in type(qp)._fields_:
        if name in orc_fields and name not in derived:
            v = getattr(qp, name)
            kw[name] = list(v) if hasattr(v, "__len__") else v
    return oracle.make_params(**kw)


def oracle_replay(p, events):
    """The reference node's loop on a recorded event log with the oracle's one-filter object
    (same schedule as quadrotor_landing_amd.replay.replay / ekf_driver --sequence).
    -> rows [t, x16, accel3, performed, upds, delay, P00, Ptt00] per active tick."""
    from quadrotor_landing_amd.replay import tick_times
    f = oracle.Filter(p)
    rows, k = [], 0
    for t in tick_times(events, 1.0 / p.update_freq):
        while k < len(events) and events[k][1] <= t:
            e = events[k]; k += 1
            if e[0] == "imu":
                f.set_imu(e[2][:3], e[2][3:])
            else:
                f.set_apriltag(e[3][:3], e[3][3:], e[2])
        if not f.f.state_initialized:
            continue
        f.filter_update(t)
        P = f.P()
        rows.append(np.concatenate([[t], f.x(), list(f.f.accel_rel), [f.f.performed_correction, f.f.upds_since_correction,
                                                                      f.f.measurement_delay_curr, P[0, 0], P[6, 6]]]))
    return np.array(rows)
