"""Innovation diagnostics and the chi-square gate, host side.

innovation_ref is the numpy restatement the GPU tests (test_gpu_innovation.py) check the engine against: the first half of
oracle/ekf_np.correction_step (relative_pose_EKF.cpp:417-475) -- the innovation delta_y, G, N, R_k = N R N^T, S = G P G^T + R_k --
and NIS = delta_y^T S^-1 delta_y.  The tests here hold it to correction_step itself and check the ctypes binding of the new entry points.
"""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
from oracle import ekf_np
from oracle.ekf_np import observe, qconj, qmul, quaternion_exp, quaternion_log, quaternion_norm, rot, skew
from quadrotor_landing_amd import _lib
from util import meas_near, rand_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHI2_6_099 = 16.81    # 0.99 quantile of chi-square with 6 degrees of freedom
CHI2_6_0999 = 22.46   # 0.999 quantile


def innovation_ref(p, x, P, z):
    """(delta_y [6], G [6,n], S [6,6], nis) of one filter; p is an ekf_np.Params."""
    x = np.asarray(x, dtype=np.float64)
    n = p.num_states
    P = np.asarray(P, dtype=np.float64).reshape(n, n)
    r, q = x[0:3], x[6:10]
    Cc = rot(q)
    r_obs, q_obs = observe(p, None if p.direct_orien_method else q, np.asarray(z[:3], float), np.asarray(z[3:7], float))
    dy = np.zeros(6)
    dy[0:3] = r_obs - r
    dy[3:6] = quaternion_log(quaternion_norm(qmul(qconj(q), q_obs)))
    G = np.zeros((6, n))
    G[0:3, 0:3] = np.eye(3)
    G[3:6, 6:9] = np.eye(3)
    N = np.zeros((6, 6))
    N[0:3, 0:3] = -Cc @ p.C_vc
    N[3:6, 3:6] = p.C_vc
    if p.direct_orien_method:
        N[0:3, 3:6] = skew(r)
    else:
        G[0:3, 6:9] = Cc @ skew(Cc.T @ r)
    Rk = N @ np.diag(p.R) @ N.T
    S = G @ P @ G.T + Rk
    nis = float(dy @ np.linalg.solve(S, dy))
    return dy, G, S, nis


def innovation_ref_batch(p, x, P, z, R=None, mask=None):
    """Batched innovation_ref; R [B,6] per-filter noise overrides; filters with mask 0 get nu = 0, S = 0, nis = NaN."""
    B = x.shape[0]
    nu = np.zeros((B, 6)); S = np.zeros((B, 6, 6)); nis = np.full(B, np.nan)
    for i in range(B):
        if mask is not None and not mask[i]:
            continue
        pi = p
        if R is not None:
            pi = copy.copy(p)
            pi.R = np.asarray(R[i], dtype=np.float64)
        nu[i], _, S[i], nis[i] = innovation_ref(pi, x[i], P[i], z[i])
    return nu, S, nis


@pytest.mark.parametrize("est_bias", [1, 0])
@pytest.mark.parametrize("direct", [1, 0])
def test_restatement_reproduces_correction_step(direct, est_bias):
    """K = P G^T S^-1 from the restatement gives correction_step's posterior (x and P) to 1e-12."""
    po = oracle.make_params(update_freq=400.0, direct_orien_method=direct, est_bias=est_bias,
                            r_v_cv=[0.06036412, -0.00145196, -0.04439579], q_vc=[-0.7035177, 0.7106742, 0.0014521, -0.0017207])
    p = ekf_np.Params.from_orc(po)
    n = p.num_states
    rng = np.random.default_rng(11 + 2 * direct + est_bias)
    B = 40
    x, P = rand_states(rng, B, n, cov_scale=0.3)
    z = meas_near(rng, po, x, ang=np.deg2rad(170.0))
    for i in range(B):
        dy, G, S, nis = innovation_ref(p, x[i], P[i], z[i])
        K = P[i] @ G.T @ np.linalg.inv(S)
        Po = (np.eye(n) - K @ G) @ P[i]
        dx = K @ dy
        xo = np.zeros(16)
        xo[0:3] = x[i, 0:3] + dx[0:3]
        xo[3:6] = x[i, 3:6] + dx[3:6]
        xo[6:10] = quaternion_norm(qmul(x[i, 6:10], quaternion_exp(dx[6:9])))
        if est_bias:
            xo[10:13] = x[i, 10:13] + dx[9:12]; xo[13:16] = x[i, 13:16] + dx[12:15]
        xr, Pr, _, _ = ekf_np.correction_step(p, x[i], P[i], z[i, :3], z[i, 3:])
        np.testing.assert_allclose(xo, xr, rtol=0, atol=1e-12)
        np.testing.assert_allclose(Po, Pr, rtol=0, atol=1e-12 * np.abs(Pr).max())
        assert nis > 0 and np.isfinite(nis)
        np.testing.assert_allclose(S, S.T, rtol=0, atol=1e-15 * np.abs(S).max())


def _ctype(decl):
    decl = " ".join(decl.split())
    table = {"qle_batch *": C.c_void_p, "const double *": C.POINTER(C.c_double), "double *": C.POINTER(C.c_double),
             "const uint8_t *": C.POINTER(C.c_uint8), "uint8_t *": C.POINTER(C.c_uint8), "double": C.c_double}
    return table[decl]


def test_lib_binds_innovation_entry_points_with_header_types():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qle_ekf.h")).read(), flags=re.S)
    for name in ("qle_innovation", "qle_update_gated", "qle_step_gated"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{name} not declared"
        args = [re.sub(r"\s*\w+$", "", a.strip()).replace("*", " *").strip() for a in m.group(1).split(",")]
        want = [_ctype(a) for a in args]
        res, got = _lib.SYMBOLS[name]
        assert res is C.c_int
        assert got == want, (name, got, want)
