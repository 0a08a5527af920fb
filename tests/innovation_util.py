"""The numpy restatement of the innovation that the CPU and GPU tests of the diagnostics and the gate check the engine against: the first
half of oracle/ekf_np.correction_step (relative_pose_EKF.cpp:417-475) -- the innovation delta_y, G, N, R_k = N R N^T,
S = G P G^T + R_k -- and NIS = delta_y^T S^-1 delta_y.  tests/test_innovation_cpu.py holds it to correction_step itself."""
import copy

import numpy as np

from oracle.ekf_np import observe, qconj, qmul, quaternion_log, quaternion_norm, rot, skew

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
