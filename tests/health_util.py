"""Shared by the lifecycle tests (test_health_cpu.py, test_gpu_lifecycle.py): the list of filter cases a health check must tell apart,
and the numpy restatement of the status byte of include/qle_health.h.

Reference: float64 numpy on exactly the values the code under test holds -- `isfinite`, the sign of `eigvalsh`, plain comparisons.
No tolerance: a status byte is right or wrong.  The one place rounding could decide is the positive-definite test, so every case is
built with |lambda_min| >= 0.5 on either side of zero and `classify` returns that margin for the tests to assert.
"""
import numpy as np

NONFINITE, NOT_PD, QNORM, SIGMA_R, SIGMA_V, SIGMA_THETA = 1, 2, 4, 8, 16, 32
LIMIT = 2.0   # sigma_r_max of the cases: limit^2 = 4 is representable in fp32
LIMITS = dict(sigma_r_max=LIMIT, sigma_v_max=float("inf"), sigma_theta_max=3.0, qnorm_tol=1e-3)
CASE_NAMES = ("healthy", "nan_in_x", "inf_in_P", "indefinite", "q_scaled", "at_limit", "above_limit", "no_state")


def held(dtype, a):
    """a as a handle of `dtype` holds it"""
    return a.astype(np.float32).astype(np.float64) if dtype == "f32" else np.array(a, dtype=np.float64)


def case_list(dtype, n, seed=5):
    """(x [8,16], P [8,n,n]) in the order of CASE_NAMES, as a handle of `dtype` holds them: one healthy filter (P = A A^T + I) and
    seven variations of it."""
    rng = np.random.default_rng(seed + n)
    A = 0.2 * rng.normal(size=(n, n))
    P0 = held(dtype, A @ A.T + np.eye(n))
    P0 = 0.5 * (P0 + P0.T)
    x0 = np.zeros(16)
    x0[0:6] = rng.normal(size=6)
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    x0[6:10] = q
    if n == 15:
        x0[10:16] = 0.01 * rng.normal(size=6)
    x0 = held(dtype, x0)
    x = np.tile(x0, (8, 1)); P = np.tile(P0, (8, 1, 1))
    x[1, 4] = np.nan
    P[2, 1, 7] = P[2, 7, 1] = np.inf
    lam, V = np.linalg.eigh(P0)
    P[3] = held(dtype, P0 - 2.0 * lam[-1] * np.outer(V[:, -1], V[:, -1]))
    P[3] = 0.5 * (P[3] + P[3].T)
    x[4, 6:10] = held(dtype, 1.1 * x0[6:10])
    P[5, 1, 1] = LIMIT ** 2
    P[6, 1, 1] = np.nextafter(np.float32(LIMIT ** 2), np.float32(np.inf)) if dtype == "f32" else np.nextafter(LIMIT ** 2, np.inf)
    x[7] = 0.0
    assert P0.diagonal().max() < LIMIT ** 2
    return x, P


def classify(x, P, sigma_r_max=float("inf"), sigma_v_max=float("inf"), sigma_theta_max=float("inf"), qnorm_tol=1e-3, mask=None):
    """(status [B] uint8, margin): the status bytes of include/qle_health.h restated on the doubles x [B,16], P [B,n,n], and the
    smallest |lambda_min| over the filters whose covariance was factored."""
    B = x.shape[0]
    st = np.zeros(B, np.uint8)
    margin = np.inf
    lim2 = [float(sigma_r_max) ** 2, float(sigma_v_max) ** 2, float(sigma_theta_max) ** 2]
    for i in range(B):
        if (mask is not None and not mask[i]) or not x[i, 6:10].any():
            continue
        if not (np.isfinite(x[i]).all() and np.isfinite(P[i]).all()):
            st[i] = NONFINITE
            continue
        lam_min = np.linalg.eigvalsh(P[i])[0]
        margin = min(margin, abs(lam_min))
        s = NOT_PD if lam_min <= 0.0 else 0
        q = x[i, 6:10]
        qq = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]
        s |= QNORM if abs(qq - 1.0) > qnorm_tol else 0
        d = P[i].diagonal()
        for b, bit in enumerate((SIGMA_R, SIGMA_V, SIGMA_THETA)):
            s |= bit if d[3 * b:3 * b + 3].max() > lim2[b] else 0
        st[i] = s
    return st, margin


def summary_of(status, select, x, mask=None):
    """The nine counts of qhl_summary from status bytes."""
    on = np.ones(len(status), bool) if mask is None else np.asarray(mask) != 0
    init = x[:, 6:10].any(axis=1)   # NaN counts as non-zero, as it does on the device
    out = [int((on & init).sum()), int(((status & select) != 0).sum()), int((on & ~init).sum())]
    return np.array(out + [int(((status >> b) & 1).sum()) for b in range(6)], dtype=np.float64)
