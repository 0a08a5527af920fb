"""Shared by the consistency tests (test_consistency_cpu.py, test_gpu_consistency.py): the construction of states, covariances and
truths, the numpy reference of NEES = e^T P^-1 e, and the tolerance it is held to.

Reference: float64 numpy on exactly the values the code under test was given -- the error vector of include/qle_consistency.h with the
quaternion helpers of oracle/ekf_np.py, `np.linalg.solve` on the selected sub-matrix.  The marginal is taken by SLICING, so the
identity-row device of nees_eval (e_j = 0, P_jj = 1, zero row and column for an unselected state) is checked, not restated.

Tolerance (derived, not tuned): an L D L^T solve is backward stable and its error is governed by the condition number of the
diagonally scaled matrix, so per filter
    |nees - ref| <= 16 n kappa(C_i) u ref,   C_i = D^-1 P_i D^-1, D = sqrt(diag P_i),   u = 2^-24 (fp32) / 2^-53 (fp64),
n the handle's number of states, kappa(C_i) computed here from the P the code was given.  At kappa = 100 and n = 15 this is 1.4e-3 in
fp32; a wrong index in the packed factor shows as an error of order 1.  err is held to 8 u relative to its block's norm, the attitude
block absolutely to 8 u pi.
"""
import numpy as np

from oracle import ekf_np
from util import qmul, rand_states

U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
# standard deviations of the five blocks r [m], v [m/s], theta [rad], ab [m/s^2], wb [rad/s]: the real spread of a landing filter's
# covariance, 1 down to 1e-4, so that only the conditioning of the correlation matrix matters
BLOCK_SCALE = np.array([1.0, 0.3, 0.03, 1e-2, 1e-4])
KAPPA_MAX = 100.0
NAMED_BLOCKS = {"all": 31, "pose": 5, "r": 1, "theta": 4, "r+theta+ab+wb": 29}


def rand_corr(rng, B, n, kappa_max=KAPPA_MAX):
    """B random correlation matrices (unit diagonal) with 2-norm condition number <= 0.9 kappa_max: eigenvalues log-uniform over a
    random spread, a random orthogonal basis, rescaled to unit diagonal and redrawn where the rescaling left kappa too large."""
    out = np.empty((B, n, n))
    for i in range(B):
        while True:
            Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
            lam = np.exp(rng.uniform(0.0, np.log(rng.uniform(1.5, kappa_max)), size=n))
            A = (Q * lam) @ Q.T
            s = 1.0 / np.sqrt(np.diag(A))
            Cm = A * s[:, None] * s[None, :]
            Cm = 0.5 * (Cm + Cm.T)
            np.fill_diagonal(Cm, 1.0)
            if np.linalg.cond(Cm) <= 0.9 * kappa_max:
                break
        out[i] = Cm
    return out


def quat_exp_batch(v):
    a = np.linalg.norm(v, axis=1, keepdims=True)
    k = np.where(a > 1e-12, np.sin(a / 2) / np.where(a > 1e-12, a, 1.0), 0.5)
    return np.concatenate([v * k, np.cos(a / 2)], axis=1)


def displace(x, e, ab_static, wb_static):
    """The truth rows [B,16] that lie at error e [B,n] from the states x: r + e_r, v + e_v, q (x) exp(e_theta), and the TOTAL true
    biases nom + static + e."""
    B, n = e.shape
    xt = np.zeros((B, 16))
    xt[:, 0:6] = x[:, 0:6] + e[:, 0:6]
    xt[:, 6:10] = qmul(x[:, 6:10], quat_exp_batch(e[:, 6:9]))
    xt[:, 10:13] = x[:, 10:13] + ab_static
    xt[:, 13:16] = x[:, 13:16] + wb_static
    if n == 15:
        xt[:, 10:16] += e[:, 9:15]
    return xt


def make_case(rng, B, n, dtype, ab_static, wb_static):
    """(x, P, x_true): states from util.rand_states, P = D C D with C a random correlation matrix (kappa <= 100) and D the real spread
    of scales, the truth displaced by errors drawn from the filter's own P (e = L xi); one eighth of the cases with an attitude error
    of 90..170 degrees instead, one eighth with a truth quaternion of w < 0.  Rounded to what a handle of `dtype` holds."""
    x, _ = rand_states(rng, B, n)
    if n == 9:
        x[:, 10:16] = 0.0
    d = np.repeat(BLOCK_SCALE[:n // 3], 3)[None, :] * rng.uniform(0.5, 1.0, size=(B, n))
    P = rand_corr(rng, B, n) * d[:, :, None] * d[:, None, :]
    e = np.einsum("bij,bj->bi", np.linalg.cholesky(P), rng.normal(size=(B, n)))
    big = np.arange(B) % 8 == 3
    ax = rng.normal(size=(B, 3)); ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    e[big, 6:9] = (ax * np.deg2rad(rng.uniform(90.0, 170.0, size=(B, 1))))[big]
    xt = displace(x, e, ab_static, wb_static)
    neg = np.arange(B) % 8 == 5
    xt[neg, 6:10] *= -np.sign(xt[neg, 9:10])
    assert (xt[neg, 9] < 0).all()
    if dtype == "f32":
        x, P, xt = (a.astype(np.float32).astype(np.float64) for a in (x, P, xt))
    return x, P, xt


def err_ref(x, xt, ab_static, wb_static, n):
    """e [B,n]: truth minus estimate in the error-state convention, float64, the reference's quaternion helpers."""
    B = x.shape[0]
    e = np.zeros((B, 15))
    e[:, 0:6] = xt[:, 0:6] - x[:, 0:6]
    for i in range(B):
        e[i, 6:9] = ekf_np.quaternion_log(ekf_np.quaternion_norm(ekf_np.qmul(ekf_np.qconj(x[i, 6:10]), xt[i, 6:10])))
    # truth - (nom + static) in extended precision: the bias error is orders of magnitude below the biases, and in float64 the sum's own
    # rounding (u |bias|) would be 10 - 100 x the bar of 8 u |e| this reference is used to hold
    ld = np.longdouble
    e[:, 9:12] = (xt[:, 10:13].astype(ld) - (x[:, 10:13].astype(ld) + np.asarray(ab_static, ld))).astype(np.float64)
    e[:, 12:15] = (xt[:, 13:16].astype(ld) - (x[:, 13:16].astype(ld) + np.asarray(wb_static, ld))).astype(np.float64)
    return e[:, :n]


def selected(blocks, n):
    return [j for j in range(n) if (blocks >> (j // 3)) & 1]


def nees_ref(P, e, blocks):
    """e_s^T P_ss^-1 e_s with the marginal taken by slicing."""
    sel = selected(blocks, P.shape[1])
    Ps = P[:, sel][:, :, sel]
    es = e[:, sel]
    return np.einsum("bi,bi->b", es, np.linalg.solve(Ps, es[:, :, None])[:, :, 0])


def kappa_scaled(P):
    """2-norm condition number of D^-1 P D^-1, D = sqrt(diag P), per filter."""
    d = np.sqrt(np.einsum("bii->bi", P))
    return np.linalg.cond(P / (d[:, :, None] * d[:, None, :]))


def nees_tol(P, ref, dtype):
    return 16.0 * P.shape[1] * kappa_scaled(P) * U[dtype] * np.abs(ref)


def nees_ratio(nees, ref, P, dtype):
    """worst |nees - ref| / tolerance over the batch (must be <= 1); a non-finite value counts as infinite"""
    r = np.abs(nees - ref) / nees_tol(P, ref, dtype)
    return float(np.where(np.isfinite(r), r, np.inf).max())


def err_ratio(err, eref, dtype):
    """worst deviation of err from the reference over its bars: 8 u x the block's 2-norm (r, v, ab, wb), 8 u pi absolutely (theta)"""
    u = U[dtype]
    worst = 0.0
    for b in range(eref.shape[1] // 3):
        s = slice(3 * b, 3 * b + 3)
        dev = np.abs(err[:, s] - eref[:, s]).max(axis=1)
        bar = np.full(len(dev), 8.0 * u * np.pi) if b == 2 else 8.0 * u * np.linalg.norm(eref[:, s], axis=1)
        ok = dev <= bar
        r = np.where(bar > 0, dev / np.where(bar > 0, bar, 1.0), np.where(ok, 0.0, np.inf))
        worst = max(worst, float(np.where(np.isfinite(r), r, np.inf).max()))
    return worst
