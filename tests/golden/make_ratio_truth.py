"""Generator of ratio_truth.npz: one correction per case at five prior-to-noise ratios, from tests/truth_mp.py (mpmath, 80 digits).

    python tests/golden/make_ratio_truth.py          # rewrites tests/golden/ratio_truth.npz

P_hat = P - K S K^T cancels all but a fraction 1 / (1 + rho) of P, rho the ratio of G P G^T to R_k, so the rounding error of P_hat
relative to its own scale grows like u (1 + rho).  This fixture walks that axis: per case one state, covariance and tag pose, and the
noise vectors R(rho) = R(1) / rho for rho = 1, 1e2, 1e4, 1e6, 1e8, passed to truth_mp.correct as one Rs list.

Every input (x, P, z, R) is a float32 value, as in make_linearisation_truth.py (same HW, 400 Hz; state quaternions snapped to a
float32 neighbour whose squared norm is 1 to 1e-15, a wider search than that fixture's).  Per branch d{direct}b{est_bias}, 16 cases:
  state: util.rand_states words, rows 0, 5, 10, 15 with a negative stored w in (-0.75, 0);
  covariance: D (0.7 C + 0.3 I) D, C a random correlation matrix, D^2 the variances the filters carry (r, v 0.1, theta 0.05, ab 0.01,
    wb 0.001, each times a factor in 0.5 .. 2), rounded to float32 and mirrored from the upper triangle;
  tag pose: the noise-free pose of x [+] dx, |dr| ~ 0.02 m, |dtheta| ~ 0.02 rad, sign of q_ct random: the update stays in the linear
    regime; redrawn until both w that quaternion_norm inspects are 1e-3 away from -0.75;
  noise: R(rho) = float32((0.1, 0.1, 0.1, 0.05, 0.05, 0.05) / rho), the same for every case: one decade of the fixture is also a batch with
    shared parameters.
Stored per case: x, P, z, R [5, 6], rho_eff [5] = max_k (S - R_k)_kk / (R_k)_kk of the truth; per decade S, nis, x_hat, P_hat and
lam_min, the smallest eigenvalue of P_hat normalised to unit diagonal (the room a rounding error has before P_hat stops being positive
definite).  Covariances and S are stored as upper triangles (row-major).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import truth_mp as tm  # noqa: E402
from make_linearisation_truth import BRANCHES, HW, MARGIN, draw_state, f32, snap_unit, tag, triu, unit_defect  # noqa: E402

PATH = os.path.join(HERE, "ratio_truth.npz")
DECADES = np.array([1.0, 1e2, 1e4, 1e6, 1e8])
NCASE = 16
SEED = 7300
UNIT_TOL = 1e-15     # the dense fp64 routes resolve 1 - |q|^2 of the linearisation fixture (2e-14) at rho = 1: a wider search here
VAR = np.array([0.1] * 6 + [0.05] * 3 + [0.01] * 3 + [0.001] * 3)
R_ONE = np.array([0.1, 0.1, 0.1, 0.05, 0.05, 0.05])


def draw_cov(rng, n):
    A = rng.normal(size=(n, n))
    C = A @ A.T
    s = 1.0 / np.sqrt(np.diag(C))
    C = 0.7 * (C * s[:, None] * s[None, :]) + 0.3 * np.eye(n)
    d = np.sqrt(VAR[:n] * rng.uniform(0.5, 2.0, size=n))
    P = f32(C * d[:, None] * d[None, :])
    return np.triu(P) + np.triu(P, 1).T


def make_case(rng, p, direct, i):
    n = p.n
    while True:
        x, _ = draw_state(rng, n, negative_w=(i % 5 == 0))
        x[6:10] = snap_unit(x[6:10], K=512)
        if unit_defect(x[6:10]) > UNIT_TOL:
            continue
        P = draw_cov(rng, n)
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        dx = np.zeros(n)
        dx[0:3] = rng.normal(size=3) * 0.02
        dx[6:9] = 0.02 * rng.uniform(0.5, 1.5) * ax
        sign = 1.0 if rng.uniform() < 0.5 else -1.0
        R = f32(R_ONE[None, :] / DECADES[:, None])
        r_c, q_ct = tm.synth(p, tm.boxplus(tm.vec(x), tm.vec(dx)))
        z = f32(np.concatenate([tm.f64(r_c), sign * tm.f64(q_ct)]))
        ws = []
        tm.residual(p, direct, tm.vec(x), (tm.vec(z[0:3]), tm.vec(z[3:7])), ws)
        if min(abs(float(w) + 0.75) for w in ws) < MARGIN:
            continue
        return x, P, z, R


def rho_eff(p, direct, x, R, S):
    """max_k (S - R_k)_kk / (R_k)_kk with the truth's own R_k = N R N^T."""
    Rk = tm.f64(tm.R_k(p, direct, tm.vec(x), tm.vec(R)))
    return float(((np.diag(S) - np.diag(Rk)) / np.diag(Rk)).max())


def lam_min(P_hat):
    s = 1.0 / np.sqrt(np.diag(P_hat))
    return float(np.linalg.eigvalsh(P_hat * s[:, None] * s[None, :])[0])


def generate():
    out = {"decades": DECADES}
    for direct, est_bias in BRANCHES:
        p = tm.Params(est_bias, HW["q_vc"], HW["r_v_cv"])
        t = tag(direct, est_bias)
        rng = np.random.default_rng(SEED + 2 * direct + est_bias)
        rows = {k: [] for k in ("x", "P", "z", "R", "rho_eff", "S", "nis", "x_hat", "P_hat", "lam_min")}
        for i in range(NCASE):
            x, P, z, R = make_case(rng, p, direct, i)
            _, w_obs, w_dq, res = tm.correct(p, direct, x, P, z, list(R))
            assert min(abs(w_obs + 0.75), abs(w_dq + 0.75)) >= MARGIN
            assert unit_defect(x[6:10]) <= UNIT_TOL and np.array_equal(x, f32(x))
            rows["x"].append(x); rows["P"].append(triu(P)); rows["z"].append(z); rows["R"].append(R)
            rows["rho_eff"].append([rho_eff(p, direct, x, Rd, r["S"]) for Rd, r in zip(R, res)])
            rows["S"].append([triu(r["S"]) for r in res]); rows["nis"].append([r["nis"] for r in res])
            rows["x_hat"].append([r["x_hat"] for r in res]); rows["P_hat"].append([triu(r["P_hat"]) for r in res])
            rows["lam_min"].append([lam_min(r["P_hat"]) for r in res])
        for k, v in rows.items():
            out[f"{t}__{k}"] = np.array(v, dtype=np.float32 if k in ("x", "P", "z", "R") else np.float64)
    return out


if __name__ == "__main__":
    np.savez_compressed(PATH, **generate())
    print(PATH, os.path.getsize(PATH), "bytes")
