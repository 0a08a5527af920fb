"""Generator of linearisation_truth.npz: corrections and Jacobians from tests/truth_mp.py (mpmath, 80 digits).

    python tests/golden/make_linearisation_truth.py          # rewrites tests/golden/linearisation_truth.npz

Every input (x, P, z, R) is a float32 value, so one fixture serves both engine dtypes and set_state / get_state move it bit for bit; the
truth is computed on those rounded values.  Shared parameters: HW of tests/test_gpu_parity.py at update_freq = 400, with the default
tag noise rounded to float32 (R_shared).  State quaternions are moved to a float32 neighbour whose norm is 1 to 2e-14 (snap_unit): the
reference's G is the model's derivative for unit quaternions only, and a plain float32 rounding leaves 1 - |q|^2 ~ 1e-7 in it.

Per branch d{direct}b{est_bias}:
  40 corrections: states of util.rand_states (cov_scale 0.3; rows 0, 5, .. 35 keep a negative stored w in (-0.75, 0)), z the noise-free
    pose of x [+] dx with |dr| ~ 0.1 m and an attitude innovation angle cycling through ANGLES, the sign of q_ct random; redrawn
    until both w that quaternion_norm inspects (q_tv_obs, delta_q) are 1e-3 away from -0.75.  Truth for the per-filter R and for R_shared.
  4 probe states (identity attitude, r = 0, negative stored w, |r| = 4) with the truth's G and R_k (R_shared).
Covariances and S are stored as upper triangles (row-major).
"""
import os
import sys
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import truth_mp as tm  # noqa: E402
from util import rand_states  # noqa: E402

PATH = os.path.join(HERE, "linearisation_truth.npz")
HW = dict(r_v_cv=[0.06036412, -0.00145196, -0.04439579], q_vc=[-0.7035177, 0.7106742, 0.0014521, -0.0017207])   # test_gpu_parity.HW
R_SHARED = np.array([0.005, 0.005, 0.015, 0.0025, 0.0025, 0.025]).astype(np.float32).astype(np.float64)
THETA_STAR = float(tm.THETA_STAR)
ANGLES = [0.0, 1e-12, 1e-6, 0.5, 3.0, np.pi - 1e-3, np.pi + 1e-3, 4.0, THETA_STAR - 0.01, THETA_STAR + 0.01, 2 * np.pi - 0.5, 2 * np.pi - 1e-6]
NCASE = 40
MARGIN = 1e-3
UNIT_TOL = 2e-14
BRANCHES = [(d, e) for d in (1, 0) for e in (1, 0)]


def tag(direct, est_bias):
    return f"d{direct}b{est_bias}"


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def unit_defect(q):
    return float(abs(sum(Fraction(float(c)) ** 2 for c in q) - 1))


def snap_unit(q, K=128):
    """The float32 quaternion within K ulp per component of q / |q| whose squared norm is closest to 1 (meet in the middle)."""
    q = np.asarray(q, dtype=np.float64)
    q32 = (q / np.linalg.norm(q)).astype(np.float32)
    if unit_defect(q32) == 0.0:
        return q32.astype(np.float64)
    offs = np.arange(-K, K + 1, dtype=np.int32)
    cand = [(np.full(offs.size, c, dtype=np.float32).view(np.int32) + offs).view(np.float32).astype(np.float64) if abs(c) > 1e-3
            else np.array([float(c)]) for c in q32]
    a = (cand[0][:, None] ** 2 + cand[1][None, :] ** 2).ravel()
    b = (cand[2][:, None] ** 2 + cand[3][None, :] ** 2).ravel()
    order = np.argsort(a, kind="stable")
    a_s = a[order]
    pos = np.clip(np.searchsorted(a_s, 1.0 - b), 1, a.size - 1)
    best = None
    for p in (pos - 1, pos):
        err = np.abs(a_s[p] + b - 1.0)
        j = int(np.argmin(err))
        if best is None or err[j] < best[0]:
            best = (err[j], int(order[p[j]]), j)
    _, ia, ib = best
    n1, n3 = cand[1].size, cand[3].size
    out = np.array([cand[0][ia // n1], cand[1][ia % n1], cand[2][ib // n3], cand[3][ib % n3]])
    return out


def triu(M):
    M = np.asarray(M)
    i, j = np.triu_indices(M.shape[-1])
    return M[..., i, j]


def untriu(t, n):
    t = np.asarray(t, dtype=np.float64)
    M = np.zeros(t.shape[:-1] + (n, n))
    i, j = np.triu_indices(n)
    M[..., i, j] = t
    M[..., j, i] = t
    return M


def draw_state(rng, n, negative_w=False):
    while True:
        x, P = rand_states(rng, 1, n, cov_scale=0.3)
        x, P = x[0], P[0]
        if n == 9:
            x[10:16] = 0.0
        if negative_w:
            if not 0.05 < x[9] < 0.7:
                continue
            x[6:10] = -x[6:10]
        x[6:10] = snap_unit(x[6:10])
        if unit_defect(x[6:10]) > UNIT_TOL:      # a coarse lattice near this quaternion: draw another
            continue
        x = f32(x)
        P = f32(P)
        P = np.triu(P) + np.triu(P, 1).T
        return x, P


def make_case(rng, p, direct, i):
    n = p.n
    while True:
        x, P = draw_state(rng, n, negative_w=(i % 5 == 0))
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        dx = np.zeros(n)
        dx[0:3] = rng.normal(size=3) * 0.1
        dx[6:9] = ANGLES[i % 12] * ax
        sign = 1.0 if rng.uniform() < 0.5 else -1.0
        R = f32(R_SHARED * rng.uniform(0.3, 3.0, size=6))
        r_c, q_ct = tm.synth(p, tm.boxplus(tm.vec(x), tm.vec(dx)))
        z = f32(np.concatenate([tm.f64(r_c), sign * tm.f64(q_ct)]))
        ws = []
        tm.residual(p, direct, tm.vec(x), (tm.vec(z[0:3]), tm.vec(z[3:7])), ws)
        if min(abs(float(w) + 0.75) for w in ws) < MARGIN:
            continue
        return x, P, z, R


def probe_states(rng, n):
    xs = []
    for k in range(4):
        x, _ = draw_state(rng, n, negative_w=(k == 2))
        if k == 0:
            x[6:10] = [0.0, 0.0, 0.0, 1.0]
        elif k == 1:
            x[0:3] = 0.0
        elif k == 3:
            x[0:3] = f32(x[0:3] * (4.0 / np.linalg.norm(x[0:3])))
        xs.append(x)
    return np.array(xs)


def generate():
    out = {"R_shared": R_SHARED.astype(np.float32), "angles": np.array(ANGLES)}
    for direct, est_bias in BRANCHES:
        p = tm.Params(est_bias, HW["q_vc"], HW["r_v_cv"])
        n = p.n
        t = tag(direct, est_bias)
        rng = np.random.default_rng(4100 + 2 * direct + est_bias)
        rows = {k: [] for k in ("x", "P", "z", "R", "nu", "w", "pfp__S", "pfp__nis", "pfp__x_hat", "pfp__P_hat",
                                "shared__S", "shared__nis", "shared__x_hat", "shared__P_hat")}
        for i in range(NCASE):
            x, P, z, R = make_case(rng, p, direct, i)
            nu, w_obs, w_dq, res = tm.correct(p, direct, x, P, z, [R, R_SHARED])
            assert min(abs(w_obs + 0.75), abs(w_dq + 0.75)) >= MARGIN
            rows["x"].append(x); rows["P"].append(triu(P)); rows["z"].append(z); rows["R"].append(R)
            rows["nu"].append(nu); rows["w"].append([w_obs, w_dq])
            for name, r in zip(("pfp", "shared"), res):
                rows[f"{name}__S"].append(triu(r["S"])); rows[f"{name}__nis"].append(r["nis"])
                rows[f"{name}__x_hat"].append(r["x_hat"]); rows[f"{name}__P_hat"].append(triu(r["P_hat"]))
        w = np.array(rows["w"])
        for col in range(2):   # both sides of the cover, for the w of q_tv_obs and of delta_q
            assert (w[:, col] < -0.75).any() and (w[:, col] > -0.75).any(), (t, col)
        for k, v in rows.items():
            out[f"{t}__{k}"] = np.array(v, dtype=np.float32 if k in ("x", "P", "z", "R") else np.float64)
        px = probe_states(rng, n)
        out[f"{t}__probe_x"] = px.astype(np.float32)
        out[f"{t}__probe_G"] = np.array([tm.f64(tm.G(p, direct, tm.vec(x))) for x in px])
        out[f"{t}__probe_Rk"] = np.array([tm.f64(tm.R_k(p, direct, tm.vec(x), tm.vec(R_SHARED))) for x in px])
    return out


if __name__ == "__main__":
    np.savez_compressed(PATH, **generate())
    print(PATH, os.path.getsize(PATH), "bytes")
