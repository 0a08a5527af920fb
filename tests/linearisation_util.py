"""Reader of tests/golden/linearisation_truth.npz (made by tests/golden/make_linearisation_truth.py from tests/truth_mp.py) and the
probe covariances, shared by test_linearisation_cpu.py and test_gpu_linearisation.py.  Needs no mpmath."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HW = dict(ab_static=[0.2, -0.09, -0.03], wb_static=[-0.02, -0.01, 0.0], r_v_cv=[0.06036412, -0.00145196, -0.04439579],
          q_vc=[-0.7035177, 0.7106742, 0.0014521, -0.0017207])            # HW of tests/test_gpu_parity.py
BRANCHES = [(d, e) for d in (1, 0) for e in (1, 0)]
THETA_STAR = 2 * np.arccos(-0.75)
_FX = None


def fixture():
    global _FX
    if _FX is None:
        with np.load(os.path.join(GOLDEN, "linearisation_truth.npz")) as d:
            _FX = {k: d[k] for k in d.files}
    return _FX


def untriu(t, n):
    t = np.asarray(t, dtype=np.float64)
    M = np.zeros(t.shape[:-1] + (n, n))
    i, j = np.triu_indices(n)
    M[..., i, j] = t
    M[..., j, i] = t
    return M


def params_kw(direct, est_bias):
    """Keyword set for oracle.make_params / quadrotor_landing_amd.make_params: HW at 400 Hz with the fixture's shared tag noise."""
    R = fixture()["R_shared"].astype(np.float64)
    return dict(update_freq=400.0, direct_orien_method=direct, est_bias=est_bias, R_r=list(R[0:3]), R_ang=list(R[3:6]), **HW)


def table(direct, est_bias):
    """The 40 corrections of a branch, covariances expanded, as float64 (the inputs are float32 values)."""
    fx = fixture()
    t = f"d{direct}b{est_bias}__"
    n = 15 if est_bias else 9
    out = dict(n=n, x=fx[t + "x"].astype(np.float64), P=untriu(fx[t + "P"], n), z=fx[t + "z"].astype(np.float64),
               R=fx[t + "R"].astype(np.float64), R_shared=fx["R_shared"].astype(np.float64), nu=fx[t + "nu"], w=fx[t + "w"],
               angle=fx["angles"][np.arange(fx[t + "x"].shape[0]) % len(fx["angles"])])
    for v in ("pfp", "shared"):
        out[v] = dict(S=untriu(fx[f"{t}{v}__S"], 6), nis=fx[f"{t}{v}__nis"], x_hat=fx[f"{t}{v}__x_hat"], P_hat=untriu(fx[f"{t}{v}__P_hat"], n))
    return out


def probes(direct, est_bias):
    """(x [4,16], G [4,6,n], R_k [4,6,6]): identity attitude, r = 0, negative stored w, |r| = 4."""
    fx = fixture()
    t = f"d{direct}b{est_bias}__"
    return fx[t + "probe_x"].astype(np.float64), fx[t + "probe_G"], fx[t + "probe_Rk"]


def probe_covs(n):
    """P = 0, e_i e_i^T and (e_i + e_j)(e_i + e_j)^T, i < j: 1 + n (n + 1) / 2 covariances from which every g_i g_j^T of
    S - R_k = G P G^T can be read, so that an error in one column of G cannot hide in a sum."""
    P = [np.zeros((n, n))]
    I = np.eye(n)
    for i in range(n):
        P.append(np.outer(I[i], I[i]))
    for i in range(n):
        for j in range(i + 1, n):
            P.append(np.outer(I[i] + I[j], I[i] + I[j]))
    return np.array(P)


def rel(a, b):
    """max |a - b| over the largest |b| of each leading-index item."""
    scale = np.abs(b).max(axis=tuple(range(1, b.ndim)), keepdims=True)
    return float((np.abs(a - b) / np.maximum(scale, 1e-300)).max())
