"""Reader of tests/golden/ratio_truth.npz (made by tests/golden/make_ratio_truth.py from tests/truth_mp.py), the deviation metrics and
the error law of the correction over prior-to-noise ratios, shared by test_ratio_cpu.py and test_gpu_ratio.py.  Needs no mpmath.

P_hat = P - K S K^T keeps a fraction 1 / (1 + rho) of P, so a rounding error of size u |P| is an error of size u (1 + rho) relative
to P_hat: law(dtype, rho_eff).  The constant in front depends on the route and the method, not on the decade; C_HOST is that constant
as the host build of each route measured it (tests/test_ratio_cpu.py, tests/tolerances_ratio.md), rounded up to one digit.  The GPU
tests hold the kernels to GPU_FACTOR x C_HOST x law; no number here comes from a GPU run.
"""
import os

import numpy as np

from linearisation_util import BRANCHES, GOLDEN, HW, rel, untriu  # noqa: F401  (re-exported)
from util import cov_dev, quat_err, state_dev  # noqa: F401  (re-exported)

U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
DECADES = (1.0, 1e2, 1e4, 1e6, 1e8)
NCASE = 16
GPU_FACTOR = 4.0            # device against the host build of the same headers: contracted FMAs, fp32 division and sqrt to 2.5 ulp
FLAT = 8.0                  # the constant of the worst decade over that of the best, at most
# The host build itself bends the law for two routes, downwards: the whole ticks in fp32 with the direct method.  Their constant falls
# from 14 - 16 at rho = 1 to 1.6 - 1.7 at rho = 1e8 (measured two-sided ratio 8.9 / 9.6), where no fp32 P_hat is positive definite any
# more.  For these (route, dtype, direct) the two-sided ratio over all five decades is held to the value here (the measured one rounded
# up); they are held to FLAT inside the envelope and to no growth by FLAT over any lower decade.  Every other route: FLAT, two-sided.
FLAT_EXCEPTIONS = {("fused", "f32", 1): 9.0, ("quad", "f32", 1): 10.0}
F64_COV_AT_1E8 = 1e-5       # every fp64 route keeps cov_dev below this at rho = 1e8
BAND = 1e-3                 # |smallest eigenvalue of the correlation-normalised P_hat| below which positive definiteness is undecided
BAND_CAP = NCASE // 4       # cases of one decade that may lie inside the band
# the stand-alone-update tolerances of tests/test_gpu_parity.py (F32U / F64U): state words and quaternion need no scaling by the law
STATE_TOL = {"f32": dict(state=5e-6, quat=2e-6), "f64": dict(state=2e-11, quat=2e-10)}
IMU = np.array([0.375, -0.25, 9.8125, 0.0625, -0.125, 0.03125])      # the sample of the teacher-forced ticks (float32 values)

# C_HOST[route][dtype][direct]: max over cases and decades inside the envelope of cov_dev / law, host build, rounded up to one digit
# (so 10.4 and 11.2 become 20: up to 2 x of slack on top of GPU_FACTOR; the measured column of tolerances_ratio.md shows what is used).
# util.note lets a NaN deviation pass; here count_nonfinite() == 0 and the eigenvalue checks stand in front of every note.
# (tests/tolerances_ratio.md has the measured values, the host, the compiler and the date).
C_HOST = {
    "oracle_c": {"f64": {1: 10.0, 0: 9.0}},
    "ekf_np": {"f64": {1: 8.0, 0: 8.0}},
    "levels": {"f64": {1: 6.0, 0: 3.0}, "f32": {1: 7.0, 0: 2.0}},
    "packed": {"f64": {1: 6.0, 0: 3.0}, "f32": {1: 7.0, 0: 2.0}},
    "split": {"f64": {1: 8.0, 0: 3.0}, "f32": {1: 20.0, 0: 3.0}},
    "fused": {"f64": {1: 10.0, 0: 4.0}, "f32": {1: 20.0, 0: 2.0}},
    "quad": {"f64": {1: 20.0, 0: 3.0}, "f32": {1: 20.0, 0: 3.0}},
}
# ENVELOPE[route][dtype]: the largest decade in which every case of the host build keeps P_hat positive definite with
# cov_dev < lam_min / 10 (both methods).
ENVELOPE = {r: ({"f64": 1e8} if r in ("oracle_c", "ekf_np") else {"f64": 1e8, "f32": 1e4}) for r in C_HOST}

_FX = None


def fixture():
    global _FX
    if _FX is None:
        with np.load(os.path.join(GOLDEN, "ratio_truth.npz")) as d:
            _FX = {k: d[k] for k in d.files}
    return _FX


def params_kw(direct, est_bias, R=None):
    """Keyword set for oracle.make_params / quadrotor_landing_amd.make_params: HW at 400 Hz; R [6] the shared tag noise, if given."""
    kw = dict(update_freq=400.0, direct_orien_method=direct, est_bias=est_bias, **HW)
    if R is not None:
        kw.update(R_r=[float(v) for v in R[0:3]], R_ang=[float(v) for v in R[3:6]])
    return kw


def table(direct, est_bias):
    """The 16 cases of a branch, covariances expanded, float64 (the inputs are float32 values): x [16,16], P [16,n,n], z [16,7],
    R [16,5,6], rho_eff [16,5] and per decade S [16,5,6,6], nis [16,5], x_hat [16,5,16], P_hat [16,5,n,n], lam_min [16,5]."""
    fx = fixture()
    t = f"d{direct}b{est_bias}__"
    n = 15 if est_bias else 9
    return dict(n=n, x=fx[t + "x"].astype(np.float64), P=untriu(fx[t + "P"], n), z=fx[t + "z"].astype(np.float64),
                R=fx[t + "R"].astype(np.float64), rho_eff=fx[t + "rho_eff"], S=untriu(fx[t + "S"], 6), nis=fx[t + "nis"],
                x_hat=fx[t + "x_hat"], P_hat=untriu(fx[t + "P_hat"], n), lam_min=fx[t + "lam_min"])


def law(dtype, rho_eff):
    return U[dtype] * (1.0 + np.asarray(rho_eff, dtype=np.float64))


def cov_dev_each(P, Pr):
    """cov_dev of util.py per leading-index item."""
    d = np.sqrt(np.einsum("...ii->...i", Pr))
    return (np.abs(P - Pr) / (d[..., :, None] * d[..., None, :] + 1e-300)).max(axis=(-2, -1))


def state_dev_each(x, xr):
    keep = [i for i in range(16) if not 6 <= i < 10]
    return (np.abs(x[..., keep] - xr[..., keep]) / (1.0 + np.abs(xr[..., keep]))).max(axis=-1)


def quat_err_each(x, xr):
    a, b = x[..., 6:10], xr[..., 6:10]
    return np.minimum(np.abs(a - b).max(axis=-1), np.abs(a + b).max(axis=-1))


def constant(dev, dtype, rho_eff):
    """max over cases of dev / law."""
    return float((np.asarray(dev) / law(dtype, rho_eff)).max())


def corr_lam_min(P):
    """Smallest eigenvalue of each P normalised to unit diagonal, float64 eigvalsh; -inf for a P with a non-finite word or a diagonal
    element that is not positive (such a matrix is not positive definite, whatever the rest of it holds)."""
    P = np.asarray(P, dtype=np.float64)
    d2 = np.einsum("...ii->...i", P)
    ok = np.isfinite(P).all(axis=(-2, -1)) & (d2 > 0).all(axis=-1)
    d = np.sqrt(np.where(ok[..., None], d2, 1.0))
    C = np.where(ok[..., None, None], P / (d[..., :, None] * d[..., None, :]), np.eye(P.shape[-1]))
    return np.where(ok, np.linalg.eigvalsh(C)[..., 0], -np.inf)


def truth_correct(direct, est_bias, x, P, z, Rs):
    """truth_mp.correct on run-time inputs (teacher forcing: x, P as a predict left them) -> dict of S, nis, x_hat, P_hat, rho_eff,
    lam_min, each with a leading axis over Rs.  Needs mpmath; cached on the inputs' bits."""
    import truth_mp as tm
    key = (direct, est_bias, x.tobytes(), P.tobytes(), z.tobytes(), np.asarray(Rs).tobytes())
    if key not in _TRUTH:
        p = _TRUTH.setdefault(("params", est_bias), tm.Params(est_bias, HW["q_vc"], HW["r_v_cv"]))
        _, _, _, res = tm.correct(p, direct, x, P, z, list(Rs))
        Nk = tm.N(p, direct, tm.vec(x))
        out = {k: np.array([r[k] for r in res]) for k in ("S", "nis", "x_hat", "P_hat")}
        rho = []
        for R, r in zip(Rs, res):
            Rk = tm.f64(tm.mm([[a * b for a, b in zip(row, tm.vec(R))] for row in Nk], tm.tr(Nk)))
            rho.append(((np.diag(r["S"]) - np.diag(Rk)) / np.diag(Rk)).max())
        out["rho_eff"] = np.array(rho)
        out["lam_min"] = corr_lam_min(out["P_hat"])
        _TRUTH[key] = out
    return _TRUTH[key]


_TRUTH = {}
