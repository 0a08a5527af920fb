"""The correction over prior-to-noise ratios, host side: every host-executable route against the truth of tests/golden/ratio_truth.npz
(tests/truth_mp.py, mpmath), and where the constants of the error law come from.

Routes (ROUTES): the dense C oracle and ekf_np.correction_step (fp64 only); the engine's headers compiled for the host -- the
sequential update on the flat covariance ("levels": what k_update and the levelled tick run), the same between the unpack and pack of
the packed multirate replay ("packed"), the batch-form correction on the split covariance ("split": the fp64 multirate replay), all
three through the update-only entry oracle.structured_update_batch on the fixture's truth; and the two routes that exist as whole ticks
only, the fused tick ("fused", structured_run_batch) and the four-lane arithmetic ("quad", quad_run_batch), teacher forced: the truth
is truth_mp.correct on what the route's own predict-only tick leaves (needs mpmath; skipped with that reason without it).

Asserted per (route, dtype, method): the law cov_dev <= C u (1 + rho_eff) holds with a constant that is flat over the decades
(worst / best <= ratio_util.FLAT over all five decades; the two routes of ratio_util.FLAT_EXCEPTIONS, where the host build itself bends
the law downwards, are held flat inside the envelope and to no growth beyond it) and every case inside the envelope stays within
C_HOST x law; fp64 keeps cov_dev below 1e-5 at rho = 1e8; state and
quaternion stay within the stand-alone-update tolerances wherever the route's own P_hat is positive definite; the tables C_HOST and
ENVELOPE of ratio_util.py are what this host measures, rounded up (tests/tolerances_ratio.md).  `python tests/test_ratio_cpu.py`
prints the tables.
"""
import functools
import importlib.util
import math
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":      # run as a script: the repository root is not on the path (pytest gets it from conftest.py)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle
import ratio_util as ru
from oracle import ekf_np

ROUTES = ("oracle_c", "ekf_np", "levels", "packed", "split", "fused", "quad")
FP64_ONLY = ("oracle_c", "ekf_np")
TEACHER_FORCED = ("fused", "quad")
GRID = [(r, d, m) for r in ROUTES for d in ("f64", "f32") for m in (1, 0) if not (d == "f32" and r in FP64_ONLY)]
grid = pytest.mark.parametrize("route,dtype,direct", GRID, ids=[f"{r}-{d}-direct{m}" for r, d, m in GRID])


def _generator():
    spec = importlib.util.spec_from_file_location("make_ratio_truth", os.path.join(ru.GOLDEN, "make_ratio_truth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_is_what_the_generator_makes():
    pytest.importorskip("mpmath")
    made = _generator().generate()
    have = ru.fixture()
    assert sorted(made) == sorted(have)
    for k in made:
        assert made[k].dtype == have[k].dtype and made[k].shape == have[k].shape, k
        assert made[k].tobytes() == have[k].tobytes(), k
    assert os.path.getsize(os.path.join(ru.GOLDEN, "ratio_truth.npz")) < 1024 * 1024


def test_fixture_is_what_the_issue_of_the_axis_needs():
    """float32 inputs, unit quaternions, exactly symmetric P, R(rho) = R(1) / rho, rho_eff growing with the decade."""
    for direct, est_bias in ru.BRANCHES:
        t = ru.table(direct, est_bias)
        assert t["x"].shape == (ru.NCASE, 16) and t["R"].shape == (ru.NCASE, 5, 6)
        for k in ("x", "P", "z", "R"):
            assert np.array_equal(t[k], t[k].astype(np.float32).astype(np.float64)), k
        assert np.array_equal(t["P"], t["P"].transpose(0, 2, 1))
        assert np.abs(np.linalg.norm(t["x"][:, 6:10], axis=1) - 1).max() < 1e-13
        assert np.linalg.eigvalsh(t["P"]).min() > 0 and (t["lam_min"] > 10 * ru.BAND).all()
        for k, rho in enumerate(ru.DECADES):
            assert np.abs(t["R"][:, k] * rho / t["R"][:, 0] - 1).max() < 2.0 ** -23
            assert (t["rho_eff"][:, k] > 0.5 * rho).all() and (t["rho_eff"][:, k] < 20 * rho).all()


def _run_route(route, dtype, direct, est_bias):
    """-> (x_hat [16,5,16], P_hat [16,5,n,n], truth dict with the same leading axes) of one branch."""
    t = ru.table(direct, est_bias)
    n = t["n"]
    truth = {k: t[k] for k in ("x_hat", "P_hat", "rho_eff", "lam_min")}
    xo = np.empty((ru.NCASE, 5, 16)); Po = np.empty((ru.NCASE, 5, n, n))
    if route in ("levels", "packed", "split"):
        po = oracle.make_params(**ru.params_kw(direct, est_bias))
        rep = lambda a: np.repeat(a, 5, axis=0)    # noqa: E731  (case-major: row 5 i + k is case i at decade k)
        x, P = oracle.structured_update_batch(po, rep(t["x"]), rep(t["P"]), rep(t["z"]), t["R"].reshape(-1, 6), dtype=dtype, route=route)
        return x.reshape(ru.NCASE, 5, 16), P.reshape(ru.NCASE, 5, n, n), truth
    if route in TEACHER_FORCED:
        run = (lambda *a, **k: oracle.structured_run_batch(*a, levels="fused", **k)) if route == "fused" else oracle.quad_run_batch
        truth = {k: np.empty_like(v) for k, v in truth.items()}
        for i in range(ru.NCASE):
            x, P, z = t["x"][i:i + 1], t["P"][i:i + 1], t["z"][i:i + 1]
            po = oracle.make_params(**ru.params_kw(direct, est_bias))
            xp, Pp = run(po, x, P, ru.IMU[None, None], dtype=dtype)            # the route's own predict, no tag pose
            tr = ru.truth_correct(direct, est_bias, xp[0], Pp[0], z[0], t["R"][i])
            for k in truth:
                truth[k][i] = tr[k]
            for k in range(5):
                po = oracle.make_params(**ru.params_kw(direct, est_bias, R=t["R"][i, k]))
                xk, Pk = run(po, x, P, ru.IMU[None, None], z[None], np.ones((1, 1), np.uint8), dtype=dtype)
                xo[i, k], Po[i, k] = xk[0], Pk[0]
        return xo, Po, truth
    for i in range(ru.NCASE):
        for k in range(5):
            po = oracle.make_params(**ru.params_kw(direct, est_bias, R=t["R"][i, k]))
            x, P, z = t["x"][i], t["P"][i], t["z"][i]
            if route == "oracle_c":
                xo[i, k], Po[i, k], _, _ = oracle.correction_step(po, x, P, z[:3], z[3:])
            else:
                xo[i, k], Po[i, k], _, _ = ekf_np.correction_step(ekf_np.Params.from_orc(po), x, P, z[:3], z[3:])
    return xo, Po, truth


@functools.lru_cache(maxsize=None)
def measure(route, dtype, direct):
    """Both record sizes of a method, 32 cases x 5 decades -> dict of [32, 5] arrays: cov (cov_dev), state, quat, rho_eff, lam_min (of
    the truth) and own_lam (of the route's own P_hat, correlation-normalised)."""
    out = {k: [] for k in ("cov", "state", "quat", "rho_eff", "lam_min", "own_lam", "sym")}
    for est_bias in (1, 0):
        xo, Po, truth = _run_route(route, dtype, direct, est_bias)
        out["cov"].append(ru.cov_dev_each(Po, truth["P_hat"]))
        out["state"].append(ru.state_dev_each(xo, truth["x_hat"]))
        out["quat"].append(ru.quat_err_each(xo, truth["x_hat"]))
        out["rho_eff"].append(truth["rho_eff"]); out["lam_min"].append(truth["lam_min"])
        out["own_lam"].append(ru.corr_lam_min(Po))
        out["sym"].append(np.abs(Po - np.swapaxes(Po, -1, -2)).max(axis=(-2, -1)))
    return {k: np.concatenate(v) for k, v in out.items()}


def constants(m, dtype):
    """The constant of the law per decade [5]."""
    return np.array([ru.constant(m["cov"][:, k], dtype, m["rho_eff"][:, k]) for k in range(5)])


def envelope(m):
    """The largest decade up to which every case keeps P_hat positive definite with cov_dev < lam_min / 10 (0 if none)."""
    env = 0.0
    for k, rho in enumerate(ru.DECADES):
        if not ((m["own_lam"][:, k] > 0).all() and (m["cov"][:, k] < 0.1 * m["lam_min"][:, k]).all()):
            break
        env = rho
    return env


def round_up(v):
    """v rounded up to one significant digit."""
    e = 10.0 ** math.floor(math.log10(v))
    return math.ceil(v / e - 1e-9) * e


def _need_truth(route):
    if route in TEACHER_FORCED:
        pytest.importorskip("mpmath", reason="the truth of a teacher-forced route is truth_mp.correct at run time")


@grid
def test_the_law_holds_with_a_flat_constant(route, dtype, direct):
    _need_truth(route)
    m = measure(route, dtype, direct)
    c = constants(m, dtype)
    print(f"{route} {dtype} direct{direct}: C per decade " + " ".join(f"{v:.2f}" for v in c) + f"  worst/best {c.max() / c.min():.2f}"
          + f"  envelope {envelope(m):.0e}")
    assert route in FP64_ONLY or (m["sym"] == 0).all()      # the engine holds one triangle; the dense references form (I - K G) P
    ks = [k for k in range(5) if ru.DECADES[k] <= ru.ENVELOPE[route][dtype]]     # the stated envelope, not the one this run finds
    # the tripwire for a kernel or a host route that loses digits: every case inside the envelope within the stated constant
    for k in ks:
        worst = (m["cov"][:, k] / ru.law(dtype, m["rho_eff"][:, k])).max()
        assert worst <= ru.C_HOST[route][dtype][direct], (ru.DECADES[k], worst)
    if (route, dtype, direct) in ru.FLAT_EXCEPTIONS:     # the host build itself bends the law here (ratio_util.FLAT_EXCEPTIONS)
        assert c[ks].max() <= ru.FLAT * c[ks].min(), c                         # flat where the GPU is held to it
        assert all(c[k] <= ru.FLAT * c[:k].min() for k in range(1, 5)), c      # and nowhere growing faster than linearly in rho
        assert c.max() <= ru.FLAT_EXCEPTIONS[(route, dtype, direct)] * c.min(), c
    else:
        assert c.max() <= ru.FLAT * c.min(), c           # worst decade over best, all five decades
    if dtype == "f64":
        assert m["cov"][:, 4].max() < ru.F64_COV_AT_1E8, m["cov"][:, 4].max()


@grid
def test_state_and_quaternion_need_no_scaling(route, dtype, direct):
    """x_hat within the stand-alone-update tolerances in every decade and case whose own P_hat is still positive definite."""
    _need_truth(route)
    m = measure(route, dtype, direct)
    pd = m["own_lam"] > 0
    tol = ru.STATE_TOL[dtype]
    for k in range(5):
        s, q = m["state"][pd[:, k], k], m["quat"][pd[:, k], k]
        print(f"{route} {dtype} direct{direct} rho {ru.DECADES[k]:.0e}: {pd[:, k].sum()} pd, state {s.max(initial=0):.2e} quat {q.max(initial=0):.2e}")
        assert s.max(initial=0) <= tol["state"] and q.max(initial=0) <= tol["quat"], (k, s.max(initial=0), q.max(initial=0))


@grid
def test_tables_of_ratio_util_are_these_numbers_rounded_up(route, dtype, direct):
    """C_HOST bounds what this host measures inside the envelope and is not more than twice its rounded-up value (compilers differ in
    the last digit, not in the decade); ENVELOPE is what this host finds."""
    _need_truth(route)
    m = measure(route, dtype, direct)
    env = min(envelope(measure(route, dtype, d)) for d in (1, 0))
    assert env == ru.ENVELOPE[route][dtype], (env, ru.ENVELOPE[route][dtype])
    inside = [k for k in range(5) if ru.DECADES[k] <= env]
    c = constants(m, dtype)[inside].max()
    stated = ru.C_HOST[route][dtype][direct]
    assert c <= stated <= 2 * round_up(c), (c, stated)


@pytest.mark.parametrize("direct", [1, 0])
def test_undecided_band_is_small_for_the_host_fp32_build(direct):
    """Beyond the envelope the GPU tests compare health()'s not-positive-definite bit with eigvalsh of the GPU's own P_hat, leaving out
    cases whose smallest correlation eigenvalue is within BAND of zero; the fixture's seed keeps those to a quarter of a decade's cases
    for the host fp32 build of the sequential update, per record size."""
    for est_bias in (1, 0):
        _, Po, _ = _run_route("levels", "f32", direct, est_bias)
        lam = ru.corr_lam_min(Po)
        for k in range(5):
            n_in = int((np.abs(lam[:, k]) < ru.BAND).sum())
            print(f"direct{direct} bias{est_bias} rho {ru.DECADES[k]:.0e}: {n_in} inside the band, {int((lam[:, k] <= 0).sum())} not pd")
            assert n_in <= ru.BAND_CAP


if __name__ == "__main__":
    print("| route | dtype | method | C per decade (1, 1e2, 1e4, 1e6, 1e8) | worst/best | C inside envelope | envelope | state | quat |")
    print("|---|---|---|---|---|---|---|---|---|")
    for route, dtype, direct in GRID:
        m = measure(route, dtype, direct)
        c = constants(m, dtype)
        env = min(envelope(measure(route, dtype, d)) for d in (1, 0))
        inside = [k for k in range(5) if ru.DECADES[k] <= env]
        pd = m["own_lam"] > 0
        print(f"| {route} | {dtype} | {'direct' if direct else 'conventional'} | " + " ".join(f"{v:.1f}" for v in c) +
              f" | {c.max() / c.min():.1f} | {c[inside].max():.2f} | {env:.0e} | {m['state'][pd].max():.1e} | {m['quat'][pd].max():.1e} |"
              f"  <!-- not pd per decade {(~pd).sum(axis=0).tolist()} cov at 1e8 {m['cov'][:, 4].max():.1e} -->")
