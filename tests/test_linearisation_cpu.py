"""The conventional linearisation and the delta_q flip of correction_step, held to a truth derived from the measurement model.

tests/truth_mp.py differentiates the twin-pinned direct observation in mpmath; nothing of G, the conventional r_obs or the flip is typed
into it.  Here: (a) the committed fixture is what the generator makes; (b) the truth's G is the exact first derivative of its residual,
and the innovations of the C oracle and of innovation_ref obey the same second-order bound; (c) G and R_k of innovation_ref, column by
column, through probe covariances; (d) ekf_oracle.c and ekf_np.correction_step against the truth's 160 corrections; (e) what the flip
must preserve.  The C oracle exports no innovation and rank-one probe covariances leave S unrecoverable from (P, P_hat), so (c) runs
through innovation_ref only; the C oracle's G is held by (d).  Tolerances: tests/tolerances_linearisation.md.
"""
import importlib.util
import os

import numpy as np
import pytest

import oracle
import truth_mp as tm
from linearisation_util import BRANCHES, GOLDEN, HW, THETA_STAR, fixture, params_kw, probe_covs, probes, rel, table
from oracle import ekf_np
from innovation_util import innovation_ref
from util import cov_dev, quat_err, state_dev

branches = pytest.mark.parametrize("direct,est_bias", BRANCHES, ids=[f"direct{d}-bias{e}" for d, e in BRANCHES])

# (d): 50 x the deviation measured on the CPU, rounded up to one digit (tests/tolerances_linearisation.md)
# measured worst over the 8 parametrisations: state 1.5e-14, quat 4.8e-15, cov 2.8e-13, nu 3.4e-14, S 3.4e-14, NIS 3.3e-14
TOL_D = dict(state=8e-13, quat=3e-13, cov=2e-11, nu=2e-12, S=2e-12, nis=2e-12)
# (c): S = G P G^T + R_k in float64, relative to its largest element: two products of at most 15 terms (30 eps = 3.3e-15), entries of
# G up to |r| = 4 against a largest element of (2 |r|)^2, the state quaternion unit to 2e-14 (fixture) -> 4e-14 in G G^T; stated 1e-13.
TOL_C = 1e-13


def _generator():
    spec = importlib.util.spec_from_file_location("make_linearisation_truth", os.path.join(GOLDEN, "make_linearisation_truth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_is_what_the_generator_makes():
    pytest.importorskip("mpmath")
    made = _generator().generate()
    have = fixture()
    assert sorted(made) == sorted(have)
    for k in made:
        assert made[k].dtype == have[k].dtype and made[k].shape == have[k].shape, k
        assert made[k].tobytes() == have[k].tobytes(), k
    assert os.path.getsize(os.path.join(GOLDEN, "linearisation_truth.npz")) < 400 * 1024


def _np_params(direct, est_bias, R=None):
    p = ekf_np.Params.from_orc(oracle.make_params(**params_kw(direct, est_bias)))
    if R is not None:
        p.R = np.asarray(R, dtype=np.float64)
    return p


DIRS = np.random.default_rng(77).normal(size=(16, 15))
DIRS[:, 3:6] = 0.0; DIRS[:, 9:15] = 0.0          # the residual does not see v or the biases: the norm goes to (dr, dtheta)
DIRS /= np.linalg.norm(DIRS, axis=1, keepdims=True)
EPS = (1e-2, 5e-3, 1e-3)


def _remainder(p, direct, x, Gk, d, eps):
    """(|position rows|, |rotation rows|) of residual(x, synth(x [+] eps d)) - G eps d, in mpmath; and the tag pose."""
    dx = [tm.mpf(float(v)) * tm.mpf(eps) for v in d]
    z = tm.synth(p, tm.boxplus(x, dx))
    res = tm.residual(p, direct, x, z)
    rem = [a - b for a, b in zip(res, tm.mv(Gk, dx))]
    return tm.mp.sqrt(tm.mp.fsum(c * c for c in rem[0:3])), tm.mp.sqrt(tm.mp.fsum(c * c for c in rem[3:6])), z


@pytest.mark.parametrize("direct", [1, 0])
def test_truth_G_is_the_first_derivative_and_restatements_follow(direct):
    """(b): rotation rows exact, position rows second order with the constant (1 + |r|) / 2 (doubled for the third order at
    eps <= 1e-2: |C [dtheta]x C^T dr| + |C [dtheta]x^2 C^T r| / 2 <= (1 + |r|) eps^2 / 2), and the remainder quarters when eps halves."""
    est_bias = 1
    p = tm.Params(est_bias, HW["q_vc"], HW["r_v_cv"])
    pn = _np_params(direct, est_bias)
    po = oracle.make_params(**params_kw(direct, est_bias))
    xs, _, _ = probes(direct, est_bias)
    P = np.eye(15) * 0.1
    for x64 in xs:
        x = tm.vec(x64)
        Gk = tm.G(p, direct, x)
        Gf = tm.f64(Gk)
        rn = float(np.linalg.norm(x64[0:3]))
        for eps in EPS:
            bound = (1 + rn) * eps ** 2
            for d in DIRS:
                e_r, e_t, z = _remainder(p, direct, x, Gk, d, eps)
                assert e_t < tm.mpf(10) ** -40, (eps, float(e_t))
                assert e_r <= bound, (eps, float(e_r), bound)
                # the restatements' innovations, float64: numpy with its own G, the C oracle with the truth's
                z64 = np.concatenate([tm.f64(z[0]), tm.f64(z[1])])
                dy, Gn, _, _ = innovation_ref(pn, x64, P, z64)
                assert np.linalg.norm(dy - Gn @ (eps * d)) <= bound
                _, _, r_obs, q_obs = oracle.correction_step(po, x64, P, z64[:3], z64[3:])
                dq = oracle.quat_mul(x64[6:10] * [-1, -1, -1, 1], q_obs)
                dyc = np.concatenate([r_obs - x64[0:3], oracle.quaternion_log(oracle.quaternion_norm(dq))])
                assert np.linalg.norm(dyc - Gf @ (eps * d)) <= bound
        if not direct and rn > 0:
            e1 = _remainder(p, direct, x, Gk, DIRS[0], 1e-2)[0]
            e2 = _remainder(p, direct, x, Gk, DIRS[0], 5e-3)[0]
            assert 3.5 <= e1 / e2 <= 4.5, float(e1 / e2)       # a first-order error in G would give 2


@branches
def test_restatement_G_and_Rk_column_by_column(direct, est_bias):
    """(c): innovation_ref's S on the probe covariances against the truth's G P G^T + R_k."""
    pn = _np_params(direct, est_bias)
    n = pn.num_states
    xs, Gt, Rkt = probes(direct, est_bias)
    Ps = probe_covs(n)
    assert len(Ps) == 1 + n * (n + 1) // 2
    z = np.array([0.1, -0.2, 2.0, 0.0, 0.0, 0.0, 1.0])
    worst = 0.0
    for x, Gk, Rk in zip(xs, Gt, Rkt):
        S = np.array([innovation_ref(pn, x, P, z)[2] for P in Ps])
        worst = max(worst, rel(S, Gk @ Ps @ Gk.T + Rk))
        assert rel(S[:1], Rk[None]) <= TOL_C
    print(f"probe S, direct={direct} est_bias={est_bias}: {worst:.2e}")
    assert worst <= TOL_C


def _oracle_nu(po, x, q_obs, r_obs):
    dq = oracle.quat_mul(x[6:10] * [-1, -1, -1, 1], q_obs)
    return np.concatenate([r_obs - x[0:3], oracle.quaternion_log(oracle.quaternion_norm(dq))])


@pytest.mark.parametrize("variant", ["pfp", "shared"])
@branches
def test_case_table_oracles_against_truth(direct, est_bias, variant):
    """(d): both restatements of correction_step (and innovation_ref's nu, S, NIS) on the truth's 40 corrections of the branch."""
    t = table(direct, est_bias)
    truth = t[variant]
    n = t["n"]
    dev = {k: 0.0 for k in ("c_state", "c_quat", "c_cov", "c_nu", "np_state", "np_quat", "np_cov", "nu", "S", "nis")}
    for i in range(len(t["x"])):
        R = t["R"][i] if variant == "pfp" else t["R_shared"]
        po = oracle.make_params(**dict(params_kw(direct, est_bias), R_r=list(R[0:3]), R_ang=list(R[3:6])))
        pn = ekf_np.Params.from_orc(po)
        x, P, z = t["x"][i], t["P"][i], t["z"][i]
        xh, Ph = truth["x_hat"][i:i + 1], truth["P_hat"][i:i + 1]
        xc, Pc, r_obs, q_obs = oracle.correction_step(po, x, P, z[:3], z[3:])
        xn, Pn, _, _ = ekf_np.correction_step(pn, x, P, z[:3], z[3:])
        dy, _, S, nis = innovation_ref(pn, x, P, z)
        for name, xo, Po in (("c", xc, Pc), ("np", xn, Pn)):
            dev[f"{name}_state"] = max(dev[f"{name}_state"], state_dev(xo[None], xh))
            dev[f"{name}_quat"] = max(dev[f"{name}_quat"], quat_err(xo[None, 6:10], xh[:, 6:10]))
            dev[f"{name}_cov"] = max(dev[f"{name}_cov"], cov_dev(Po[None], Ph))
        dev["c_nu"] = max(dev["c_nu"], rel(_oracle_nu(po, x, q_obs, r_obs)[None], t["nu"][i:i + 1]))
        dev["nu"] = max(dev["nu"], rel(dy[None], t["nu"][i:i + 1]))
        dev["S"] = max(dev["S"], rel(S[None], truth["S"][i:i + 1]))
        dev["nis"] = max(dev["nis"], abs(nis / truth["nis"][i] - 1))
    print(f"direct={direct} est_bias={est_bias} {variant}: " + " ".join(f"{k} {v:.2e}" for k, v in dev.items()))
    for k, v in dev.items():
        assert v <= TOL_D[k.split("_")[-1]], (k, v)


def _as_rotation(q):
    return ekf_np.rot(np.asarray(q) / np.linalg.norm(q))


@branches
def test_flip_preserves_the_rotation(direct, est_bias):
    """(e): whatever cover quaternion_norm uses, exp(nu_theta) is the rotation conj(q) q_obs, |nu_theta| <= theta*, and the corrected
    quaternion is a unit one with w >= -0.75 -- truth and oracle, every row; the table has rows on both sides of the cover."""
    t = table(direct, est_bias)
    pn = _np_params(direct, est_bias)
    po = oracle.make_params(**params_kw(direct, est_bias))
    for col in range(2):
        assert (t["w"][:, col] < -0.75).any() and (t["w"][:, col] > -0.75).any()
        assert (np.abs(t["w"][:, col] + 0.75) >= 1e-3).all()
    for i in range(len(t["x"])):
        x, P, z = t["x"][i], t["P"][i], t["z"][i]
        _, q_obs = ekf_np.observe(pn, None, z[:3], z[3:])
        want = _as_rotation(x[6:10]).T @ _as_rotation(q_obs)
        xc, _, r_obs, q_obs_c = oracle.correction_step(po, x, P, z[:3], z[3:])
        xn, _, _, _ = ekf_np.correction_step(pn, x, P, z[:3], z[3:])
        nus = dict(truth=t["nu"][i], numpy=innovation_ref(pn, x, P, z)[0], c=_oracle_nu(po, x, q_obs_c, r_obs))
        for name, nu in nus.items():
            ang = np.linalg.norm(nu[3:6])
            assert ang <= THETA_STAR + 1e-12, (name, i, ang)
            got = ekf_np.rodrigues(ang, nu[3:6] / ang) if ang > 0 else np.eye(3)
            assert np.abs(got - want).max() <= 1e-13, (name, i)         # float64 rotation matrices, a few eps at angles up to 4.84
        for name, xh in (("truth_pfp", t["pfp"]["x_hat"][i]), ("truth_shared", t["shared"]["x_hat"][i]), ("c", xc), ("numpy", xn)):
            assert abs(np.linalg.norm(xh[6:10]) - 1) <= 1e-15 and xh[9] >= -0.75, (name, i)
