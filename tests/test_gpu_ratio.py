"""The correcting kernels over prior-to-noise ratios, against the truth of tests/golden/ratio_truth.npz (tests/truth_mp.py, mpmath).

P_hat = P - K S K^T keeps a fraction 1 / (1 + rho) of P, so the rounding error of P_hat relative to its own scale grows like
u (1 + rho).  Every kernel that corrects is held to GPU_FACTOR (4) x C_HOST x u (1 + rho_eff) per case: C_HOST is the constant the HOST
build of the same route measured (tests/test_ratio_cpu.py, tests/tolerances_ratio.md; ratio_util.C_HOST), the factor 4 what separates
the device from that build (contracted FMAs; fp32 division and sqrt good to 2.5 ulp where the host divides exactly).  No bound here
comes from a GPU run.

Routes and the host route whose constant bounds them:
  update      k_update: fp32 the sequential update on the flat covariance ("levels"), fp64 the batch form on the split one ("split");
  innovation  k_innov: S and NIS, held to the bounds of test_gpu_innovation.py unscaled (they divide by the pivots of S, whose
              condition does not grow with rho);
  step        the fused tick: k_step ("fused") with QLE_QUAD=0 and on compact records, kw_tick ("quad") with QLE_QUAD=3 on full records,
              either by default on full records (the larger constant); full, 9-state and compact records;
  resident    k_run_resident over a one-tick sequence: ekf_update_split in fp64 ("split"), ekf_update_emit in fp32 ("levels").
              step and resident are teacher forced: the truth is truth_mp.correct, at run time, on what the handle's own predict of
              the same inputs leaves (needs mpmath; skipped with that reason without it);
  multirate   k_step_mr at a fixed delay of 1 tick (the smallest) and of 2: the correction reaches the history entry that set_state
              wrote, so the fixture's truth applies to it directly and the oracle's fp64 predicts replay it forward; fp32 corrects
              between cov_unpack and cov_pack ("packed"), fp64 in batch form on the split covariance ("split").
Batches: 80 filters = 16 cases x 5 decades with per-filter tag noise, case-major, so the first wave holds every decade; 16-filter
handles with shared parameters, one per decade, for update, innovation, step and resident; a ragged 65-filter batch (one wave and a
tail of one).

Inside the envelope of positive definiteness (ratio_util.ENVELOPE: fp32 1e4, fp64 1e8, from the host build): the bound, exact symmetry,
positive definiteness (fp64 eigvalsh on the host) and health() flagging nobody.  Beyond it (fp32 at 1e6 and 1e8) only what can be
known: every word finite, the state within the state tolerance, and health()'s not-positive-definite bit equal to the sign of the
smallest eigenvalue of the GPU's own correlation-normalised P_hat wherever that is 1e-3 away from zero (at most a quarter of a decade's
cases may be closer).  Families agree to the bits where they run the same kernel: compared in the order the families run in one
session (the first family's result is kept), so a run of a single family compares nothing.
"""
import numpy as np
import pytest

import oracle
import quadrotor_landing_amd as qla
import ratio_util as ru
from quadrotor_landing_amd import health as hl
from test_gpu_innovation import TOL as INNOV_TOL, _same
from util import note

pytestmark = pytest.mark.gpu

RECORDS = [("bias1", 1, None), ("bias0-full", 0, "0"), ("bias0-compact", 0, "1")]     # (id, est_bias, QLE_COMPACT)
GRID = [(d, o, r) for d in ("f64", "f32") for o in (1, 0) for r in range(len(RECORDS))]
grid = pytest.mark.parametrize("dtype,direct,record", GRID, ids=[f"{d}-direct{o}-{RECORDS[r][0]}" for d, o, r in GRID])
UPDATE_ROUTE = {"f64": "split", "f32": "levels"}
RESIDENT_ROUTE = UPDATE_ROUTE                     # k_run_resident corrects with ekf_update_split (fp64) / ekf_update_emit (fp32)
MR_ROUTE = {"f64": "split", "f32": "packed"}      # k_step_mr: the batch form on the split covariance / the update between unpack and pack
# the per-predict tolerances of tests/test_gpu_parity.py (F64 / F32 ptol): engine predict against the oracle's fp64 prediction_step
PREDICT_PTOL = {"f64": 5e-11, "f32": 3e-6}
PREDICT_STATE = {"f64": dict(state=1e-12, quat=1e-11), "f32": dict(state=5e-7, quat=1e-6)}


def _step_routes(family, record):
    """The host routes whose constant bounds a fused tick: kw_tick serves full records only, k_step everything with QLE_QUAD=0; the
    default policy may launch either on full records."""
    if family == "lanes-only" or RECORDS[record][2] == "1":
        return ("fused",)
    return ("quad",) if family == "coop-forced" else ("fused", "quad")


CASE = np.repeat(np.arange(ru.NCASE), 5)          # filter j of the 80-filter batch is case j // 5 ...
DEC = np.tile(np.arange(5), ru.NCASE)             # ... at decade j % 5
_SEEN = {}


@pytest.fixture(autouse=True, params=["default", "lanes-only", "coop-forced"])
def kernel_family(request, monkeypatch):
    """As in test_gpu_population.py (same ids, so the keys of util.note stay family-free); QLE_QUAD is read at handle creation."""
    monkeypatch.delenv("QLE_QUAD", raising=False)
    if request.param == "lanes-only":
        monkeypatch.setenv("QLE_QUAD", "0")
    elif request.param == "coop-forced":
        monkeypatch.setenv("QLE_QUAD", "3")
    return request.param


def _handle(batch, dtype, direct, record, monkeypatch, R=None):
    _, est_bias, compact = RECORDS[record]
    if compact is None:
        monkeypatch.delenv("QLE_COMPACT", raising=False)
    else:
        monkeypatch.setenv("QLE_COMPACT", compact)
    return qla.BatchedRelativePoseEKF(batch, dtype, params=qla.make_params(**ru.params_kw(direct, est_bias, R=R)))


def _set_noise(ekf, direct, est_bias, R):
    """Per-filter parameters: the shared process noise and static biases, the tag noise R [B, 6] in words 18..23."""
    pq = qla.make_params(**ru.params_kw(direct, est_bias))
    pfp = np.zeros((ekf.batch, 24))
    pfp[:, 0:12] = np.concatenate([list(pq.Q_a), list(pq.Q_w), list(pq.Q_ab), list(pq.Q_wb)])
    pfp[:, 12:15] = ru.HW["ab_static"]; pfp[:, 15:18] = ru.HW["wb_static"]
    pfp[:, 18:24] = R
    if not est_bias:
        pfp[:, 6:12] = 0.0
    ekf.set_filter_params(pfp)
    assert _same(ekf.get_filter_params()[:, 18:24], R)


def _load(ekf, x, P):
    ekf.set_state(x, P)
    xd, Pd = ekf.get_state()
    assert _same(xd, x) and _same(Pd, P)            # float32 inputs: both dtypes hold what the truth was computed on


def _check(ekf, dtype, routes, direct, dec, truth, label, extra=0.0, predicts=0):
    """The assertions on a corrected handle: truth = dict of x_hat [B,16], P_hat [B,n,n], rho_eff [B], dec [B] the decade index.
    extra: what is allowed on top of GPU_FACTOR x C_HOST x law, predicts: how many per-predict state tolerances on top of the state
    tolerance (the predicts behind a multirate correction)."""
    xg, Pg = ekf.get_state()
    c_host = max(ru.C_HOST[r][dtype][direct] for r in routes)
    env = min(ru.ENVELOPE[r][dtype] for r in routes)
    cov = ru.cov_dev_each(Pg, truth["P_hat"])
    ratio = ru.GPU_FACTOR * cov / (ru.GPU_FACTOR * c_host * ru.law(dtype, truth["rho_eff"]) + extra)      # allowed: GPU_FACTOR
    st, qe = ru.state_dev_each(xg, truth["x_hat"]), ru.quat_err_each(xg, truth["x_hat"])
    lam = ru.corr_lam_min(Pg)
    h = ekf.health()
    not_pd, flagged = (h["status"] & hl.NOT_PD) != 0, h["status"] != 0      # every status bit is selected by default
    for k, rho in enumerate(ru.DECADES):
        s = dec == k
        if not s.any():
            continue
        print(f"{label} rho {rho:.0e}: cov_dev {cov[s].max():.2e} = {ratio[s].max():.2f} C_host law; state {st[s].max():.2e} quat {qe[s].max():.2e}; "
              f"lam_min {lam[s].min():.2e}; flagged {int(flagged[s].sum())} not_pd {int(not_pd[s].sum())}")
    assert ekf.count_nonfinite() == 0
    assert _same(Pg, Pg.transpose(0, 2, 1))
    tol = {name: v + predicts * PREDICT_STATE[dtype][name] for name, v in ru.STATE_TOL[dtype].items()}
    for k, rho in enumerate(ru.DECADES):
        s = dec == k
        if not s.any():
            continue
        note(f"state_rho{rho:.0e}", st[s].max(), tol["state"])
        note(f"quat_rho{rho:.0e}", qe[s].max(), tol["quat"])
        if rho <= env:
            note(f"cov_over_chost_law_rho{rho:.0e}", ratio[s].max(), ru.GPU_FACTOR)
            assert (lam[s] > 0).all(), (rho, lam[s].min())
            assert not flagged[s].any(), (rho, h["status"][s])
        else:
            clear = np.abs(lam[s]) >= ru.BAND
            assert (~clear).sum() * ru.NCASE <= ru.BAND_CAP * s.sum(), (rho, lam[s])
            assert np.array_equal(not_pd[s][clear], lam[s][clear] <= 0), (rho, lam[s], not_pd[s])
            assert not ((h["status"][s] & ~np.uint8(hl.NOT_PD)) != 0).any(), (rho, h["status"][s])
    return xg, Pg


def _same_across_families(key, family, arrays):
    """Bit for bit against the first family that ran this key (families that run one kernel, whatever QLE_QUAD says)."""
    first = _SEEN.setdefault(key, (family, arrays))
    for a, b in zip(first[1], arrays):
        assert _same(a, b), (key, first[0], family)


def _update_with_per_filter_noise(B, dtype, direct, record, family, monkeypatch):
    est_bias = RECORDS[record][1]
    t = ru.table(direct, est_bias)
    ci, di = CASE[:B], DEC[:B]
    ekf = _handle(B, dtype, direct, record, monkeypatch)
    _set_noise(ekf, direct, est_bias, t["R"][ci, di])
    _load(ekf, t["x"][ci], t["P"][ci])
    z = t["z"][ci]
    _, S, nis = ekf.innovation(z)
    e_S, e_nis = ru.rel(S, t["S"][ci, di]), np.abs(nis / t["nis"][ci, di] - 1)
    for k, rho in enumerate(ru.DECADES):
        print(f"innovation rho {rho:.0e}: S {ru.rel(S[di == k], t['S'][ci, di][di == k]):.2e} nis {e_nis[di == k].max():.2e}")
    note("S", e_S, INNOV_TOL[dtype]["S"]); note("nis", e_nis.max(), INNOV_TOL[dtype]["nis"])
    ekf.update(z)
    truth = dict(x_hat=t["x_hat"][ci, di], P_hat=t["P_hat"][ci, di], rho_eff=t["rho_eff"][ci, di])
    xg, Pg = _check(ekf, dtype, (UPDATE_ROUTE[dtype],), direct, di, truth, f"update {dtype} direct{direct} {RECORDS[record][0]} B={B}")
    ekf.close()
    _same_across_families(("update", B, dtype, direct, record), family, (S, nis, xg, Pg))
    return xg, Pg


@grid
def test_update_and_innovation_with_per_filter_noise(dtype, direct, record, kernel_family, monkeypatch):
    """k_innov, then k_update, on 80 filters: 16 cases x 5 decades, R through words 18..23 of set_filter_params."""
    _update_with_per_filter_noise(80, dtype, direct, record, kernel_family, monkeypatch)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_update_ragged_batch(dtype, kernel_family, monkeypatch):
    """65 filters, one wave and a tail of one: the same rows as the first 65 of the 80-filter batch, bit for bit."""
    direct, record = 0, 0
    xg, Pg = _update_with_per_filter_noise(65, dtype, direct, record, kernel_family, monkeypatch)
    x80, P80 = _update_with_per_filter_noise(80, dtype, direct, record, kernel_family, monkeypatch)
    assert _same(xg, x80[:65]) and _same(Pg, P80[:65])


def _teacher_forced(entry, dtype, direct, record, family, monkeypatch, shared):
    """One whole tick through `entry` ("step": the fused tick; "resident": k_run_resident over a one-tick sequence) against the truth
    applied to what the handle's own predict of the same inputs leaves (read back with get_state): the predict in front of the
    correction is not part of what is compared.  shared: five 16-filter handles, one per decade, the noise in the handle's parameters;
    else one 80-filter handle with per-filter noise.  -> the corrected (x, P) of every handle."""
    pytest.importorskip("mpmath", reason="the truth of a teacher-forced tick is truth_mp.correct at run time")
    est_bias = RECORDS[record][1]
    t = ru.table(direct, est_bias)
    n = t["n"]
    routes = _step_routes(family, record) if entry == "step" else (RESIDENT_ROUTE[dtype],)
    out = []
    for k in (range(5) if shared else [None]):
        ci, di = (np.arange(ru.NCASE), np.full(ru.NCASE, k)) if shared else (CASE, DEC)
        B = len(ci)
        ekf = _handle(B, dtype, direct, record, monkeypatch, R=t["R"][0, k] if shared else None)
        if not shared:
            _set_noise(ekf, direct, est_bias, t["R"][ci, di])
        u = np.tile(ru.IMU, (B, 1))
        _load(ekf, t["x"][ci], t["P"][ci])
        ekf.predict(u)
        xp, Pp = ekf.get_state()
        first = np.array([int(np.nonzero(ci == c)[0][0]) for c in ci])
        assert _same(xp, xp[first]) and _same(Pp, Pp[first])          # the tag noise is no input of a predict
        truth = dict(x_hat=np.empty((B, 16)), P_hat=np.empty((B, n, n)), rho_eff=np.empty(B))
        for j in range(B):
            tr = ru.truth_correct(direct, est_bias, xp[j], Pp[j], t["z"][ci[j]], t["R"][ci[j]])     # cached per case: all five decades
            for name in truth:
                truth[name][j] = tr[name][di[j]]
        _load(ekf, t["x"][ci], t["P"][ci])
        z = t["z"][ci]
        if entry == "step":
            ekf.step(u, z)
        else:
            seq = ekf.make_inputs(1, np.ones(1, np.uint8))
            seq.upload_tick(0, u, z, np.ones(B, np.uint8))
            ekf.run_resident(seq, 0, 1)
        out += list(_check(ekf, dtype, routes, direct, di, truth,
                           f"{entry} {'shared' if shared else 'pfp'} {dtype} direct{direct} {RECORDS[record][0]} {family}"))
        ekf.close()
    return out


@grid
def test_update_and_innovation_with_shared_noise(dtype, direct, record, kernel_family, monkeypatch):
    """k_innov<F = false>, then k_update<F = false>: one 16-filter handle per decade, the decade's noise vector as the handle's
    R_r / R_ang."""
    est_bias = RECORDS[record][1]
    t = ru.table(direct, est_bias)
    out = []
    for k in range(5):
        assert (t["R"][:, k] == t["R"][0, k]).all()
        ekf = _handle(ru.NCASE, dtype, direct, record, monkeypatch, R=t["R"][0, k])
        _load(ekf, t["x"], t["P"])
        _, S, nis = ekf.innovation(t["z"])
        e_S, e_nis = ru.rel(S, t["S"][:, k]), np.abs(nis / t["nis"][:, k] - 1).max()
        print(f"innovation shared rho {ru.DECADES[k]:.0e}: S {e_S:.2e} nis {e_nis:.2e}")
        note("S", e_S, INNOV_TOL[dtype]["S"]); note("nis", e_nis, INNOV_TOL[dtype]["nis"])
        ekf.update(t["z"])
        truth = dict(x_hat=t["x_hat"][:, k], P_hat=t["P_hat"][:, k], rho_eff=t["rho_eff"][:, k])
        out += [S, nis] + list(_check(ekf, dtype, (UPDATE_ROUTE[dtype],), direct, np.full(ru.NCASE, k), truth,
                                      f"update shared {dtype} direct{direct} {RECORDS[record][0]}"))
        ekf.close()
    _same_across_families(("update_shared", dtype, direct, record), kernel_family, out)


@pytest.mark.parametrize("shared", [False, True], ids=["pfp", "shared"])
@grid
def test_fused_step_teacher_forced(dtype, direct, record, shared, kernel_family, monkeypatch):
    """The fused tick (k_step, kw_tick) with per-filter noise on 80 filters and with shared noise on 16-filter handles."""
    out = _teacher_forced("step", dtype, direct, record, kernel_family, monkeypatch, shared)
    # the default policy runs one of the two kernels: its result is that family's, bit for bit
    seen = _SEEN.setdefault(("step", dtype, direct, record, shared), {})
    seen[kernel_family] = out
    if len(seen) == 3:
        assert any(all(_same(a, b) for a, b in zip(seen["default"], seen[f])) for f in ("lanes-only", "coop-forced"))


@pytest.mark.parametrize("shared", [False, True], ids=["pfp", "shared"])
@grid
def test_run_resident_teacher_forced(dtype, direct, record, shared, kernel_family, monkeypatch):
    """k_run_resident over a one-tick sequence with a tag pose: its own predict, then ekf_update_split (fp64) / ekf_update_emit (fp32).
    One kernel whatever QLE_QUAD says: the families agree to the bits."""
    out = _teacher_forced("resident", dtype, direct, record, kernel_family, monkeypatch, shared)
    _same_across_families(("resident", dtype, direct, record, shared), kernel_family, out)


@pytest.mark.parametrize("steps", [1, 2])
@pytest.mark.parametrize("direct", [1, 0])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_multirate_correction_at_the_history_entry(dtype, direct, steps, kernel_family, monkeypatch):
    """k_step_mr with a fixed delay of `steps` ticks, 1 the smallest a handle accepts: after set_state the history is the single entry
    "state now" (EKF.cpp:305-344); steps - 1 predict-only ticks, then a tick with a tag pose whose step delay reaches back to that
    entry (EKF.cpp:200-201: ind = hist_len - step = 0).  So the correction is applied to the fixture's own state -- the truth of the
    fixture, no predict in front -- and replayed forward: steps - 1 stored IMU samples, then the current tick's predict
    (EKF.cpp:222-226, 249).  steps = 1 is the clamped anchor start without a replay, steps = 2 replays one tick.  fp32 runs the
    sequential update between cov_unpack and cov_pack ("packed"), fp64 the batch form on the split covariance ("split").
    Expected: the oracle's fp64 prediction_step applied `steps` times to the truth's (x_hat, P_hat).  Allowed on top of
    GPU_FACTOR x C_HOST x law: the per-predict tolerance of tests/test_gpu_parity.py for each of those predicts (engine predict
    against the oracle's), which dominates at rho = 1 in fp64 and is nothing against the law from rho = 1e4 on."""
    est_bias, record = 1, 0
    t = ru.table(direct, est_bias)
    dT = 1.0 / 400.0
    kw = dict(ru.params_kw(direct, est_bias), multirate_ekf=1, dynamic_meas_delay=0, measurement_delay=steps * dT,
              limit_measurement_freq=0, corner_margin_enbl=0)
    monkeypatch.delenv("QLE_COMPACT", raising=False)
    ekf = qla.BatchedRelativePoseEKF(80, dtype, params=qla.make_params(**kw))
    assert int(ekf.derived.measurement_step_delay) == steps
    _set_noise(ekf, direct, est_bias, t["R"][CASE, DEC])
    ekf.enable_gating(True)
    _load(ekf, t["x"][CASE], t["P"][CASE])
    u = np.tile(ru.IMU, (80, 1))
    for _ in range(steps - 1):
        ekf.filter_update(u)
    ekf.filter_update(u, t["z"][CASE], np.ones(80, np.uint8))
    perf, _, _ = ekf.tick_flags()
    assert perf.all()
    po = oracle.make_params(**kw)
    truth = dict(x_hat=np.empty((80, 16)), P_hat=np.empty((80, 15, 15)), rho_eff=t["rho_eff"][CASE, DEC])
    for j in range(80):
        x, P = t["x_hat"][CASE[j], DEC[j]], t["P_hat"][CASE[j], DEC[j]]
        for _ in range(steps):
            x, P, _ = oracle.prediction_step(po, x, P, ru.IMU)
        truth["x_hat"][j], truth["P_hat"][j] = x, P
    xg, Pg = _check(ekf, dtype, (MR_ROUTE[dtype],), direct, DEC, truth, f"multirate steps={steps} {dtype} direct{direct} {kernel_family}",
                    extra=steps * PREDICT_PTOL[dtype], predicts=steps)
    ekf.close()
    _same_across_families(("multirate", dtype, direct, steps), kernel_family, (xg, Pg))
