"""The multirate history (k_step_mr, ekf_multirate.hpp) held to the oracle at every place a chain can restart from, by schedule.

Each run steps the engine and one oracle.Filter per filter through a schedule of tests/mr_schedule_util.py -- two full waves and a
ragged one; filters seeded late, masked on alternate frames, never seeded, or with frames of their own; frames on a jittered cadence so
that the extra checkpoint is hit exactly, missed by a tick or two, or bypassed; checkpoint spacings 4 / 8 / 32 (QLE_MR_K), so that a
160-tick run wraps the IMU ring many times and fp32 stays comparable tick by tick -- and on EVERY tick asserts
  * tick_flags against the oracle's performed_correction / upds_since_correction,
  * hist_first, e_tick, e_want (qle_get_history_info) against the index model, which ties the census of
    tests/test_multirate_schedule_cpu.py to what the device did,
  * state and covariance of every seeded filter against its oracle filter; unseeded filters stay all-zero records.

Tolerances.  fp64: those of test_gpu_parity.py::test_multirate_replay_matches_reference_logic (1e-10 / 1e-12 / 1e-10).  fp32: 10 x the
largest deviation from the oracle that these runs measured on an MI355X, per kind (tests/tolerances_multirate.md lists measured,
stated and ratio)."""
import numpy as np
import pytest

import mr_schedule_util as ms
import oracle
import quadrotor_landing_amd as qla
from util import assert_state_close, meas_near

pytestmark = pytest.mark.gpu

F32_STATE, F32_QUAT, F32_COV = 3.8e-5, 1.7e-6, 7.4e-5    # measured 3.79e-6 / 1.65e-7 / 7.38e-6 (tests/tolerances_multirate.md)


def _run(monkeypatch, dtype, k, mode, rebase):
    sched = ms.Schedule(k, mode, rebase=rebase)
    monkeypatch.setenv("QLE_MR_K", str(k))
    if rebase:
        monkeypatch.setenv("QLE_TICK_REBASE", str(sched.rebase_at))
    else:
        monkeypatch.delenv("QLE_TICK_REBASE", raising=False)
    po = oracle.make_params(**sched.kw)
    ekf = qla.BatchedRelativePoseEKF(sched.B, dtype, params=qla.make_params(**sched.kw))
    info = ekf.history_info()
    assert (info["k"], info["Nc"], info["Cu"]) == (k, sched.Nc, sched.Cu)
    n_perf = [0]

    def after_tick(t, c):
        m, filt, seeded = c["model"], c["filt"], c["seeded"]
        perf, cons, upds = ekf.tick_flags()
        np.testing.assert_array_equal(perf.astype(bool), c["perf"], err_msg=f"tick {t}")
        np.testing.assert_array_equal(upds, np.array([f.f.upds_since_correction for f in filt], np.int32), err_msg=f"tick {t}")
        np.testing.assert_array_equal(cons.astype(bool), c["mask"] & seeded, err_msg=f"tick {t}")    # no rate limit: a pose is consumed at once
        hi = ekf.history_info()
        assert (hi["tick"], hi["e_tick"], hi["e_want"]) == (m.tick, m.e_tick, m.e_want), (t, hi, m.tick, m.e_tick, m.e_want)
        np.testing.assert_array_equal(hi["hist_first"], m.first, err_msg=f"tick {t}")
        if mode == "stamps":
            assert hi["e_tick"] == -1 and hi["e_want"] == -1
            if c["perf"].any():
                d = ekf.measurement_delay()
                ref = np.array([f.f.measurement_delay_curr for f in filt])
                np.testing.assert_allclose(d[c["perf"]], ref[c["perf"]], atol=1e-12)
        n_perf[0] += int(c["perf"].sum())
        xg, Pg = ekf.get_state()
        assert np.all(xg[~seeded] == 0) and np.all(Pg[~seeded] == 0), t          # never touched
        if seeded.any():
            if dtype == "f64":
                assert_state_close(xg[seeded], Pg[seeded], c["xr"][seeded], c["Pr"][seeded], 1e-10, 1e-12, 1e-10)
            else:
                assert_state_close(xg[seeded], Pg[seeded], c["xr"][seeded], c["Pr"][seeded], F32_STATE, F32_STATE, F32_QUAT, ptol=F32_COV)

    m = ms.run_schedule(sched, oracle, po, meas_near, dtype=dtype, ekf=ekf, after_tick=after_tick)
    assert ekf.count_nonfinite() == 0
    ekf.close()
    # what this very run reached (its corrections are the oracle's for these inputs): the same conditions as the CPU census
    assert not ms.census_ok(sched, m.counts), (ms.census_ok(sched, m.counts), m.counts)
    assert n_perf[0] > 10 * sched.B


@pytest.mark.parametrize("mode", ms.MODES)
@pytest.mark.parametrize("k", ms.KS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_every_replay_start_matches_the_oracle(dtype, k, mode, monkeypatch):
    _run(monkeypatch, dtype, k, mode, rebase=False)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_replay_starts_across_tick_origin_shifts(dtype, monkeypatch):
    """QLE_TICK_REBASE at four IMU rings, k = 4: the origin moves every two rings, between arming and filling the extra slot and
    between filling and using it (classes La / Lu of the census)."""
    _run(monkeypatch, dtype, 4, "fixed", rebase=True)


def test_checkpoint_spacing_override_takes_the_measured_values_only(monkeypatch):
    kw = ms.params_kw("fixed")
    for env, want in ((None, 32), ("16", 16), ("64", 64), ("5", 32), ("0", 32), ("abc", 32)):
        if env is None:
            monkeypatch.delenv("QLE_MR_K", raising=False)
        else:
            monkeypatch.setenv("QLE_MR_K", env)
        ekf = qla.BatchedRelativePoseEKF(70, "f32", params=qla.make_params(**kw))
        hi = ekf.history_info()
        assert hi["k"] == want and (hi["Nc"], hi["Cu"]) == ms.history_sizes(3, want)
        assert (hi["tick"], hi["e_tick"], hi["e_want"]) == (0, -1, -1) and hi["hist_first"].shape == (70,)
        ekf.close()
    single = qla.BatchedRelativePoseEKF(70, "f32", params=qla.make_params(**dict(kw, multirate_ekf=0)))
    with pytest.raises(qla.QleError):
        single.history_info()
    single.close()
