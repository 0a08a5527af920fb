"""CPU tests of the multirate history schedules (tests/mr_schedule_util.py): the model's start choice against a literal reading
of the history's description, and the census -- every committed schedule, run through the oracle's filter objects alone, must reach
every start class the GPU test (tests/test_gpu_multirate_history.py) is there to hold.  The counts are conditions: a schedule, seed
or checkpoint spacing that stops reaching a class fails here, on the CPU, instead of silently thinning what the GPU test covers."""
import numpy as np
import pytest

import mr_schedule_util as ms
import oracle
from util import meas_near


def test_start_choice_matches_a_literal_reading_of_the_history():
    rng = np.random.default_rng(5)
    kinds = {"anchor": 0, "grid": 0, "extra": 0}
    for _ in range(600):
        k = int(rng.choice([4, 8, 16, 32, 64]))
        tick = int(rng.integers(1, 400))
        first = tick - 1 - int(rng.integers(0, 90))            # may be negative: a history that starts before the (shifted) origin
        step = int(rng.integers(1, 36))
        mt = first + max(tick - first - step, 0)
        e_tick = int(rng.choice([ms.NEVER, mt, mt - 1, mt - 2, mt + 1, first, first + 1, int(rng.integers(first - 5, tick))]))
        got = ms.choose_start(first, tick, step, k, e_tick)
        assert got == ms.choose_start_bruteforce(first, tick, step, k, e_tick), (first, tick, step, k, e_tick)
        assert first <= got[1] <= got[0] <= tick - 1
        assert got[2] == "anchor" or (got[1] > first and got[0] - got[1] < k)      # at most k-1 predictions from a checkpoint
        kinds[got[2]] += 1
    assert min(kinds.values()) >= 50, kinds


def test_history_sizes_hold_the_longest_replay():
    for k in (4, 8, 16, 32, 64):
        for step_max in (1, 3, 5, 20, 35):
            Nc, Cu = ms.history_sizes(step_max, k)
            assert Cu == k * Nc and Cu >= step_max + k + 1


@pytest.mark.parametrize("k,mode,rebase", ms.RUNS, ids=[f"k{k}-{m}{'-rebase' if r else ''}" for k, m, r in ms.RUNS])
def test_census_every_schedule_reaches_every_class(k, mode, rebase):
    sched = ms.Schedule(k, mode, rebase=rebase)
    po = oracle.make_params(**sched.kw)
    assert po.measurement_step_delay == 3 and (sched.Nc, sched.Cu) == ms.history_sizes(sched.step_max, k)
    assert sched.T <= ms.T_MAX and sched.B == 165
    gaps = np.diff(sched.frame_ticks)
    assert gaps.min() > 1 and gaps.max() + sched.step_max < sched.Cu      # the host arms the extra slot only for such cadences
    n_corr = [0]

    def after_tick(t, c):
        m = c["model"]
        # the model's history start against the oracle's own history length: entries first .. t
        for i in np.nonzero(c["seeded"])[0]:
            assert c["filt"][i].f.hist_len == t + 1 - (int(m.first[i]) + m.origin), (t, i)
        n_corr[0] += int(c["perf"].sum())
        if mode == "stamps":
            assert m.e_tick == -1 and m.e_want == -1

    m = ms.run_schedule(sched, oracle, po, meas_near, after_tick=after_tick)
    print(f"census k={k} {mode}{' rebase' if rebase else ''}: {m.counts}, {n_corr[0]} corrections, {len(sched.frame_ticks)} frames, "
          f"{sched.T} ticks, ring wraps {(sched.T - 1) // sched.Cu}")
    assert not ms.census_ok(sched, m.counts), (ms.census_ok(sched, m.counts), m.counts)
    if rebase:
        assert m.origin >= 3 * (sched.rebase_at // 2)          # the origin moved several times
    # wave 1's never-seeded filters stayed out, the late ones came in on their own frames
    assert not m.seeded[sched.never].any() and m.seeded[sched.late].all()
