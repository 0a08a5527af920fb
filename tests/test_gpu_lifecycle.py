"""Filter lifecycle from GPU memory on the GPU (DeviceIO.seed / health / retire / reseed; libqle_health.so: k_health, k_health_reduce,
k_retire, k_and_masks; qle_initialize_state_slot of the tick library).

No tolerance appears: every comparison is exact equality of bits against the host path (initialize_state_masked, get_state) or exact
equality of status bytes and counts against the numpy restatement of health_util.py.  Batches: 1, 63, 64, 65, 130 (one lane, a tile
boundary on each side, a partial last tile); the reduce test adds 16 449 (more tiles than the reduce workgroup has lanes, and a
partial tile).
"""
import numpy as np
import pytest

import health_util as hu
import quadrotor_landing_amd as qla
from quadrotor_landing_amd import health
from test_gpu_devio import KW, assert_same_bits, dev, rand_imu, rand_pose

pytestmark = pytest.mark.gpu

BATCHES = [1, 63, 64, 65, 130]
MR = dict(multirate_ekf=1, measurement_delay=3 / 400.0)   # measurement_step_delay = 3 ticks
RECORDS = {"full15": (15, "0"), "full9": (9, "0"), "compact9": (9, "1")}


def _torch():
    import torch as t
    return t


@pytest.fixture(autouse=True)
def torch_first():
    """torch is imported before the first handle of a test exists: a torch that is first imported after the engine has initialised the
    HIP runtime reports no GPU."""
    return _torch()


def host(*ts):
    _torch().cuda.synchronize()
    return tuple(x.cpu().numpy() for x in ts)


def same_state(a, b, what, rows=None):
    """get_state() and state_initialized() of two handles, bit for bit (on `rows` only when given)"""
    (xa, Pa), (xb, Pb) = a.get_state(), b.get_state()
    ia, ib = a.state_initialized(), b.state_initialized()
    sel = slice(None) if rows is None else rows
    assert_same_bits(xa[sel], xb[sel], f"{what}: x")
    assert_same_bits(Pa[sel], Pb[sel], f"{what}: P")
    assert_same_bits(ia[sel], ib[sel], f"{what}: state_initialized")


def same_flags(a, b, what, rows=None):
    sel = slice(None) if rows is None else rows
    for fa, fb, name in zip(a.tick_flags(), b.tick_flags(), ("performed_correction", "consumed", "upds_since_correction")):
        assert_same_bits(fa[sel], fb[sel], f"{what}: {name}")


def prior_state(rng, B, n):
    """A state in which every other filter holds none (zero rows) and the others carry biases a reinit must clear."""
    x = np.zeros((B, 16)); P = np.zeros((B, n, n))
    has = np.arange(B) % 2 == 1
    x[has, 0:6] = rng.normal(size=(int(has.sum()), 6))
    x[has, 6:10] = rand_pose(rng, int(has.sum()))[:, 3:]
    x[has, 10:16] = 0.05 * rng.normal(size=(int(has.sum()), 6))
    A = 0.1 * rng.normal(size=(B, n, n))
    P[has] = (A @ A.transpose(0, 2, 1) + 0.01 * np.eye(n))[has]
    return x, P


def run_ticks(rng, handles, B, plan, src="float32"):
    """The same ticks on every handle through DeviceIO.tick; plan: per tick whether it carries tag poses."""
    for has_tag in plan:
        u = dev(rand_imu(rng, B).astype(src))
        z = dev(rand_pose(rng, B).astype(src)) if has_tag else None
        m = dev((rng.uniform(size=B) < 0.8).astype(np.uint8)) if has_tag else None
        for io in handles:
            io.tick(u, z, m)


# ------------------------------------------------------------------------------------------------ 1. seed parity
@pytest.mark.parametrize("multirate", [0, 1], ids=["single-rate", "multirate"])
@pytest.mark.parametrize("est_bias", [1, 0], ids=["bias", "no-bias"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_seed_from_tensors_equals_initialize_state_masked(dtype, est_bias, multirate):
    kw = dict(KW, est_bias=est_bias, limit_measurement_freq=1, **(MR if multirate else {}))
    n = 15 if est_bias else 9
    for B in BATCHES:
        for src, reinit in (("float32", False), ("float64", True), ("float32", True)):
            rng = np.random.default_rng(1000 * B + 10 * multirate + est_bias + (src == "float64"))
            x0, P0 = prior_state(rng, B, n)
            z = rand_pose(rng, B).astype(src)
            mask = (rng.uniform(size=B) < 0.67).astype(np.uint8)   # about a third masked out
            mask[0] = 1
            a, b = (qla.BatchedRelativePoseEKF(B, dtype, **kw) for _ in range(2))
            for e in (a, b):
                e.set_state(x0, P0)
                e.enable_gating(True)
            ia, ib = qla.DeviceIO(a), qla.DeviceIO(b)
            ia.seed(dev(z), dev(mask), reinit_bias=reinit)
            b.initialize_state(z.astype(np.float64), reinit_bias=reinit, mask=mask)
            what = f"{dtype} B={B} {src} reinit={reinit}"
            same_state(a, b, f"seed {what}")
            xs, _ = a.get_state()
            seeded = mask != 0
            assert np.array_equal(a.state_initialized() != 0, seeded | (np.arange(B) % 2 == 1))
            if est_bias and B > 1:
                kept = seeded & (np.arange(B) % 2 == 1)
                assert (xs[kept, 10:16] != 0).all() != reinit and (xs[seeded & ~kept, 10:16] == 0).all()
            # five ticks, tag poses on the second (history one entry deep < measurement_step_delay = 3) and the fifth (four deep)
            run_ticks(rng, (ia, ib), B, (0, 1, 0, 0, 1))
            same_state(a, b, f"ticks {what}")
            same_flags(a, b, f"ticks {what}")
            xt, _ = a.get_state()
            assert np.abs(xt[seeded] - xs[seeded]).max() > 0    # the ticks did something
            for o in (ia, ib, a, b):
                o.close()


# ------------------------------------------------------------------------------------------------ 2. a handle never seeded from the host
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_seed_on_a_never_seeded_handle_then_a_disjoint_seed(dtype):
    B = 130
    rng = np.random.default_rng(2)
    ekf = qla.BatchedRelativePoseEKF(B, dtype, **KW)
    io = qla.DeviceIO(ekf)
    with pytest.raises(qla.QleError) as e:
        io.tick(dev(rand_imu(rng, B).astype(np.float32)))
    assert e.value.code == qla._lib.QLE_ERR_STATE
    m1 = (np.arange(B) % 3 == 0).astype(np.uint8); m2 = (np.arange(B) % 3 == 1).astype(np.uint8)
    io.seed(dev(rand_pose(rng, B).astype(np.float32)), dev(m1))
    io.tick(dev(rand_imu(rng, B).astype(np.float32)))           # no QLE_ERR_STATE
    assert np.array_equal(ekf.state_initialized(), m1)
    x1, P1 = ekf.get_state()
    assert not x1[m1 == 0].any() and not P1[m1 == 0].any()
    io.seed(dev(rand_pose(rng, B)), dev(m2.astype(bool)))        # float64 poses, a bool mask
    x2, P2 = ekf.get_state()
    assert np.array_equal(ekf.state_initialized(), m1 | m2)
    keep = m2 == 0
    assert_same_bits(x2[keep], x1[keep], "x of the filters outside the second mask")
    assert_same_bits(P2[keep], P1[keep], "P of the filters outside the second mask")
    assert (x2[m2 != 0, 9] != 0).any() and not x2[(m1 | m2) == 0].any()
    io.close(); ekf.close()


# ------------------------------------------------------------------------------------------------ 3. health against numpy
def case_handle(dtype, record, B, monkeypatch, seed=11):
    """A handle whose filters are the case list of health_util tiled over the batch in a fixed random order."""
    n, compact = RECORDS[record]
    monkeypatch.setenv("QLE_COMPACT", compact)   # read at handle creation, as tests/test_gpu_compact.py sets it
    monkeypatch.setenv("QLE_QUAD", "0")
    ekf = qla.BatchedRelativePoseEKF(B, dtype, **dict(KW, est_bias=int(n == 15)))
    assert ekf.num_states == n and ekf.policy()["record_words"] == (64 if compact == "1" else 136)
    xc, Pc = hu.case_list(dtype, n)
    order = np.random.default_rng(seed + B).permutation(B) % len(xc)
    ekf.set_state(xc[order], Pc[order])
    return ekf, order


@pytest.mark.parametrize("record", list(RECORDS))
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_health_equals_the_numpy_classification(dtype, record, monkeypatch):
    for B in BATCHES:
        ekf, order = case_handle(dtype, record, B, monkeypatch)
        io = qla.DeviceIO(ekf)
        x, P = ekf.get_state()
        ref, margin = hu.classify(x, P, **hu.LIMITS)
        assert margin >= 0.5
        want = dict(healthy=0, nan_in_x=1, inf_in_P=1, indefinite=2, q_scaled=4, at_limit=0, above_limit=8, no_state=0)
        assert all(ref[i] == want[hu.CASE_NAMES[c]] for i, c in enumerate(order))      # the device holds the cases as built
        sel = hu.NONFINITE | hu.NOT_PD | hu.SIGMA_R
        status, flagged, summ = host(*io.health(select=sel, return_summary=True, **hu.LIMITS))
        print(f"{dtype} {record} B={B}: status counts {np.bincount(status, minlength=9)[:9]}, summary {summ}")
        assert status.dtype == np.uint8 and flagged.dtype == np.uint8
        assert np.array_equal(status, ref), (B, list(status), list(ref))
        assert np.array_equal(flagged, ((ref & sel) != 0).astype(np.uint8))
        assert np.array_equal(summ, hu.summary_of(ref, sel, x))
        x1, P1 = ekf.get_state()
        assert_same_bits(x1, x, "x after health"); assert_same_bits(P1, P, "P after health")   # nothing was written
        assert ekf.count_nonfinite() == summ[3] == (ref == hu.NONFINITE).sum()
        # a mask: the filters left out enter no field
        mask = (np.arange(B) % 4 != 1).astype(np.uint8)
        refm, _ = hu.classify(x, P, mask=mask, **hu.LIMITS)
        st_m, fl_m, su_m = host(*io.health(mask=dev(mask), return_summary=True, **hu.LIMITS))
        assert np.array_equal(st_m, refm) and np.array_equal(fl_m, (refm != 0).astype(np.uint8))
        assert np.array_equal(su_m, hu.summary_of(refm, 63, x, mask))
        # the host-array entry gives the same
        h = ekf.health(select=sel, **hu.LIMITS)
        assert np.array_equal(h["status"], ref) and [h[k] for k in health.SUMMARY_FIELDS] == list(summ)
        # NOT_PD is the rule of k_nees with every block of the handle selected
        xt = dev(np.where(np.isfinite(x), x, 0.0))
        nees, nsum = host(*io.nees(xt, blocks="all"))
        factored = (ref != hu.NONFINITE) & x[:, 6:10].any(axis=1)
        assert np.array_equal(np.isnan(nees.astype(np.float64))[factored], (ref[factored] & hu.NOT_PD) != 0)
        if not (ref == hu.NONFINITE).any():
            assert nsum[4] == summ[4]
        io.close(); ekf.close()


# ------------------------------------------------------------------------------------------------ 4. the batch summary
def test_summary_determinism_additivity_and_launch_counts(monkeypatch):
    B = 16449                                                   # 258 tiles: more than the 256 lanes of the reduce, the last one partial
    ekf, order = case_handle("f32", "full15", B, monkeypatch)
    io = qla.DeviceIO(ekf)
    x, P = ekf.get_state()
    H = health.health_lib()
    io.health(return_summary=True, **hu.LIMITS)                 # the partials buffer exists now
    n0 = H.qhl_launch_count()
    st1, fl1, s1 = io.health(return_summary=True, **hu.LIMITS)
    assert H.qhl_launch_count() - n0 == 2
    st2, fl2, s2 = io.health(return_summary=True, **hu.LIMITS)
    assert H.qhl_launch_count() - n0 == 4
    io.health(**hu.LIMITS)
    assert H.qhl_launch_count() - n0 == 5
    st1, fl1, s1, st2, fl2, s2 = host(st1, fl1, s1, st2, fl2, s2)
    assert_same_bits(s1, s2, "two summaries of one state")
    assert np.array_equal(st1, st2) and np.array_equal(fl1, fl2)
    counts = np.bincount(order, minlength=8)
    print(f"summary at B={B}: {s1}")
    assert np.array_equal(s1, hu.summary_of(st1, 63, x)) and s1[0] == B - counts[7] and s1[2] == counts[7]
    assert s1[3] == counts[1] + counts[2] and s1[4] == counts[3] and s1[5] == counts[4] and s1[6] == counts[6]
    tot = np.zeros(9)
    for lo, hi in ((0, 5000), (5000, 5001), (5001, B)):
        e = qla.BatchedRelativePoseEKF(hi - lo, "f32", **dict(KW, est_bias=1))
        e.set_state(x[lo:hi], P[lo:hi])
        o = qla.DeviceIO(e)
        st, _, s = host(*o.health(return_summary=True, **hu.LIMITS))
        assert np.array_equal(st, st1[lo:hi])
        tot += s
        o.close(); e.close()
    assert np.array_equal(tot, s1), (tot, s1)
    io.close(); ekf.close()


# ------------------------------------------------------------------------------------------------ 5. retire
@pytest.mark.parametrize("multirate", [0, 1], ids=["single-rate", "multirate"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_retired_filters_stay_out_and_their_neighbours_do_not_notice(dtype, multirate):
    B = 130
    rng = np.random.default_rng(50 + multirate)
    kw = dict(KW, limit_measurement_freq=1, **(MR if multirate else {}))
    a, twin = (qla.BatchedRelativePoseEKF(B, dtype, **kw) for _ in range(2))
    for e in (a, twin):
        e.enable_gating(True)
    ia, it = qla.DeviceIO(a), qla.DeviceIO(twin)
    gone = (rng.uniform(size=B) < 0.3).astype(np.uint8); gone[[0, 63, 64, 129]] = 1
    keep = gone == 0
    z0 = dev(rand_pose(rng, B).astype(np.float32))
    ia.seed(z0)                                                # every filter, then the subset is retired
    ia.retire(dev(gone))
    it.seed(z0, dev(keep.astype(np.uint8)))                    # the twin never had them
    same_state(a, twin, "after retire")                        # a retired record is a record that never had a state
    slots = a.policy()["ring_slots"]
    plan = [int(k % 3 == 1) for k in range(slots + 2)]         # more ticks than the ring has slots, tag ticks among them
    assert sum(plan) >= 1
    run_ticks(rng, (ia, it), B, plan)
    x, P = a.get_state()
    assert not x[~keep].any() and not P[~keep].any() and not a.state_initialized()[~keep].any()
    assert np.array_equal(a.state_initialized()[keep], np.ones(int(keep.sum()), np.uint8))
    same_state(a, twin, f"{len(plan)} ticks after retire")
    same_flags(a, twin, "ticks after retire", rows=keep)
    # a later seed of a retired filter is the seed of a fresh one
    z1 = dev(rand_pose(rng, B))
    back = gone.copy(); back[0] = 0
    ia.seed(z1, dev(back)); it.seed(z1, dev(back))
    same_state(a, twin, "seed of retired filters")
    assert np.array_equal(a.state_initialized(), (keep | (back != 0)).astype(np.uint8))
    run_ticks(rng, (ia, it), B, (0, 1, 0, 0, 1))
    same_state(a, twin, "ticks after the second seed")
    same_flags(a, twin, "ticks after the second seed", rows=(keep | (back != 0)))
    assert a.count_nonfinite() == 0
    for o in (ia, it, a, twin):
        o.close()


# ------------------------------------------------------------------------------------------------ 6. reseed closes the loop
@pytest.mark.parametrize("multirate", [0, 1], ids=["single-rate", "multirate"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_reseed_seeds_exactly_the_flagged_filters_with_a_detection(dtype, multirate):
    B = 130
    rng = np.random.default_rng(60 + multirate)
    kw = dict(KW, **(MR if multirate else {}))
    a, b = (qla.BatchedRelativePoseEKF(B, dtype, **kw) for _ in range(2))
    ia = qla.DeviceIO(a)
    z0 = rand_pose(rng, B)
    a.initialize_state(z0)
    x, P = a.get_state()
    nan_rows = np.arange(B) % 7 == 2; bad_P = np.arange(B) % 7 == 5
    x[nan_rows, 11] = np.nan                                    # a NaN bias: what a reseed that kept the biases would not cure
    P[bad_P, 4, 4] = -1.0
    a.set_state(x, P); b.set_state(x, P)
    x, P = a.get_state()
    bad = nan_rows | bad_P
    seen = (rng.uniform(size=B) < 0.6).astype(np.uint8)         # detections: part of the bad filters, and healthy ones too
    assert (seen[bad] == 1).any() and (seen[bad] == 0).any() and (seen[~bad] == 1).any()
    z = rand_pose(rng, B).astype(np.float32)
    status, reseeded = host(*ia.reseed(dev(z), dev(seen)))
    assert np.array_equal(status != 0, bad) and np.array_equal(status[nan_rows], np.full(int(nan_rows.sum()), hu.NONFINITE, np.uint8))
    assert np.array_equal(status[bad_P], np.full(int(bad_P.sum()), hu.NOT_PD, np.uint8))
    assert np.array_equal(reseeded != 0, bad & (seen != 0))     # exactly flagged AND seen
    b.initialize_state(z.astype(np.float64), reinit_bias=True, mask=reseeded)
    same_state(a, b, "reseed against initialize_state_masked on the same set")
    x1, P1 = a.get_state()
    untouched = reseeded == 0
    assert_same_bits(x1[untouched], x[untouched], "x of the filters not reseeded")
    assert_same_bits(P1[untouched], P[untouched], "P of the filters not reseeded")
    st2, fl2 = host(*ia.health())
    assert np.array_equal(fl2 != 0, bad & (seen == 0))          # bad filters without a detection: unchanged, still flagged
    ia.retire(dev(fl2))
    assert a.count_nonfinite() == 0
    assert np.array_equal(a.state_initialized() != 0, ~(bad & (seen == 0)))
    st3, fl3, s3 = host(*ia.health(return_summary=True))
    assert not st3.any() and s3[0] == B - fl2.sum() and s3[2] == fl2.sum() and s3[1] == 0
    for o in (ia, a, b):
        o.close()


# ------------------------------------------------------------------------------------------------ 7. no synchronisation
def test_lifecycle_calls_are_ordered_by_streams_not_by_synchronisation():
    """The check of tests/test_gpu_devio.py for tick: inputs produced by a torch op on a non-default stream right before each call,
    outputs consumed by a torch op on that stream right after, no synchronisation in between -- one pass equals the synchronised run."""
    t = _torch()
    B, rounds = 65536, 12
    rng = np.random.default_rng(70)
    z0 = dev(rand_pose(rng, B).astype(np.float32)); zs = [dev(rand_pose(rng, B).astype(np.float32)) for _ in range(3)]
    us = [dev(rand_imu(rng, B).astype(np.float32)) for _ in range(3)]
    pick = [dev((rng.uniform(size=B) < 0.2).astype(np.uint8)) for _ in range(3)]
    res = []
    for sync in (False, True):
        ekf = qla.BatchedRelativePoseEKF(B, "f32", **KW)
        io = qla.DeviceIO(ekf)
        s = t.cuda.Stream(device=0)
        t.cuda.synchronize()
        with t.cuda.stream(s):
            acc = t.zeros(3, dtype=t.float64, device="cuda:0")
            io.seed(z0 + 0.0)
            for k in range(rounds):
                j = k % 3
                io.tick(us[j] * (1.0 + 1e-3 * k), zs[j] + 0.0)
                gone = pick[j] & pick[(j + 1) % 3]               # produced on s right before the call
                io.retire(gone)
                status, flagged, summ = io.health(sigma_r_max=0.25, return_summary=True)
                acc += t.stack([status.sum(dtype=t.float64), flagged.sum(dtype=t.float64), summ.sum()])   # consumed on s right after
                st, re_ = io.reseed(zs[(j + 1) % 3] * 1.0, pick[j] | flagged, sigma_r_max=0.25)
                acc += t.stack([st.sum(dtype=t.float64), re_.sum(dtype=t.float64), t.zeros((), dtype=t.float64, device="cuda:0")])
                io.seed(zs[(j + 2) % 3] + 0.0, gone)
                del gone, status, flagged, summ, st, re_
                if sync:
                    s.synchronize(); ekf.synchronize()
            xf, Pf = io.state()
        s.synchronize()
        res.append((acc.cpu().numpy(), xf.cpu().numpy(), Pf.cpu().numpy()))
        io.close(); ekf.close()
    assert np.isfinite(res[0][0]).all() and res[0][0][1] > 0 and res[0][0][0] > 0
    for a, b, what in zip(res[0], res[1], ("reduction", "x", "P")):
        assert_same_bits(a, b, what)


# ------------------------------------------------------------------------------------------------ 8. destroy frees what the handle owns
def test_create_use_close_cycles_return_their_device_memory():
    """One fp64 handle of 16 384 filters that owns every kind of device buffer a handle can own (state, multirate history, gating
    arrays, side outputs, per-filter parameters, innovation records, an 8-tick sequence with its generated truth), created, used and
    closed 25 times, the history replaced once per cycle by parameters that change its checkpoint count.

    F = the device memory the first create takes.  After the 24 further cycles, free memory must be within F / 2 of what it was
    after the first close: a condition, not a measurement -- one batch-sized buffer class of at least F / 48 leaked per cycle exceeds
    it.  It assumes that freed device memory returns to the device at once."""
    t = _torch()
    B = 16384
    kw = dict(KW, multirate_ekf=1, dynamic_meas_delay=1, measurement_delay_max=0.2)
    t.cuda.synchronize()
    free = lambda: t.cuda.mem_get_info(0)[0]

    def cycle(after_create=None):
        ekf = qla.BatchedRelativePoseEKF(B, "f64", **kw)
        if after_create is not None:
            after_create.append(free())
        rng = np.random.default_rng(80)
        ekf.enable_gating(True); ekf.enable_aux(True)
        seq = ekf.make_inputs(8, [0, 0, 0, 1, 0, 0, 0, 1])
        ekf.synth_generate(seq, seed=0xE4F00005)
        ekf.set_filter_params(np.tile(np.concatenate([list(ekf.derived.Q), KW["ab_static"], KW["wb_static"], list(ekf.derived.R)]), (B, 1)))
        ekf.innovation(rand_pose(rng, B))
        ekf.run(seq, 0, 8)
        slots = ekf.policy()["ring_slots"]
        ekf.initialize_params(measurement_delay_max=0.4)        # another checkpoint count: the six history buffers are replaced
        assert ekf.policy()["ring_slots"] != slots
        ekf.run(seq, 0, 8)
        assert ekf.count_nonfinite() == 0
        seq.close(); ekf.close()

    before = free()
    created = []
    cycle(created)
    F = before - created[0]
    first_close = free()
    for _ in range(24):
        cycle()
    end = free()
    print(f"leak check: F = {F / 2**20:.1f} MiB; free before {before / 2**20:.1f}, after the first close {first_close / 2**20:.1f}, "
          f"after 24 more cycles {end / 2**20:.1f} MiB")
    assert F > 0
    assert abs(first_close - end) <= F / 2, (F, before, first_close, end)
