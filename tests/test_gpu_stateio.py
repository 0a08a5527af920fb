"""Device state I/O on the GPU (DeviceIO.set_state / snapshot / restore / gather / fork, stateio.Snapshot,
BatchedRelativePoseEKF.gather_state; libqle_stateio.so: k_si_pack, k_si_copy; qle_mark_state_written of the tick library).

B = 200 (three full tiles and a ragged tile of 8) and B = 70 (one tile and 6), fp32 and fp64, 15 states, 9 states with full and with
compact records, and 15 states with per-filter parameters.  Every comparison is bit for bit -- the feature moves and rounds words and computes nothing
else: against the host `set_state` of the same values on a twin handle, against numpy fancy indexing of `get_state`, and, for what
must not move, against every word of the record array read back through the device view (stateio_util.raw_read).
"""
import ctypes as C

import numpy as np
import pytest

import lookahead_util as lu
import quadrotor_landing_amd as qla
import stateio_util as su
from quadrotor_landing_amd import _lib, stateio
from test_gpu_devio import assert_same_bits, dev, rand_imu, rand_pose

pytestmark = pytest.mark.gpu

MR = dict(multirate_ekf=1, measurement_delay=3 / 400.0)
# handle kinds: name -> (num_states, compact records, per-filter parameters)
KINDS = {"full15": (15, False, False), "full9": (9, False, False), "compact9": (9, True, False), "pfp15": (15, False, True)}
GRID = [(d, k, B) for d in ("f32", "f64") for k in KINDS for B in (200, 70)]
GRID_IDS = [f"{d}-{k}-B{B}" for d, k, B in GRID]
SMALL = [(d, k) for d in ("f32", "f64") for k in KINDS]
SMALL_IDS = [f"{d}-{k}" for d, k in SMALL]


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
    return tuple(None if x is None else x.cpu().numpy() for x in ts)


def make_handles(dtype, kind, B, monkeypatch, seed, count=2, with_state=True, **kw):
    """`count` identical handles of the kind (with the case of lookahead_util.make_case as their state, or none), and the case."""
    n, compact, use_pfp = KINDS[kind]
    monkeypatch.setenv("QLE_COMPACT", "1" if compact else "0")   # read at handle creation, as tests/test_gpu_compact.py sets it
    monkeypatch.setenv("QLE_QUAD", "0")
    po, x, P, u, pfp = lu.make_case(dtype, n, use_pfp, B, seed)
    out = []
    for _ in range(count):
        ekf = qla.BatchedRelativePoseEKF(B, dtype, **dict(lu.KW, est_bias=int(n == 15), **kw))
        assert ekf.num_states == n and ekf.policy()["record_words"] == (64 if compact else 136)
        if with_state:
            ekf.set_state(x, P)
        if use_pfp:
            ekf.set_filter_params(pfp)
        out.append(ekf)
    return out, x, P, pfp


def raw(obj):
    """every word of the record array of a DeviceIO or a Snapshot"""
    obj.ekf.synchronize()
    return su.raw_read(obj._view())


def assert_states_equal(a, b, what):
    for got, ref, name in zip(a.get_state(), b.get_state(), "xP"):
        assert_same_bits(got, ref, f"{what}: {name}")


def close(*objs):
    for o in objs:
        o.close()


def tick_plan(rng, B, plan, handles, src=np.float32):
    """the same ticks on every handle: plan = a 0/1 per tick, 1 with tag poses"""
    for has_tag in plan:
        u = dev(rand_imu(rng, B).astype(src))
        z = dev(rand_pose(rng, B).astype(src)) if has_tag else None
        for io in handles:
            io.tick(u, z)


# ------------------------------------------------------------------------------------------------ 1. set_state from tensors
@pytest.mark.parametrize("src", ["float32", "float64"])
@pytest.mark.parametrize("dtype,kind,B", GRID, ids=GRID_IDS)
def test_set_state_from_tensors_equals_the_host_set_state(dtype, kind, B, src, monkeypatch):
    (a, twin), _, _, _ = make_handles(dtype, kind, B, monkeypatch, seed=100, with_state=False)
    n = a.num_states
    x, P = su.random_state(B, n, seed=B + n, dtype="f32" if src == "float32" else "f64")   # values of the source dtype, P not symmetric
    assert not np.array_equal(P, P.transpose(0, 2, 1))
    io, it = qla.DeviceIO(a), qla.DeviceIO(twin)
    twin.set_state(x, P)
    io.set_state(dev(x.astype(src)), dev(P.astype(src)))
    assert_states_equal(a, twin, f"set_state from {src}")
    words = raw(io)
    assert_same_bits(words, raw(it), "record words")
    assert np.abs(words).max() > 0
    io.set_state(*io.state())                                                 # the state written back onto itself
    assert_same_bits(raw(io), words, "record words after set_state(*state())")
    # one part at a time, and under a mask: the other part and the other filters keep their words
    x2, P2 = su.random_state(B, n, seed=B + n + 1, dtype="f32")
    mask = (np.arange(B) % 3 != 1).astype(np.uint8)
    io.set_state(dev(x2.astype(np.float32)), mask=dev(mask))
    io.set_state(None, dev(P2), mask=dev(mask.astype(bool)))
    want = su.expected_pack(words, B, dtype, KINDS[kind][1], x2, P2, mask)
    assert_same_bits(raw(io), want, "record words after the masked writes")
    close(io, it, a, twin)


# ------------------------------------------------------------------------------------------------ 2. a fresh handle ticks
@pytest.mark.parametrize("gating", [False, True], ids=["plain", "gating"])
@pytest.mark.parametrize("dtype,kind", SMALL, ids=SMALL_IDS)
def test_a_fresh_handle_given_only_device_set_state_ticks(dtype, kind, gating, monkeypatch):
    B = 200
    kw = dict(limit_measurement_freq=1) if gating else {}
    (a, twin), x, P, _ = make_handles(dtype, kind, B, monkeypatch, seed=200, with_state=False, **kw)
    for e in (a, twin):
        e.enable_gating(gating)
    with pytest.raises(qla.QleError) as e:                                    # no state yet: the tick library refuses
        a.predict(rand_imu(np.random.default_rng(0), B))
    assert e.value.code == _lib.QLE_ERR_STATE
    io, it = qla.DeviceIO(a), qla.DeviceIO(twin)
    twin.set_state(x, P)
    io.set_state(dev(x), dev(P))
    tick_plan(np.random.default_rng(201), B, (0, 1, 0), (io, it))
    assert_states_equal(a, twin, "after 3 ticks")
    if gating:
        for got, ref, name in zip(a.tick_flags(), twin.tick_flags(), ("performed_correction", "consumed", "upds_since_correction")):
            assert_same_bits(got, ref, name)
    assert a.count_nonfinite() == 0 and np.abs(a.get_state()[0] - x).max() > 0
    close(io, it, a, twin)


# ------------------------------------------------------------------------------------------------ 3. checkpoint replay
@pytest.mark.parametrize("dtype,kind", SMALL, ids=SMALL_IDS)
def test_restore_replays_the_ticks_after_the_snapshot(dtype, kind, monkeypatch):
    B = 200
    (a,), _, _, _ = make_handles(dtype, kind, B, monkeypatch, seed=300, count=1)
    io = qla.DeviceIO(a)
    tick_plan(np.random.default_rng(301), B, (0, 1, 0, 0, 1), (io,))
    snap = io.snapshot()
    at_snap = host(*io.state(), *io.report().values())
    words = raw(io)
    assert snap.view.state != io._view().state and snap.batch == B
    tick_plan(np.random.default_rng(302), B, (0, 0, 1, 0, 0), (io,))
    A = a.get_state()
    assert np.abs(A[0] - at_snap[0]).max() > 0
    assert io.restore(snap) is None
    assert_same_bits(raw(io)[su.record_offsets(B, dtype, su.RECORD_WORDS[KINDS[kind][1]])], words[su.record_offsets(B, dtype, su.RECORD_WORDS[KINDS[kind][1]])],
                     "record words after restore")
    tick_plan(np.random.default_rng(302), B, (0, 0, 1, 0, 0), (io,))
    for got, ref, name in zip(a.get_state(), A, "xP"):
        assert_same_bits(got, ref, f"replayed {name}")
    for got, ref, name in zip(host(*snap.state(), *snap.report().values()), at_snap, ("x", "P", "pose", "pose_cov", "vel", "bias")):
        assert_same_bits(got, ref, f"the snapshot's {name} after everything")
    st, fl, summary = snap.health(return_summary=True)                        # the other consumers of a view work on it
    assert host(summary)[0][0] == B and not host(fl)[0].any()
    f = snap.lookahead(dev(rand_imu(np.random.default_rng(303), B)), 3)
    assert np.isfinite(host(f.state()[0])[0]).all()
    close(io, a)


# ------------------------------------------------------------------------------------------------ 4. masked restore, word by word
@pytest.mark.parametrize("dtype,kind,B", GRID, ids=GRID_IDS)
def test_masked_restore_moves_the_masked_record_words_and_nothing_else(dtype, kind, B, monkeypatch):
    (a,), _, _, _ = make_handles(dtype, kind, B, monkeypatch, seed=400, count=1)
    compact = KINDS[kind][1]
    io = qla.DeviceIO(a)
    first, second = su.sentinel(B, dtype, seed=401), su.sentinel(B, dtype, seed=402, offset=0.25)   # they differ in every word
    a.synchronize()
    su.raw_write(io._view(), first)                                           # every word of the array, padding and ragged tail included
    snap = io.snapshot()
    rec = su.record_offsets(B, dtype, su.RECORD_WORDS[compact])
    assert_same_bits(raw(snap)[rec], first[rec], "the snapshot's record words")
    su.raw_write(io._view(), second)
    mask = (np.arange(B) % 5 != 2).astype(np.uint8); mask[B - 1] = 1; mask[0] = 0
    assert io.restore(snap, mask=dev(mask)) is None
    got = raw(io)
    want, _ = su.expected_copy(first, second, B, B, dtype, compact, None, mask)
    assert_same_bits(got, want, "the whole array after the masked restore")
    tail = su.off(np.arange(su.SW)[None, :], np.arange(B, su.padded(B))[:, None], dtype).ravel()
    pad = su.record_offsets(B, dtype, su.SW)[:, 136:].ravel()
    assert tail.size == (su.padded(B) - B) * su.SW and pad.size == 8 * B
    assert_same_bits(got[tail], second[tail], "the lanes beyond B"); assert_same_bits(got[pad], second[pad], "words 136..143")
    assert (bits_differ := (su.bits(got) != su.bits(second)).sum()) == int(mask.sum()) * su.RECORD_WORDS[compact], bits_differ
    close(io, a)


# ------------------------------------------------------------------------------------------------ 5. gather
def bad_index(rng, B, src_B=None):
    """an index over 0..src_B-1 with duplicates, across tiles, and with -1 and src_B (and far outside) in it"""
    src_B = B if src_B is None else src_B
    idx = rng.integers(0, src_B, B).astype(np.int32)
    idx[::7] = idx[3]
    idx[0], idx[1], idx[B - 1], idx[B // 2] = src_B - 1, -1, src_B, 2 ** 31 - 1
    idx[5] = -2 ** 31
    return idx


@pytest.mark.parametrize("dtype,kind,B", GRID, ids=GRID_IDS)
def test_gather_is_numpy_fancy_indexing_of_the_prior_state(dtype, kind, B, monkeypatch):
    (a, b), _, _, pfp = make_handles(dtype, kind, B, monkeypatch, seed=500)
    io = qla.DeviceIO(a)
    x0, P0 = a.get_state()
    idx = bad_index(np.random.default_rng(B), B)
    ok = (idx >= 0) & (idx < B)
    assert (~ok).sum() == 4 and len(set(idx[ok] // 64)) == su.padded(B) // 64 and len(set(idx[ok])) < ok.sum()
    written = host(io.gather(dev(idx)))[0]
    assert written.dtype == np.uint8 and np.array_equal(written, ok.astype(np.uint8))
    src = np.where(ok, idx, np.arange(B))                                     # a filter with a bad entry is untouched
    for got, ref, name in zip(a.get_state(), (x0[src], P0[src]), "xP"):
        assert_same_bits(got, ref, f"gather {name}")
    wb = b.gather_state(idx)                                                  # the host-array form
    assert np.array_equal(wb, written)
    assert_states_equal(b, a, "gather_state")
    mask = (np.arange(B) % 2).astype(np.uint8)                                # under a mask, from the state the first gather left
    x1, P1 = a.get_state()
    w2 = host(io.gather(dev(idx), mask=dev(mask)))[0]
    assert np.array_equal(w2, (ok & (mask != 0)).astype(np.uint8))
    src = np.where(w2 != 0, idx, np.arange(B))
    for got, ref, name in zip(a.get_state(), (x1[src], P1[src]), "xP"):
        assert_same_bits(got, ref, f"masked gather {name}")
    assert np.array_equal(b.gather_state(idx, mask), w2)
    assert_states_equal(b, a, "masked gather_state")
    if pfp is not None:
        assert_same_bits(a.get_filter_params(), b.get_filter_params(), "parameter records stay")
    close(io, a, b)


# ------------------------------------------------------------------------------------------------ 6. fork, and parameters that travel
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("B", [200, 72])
def test_fork_copies_the_source_member_and_keeps_the_parameter_records(dtype, B, monkeypatch):
    (a,), _, _, _ = make_handles(dtype, "pfp15", B, monkeypatch, seed=600, count=1)
    io = qla.DeviceIO(a)
    x0, P0 = a.get_state()
    pfp0 = a.get_filter_params()
    written = host(io.fork(4, source=1))[0]
    assert written.all()
    src = (np.arange(B) // 4) * 4 + 1
    for got, ref, name in zip(a.get_state(), (x0[src], P0[src]), "xP"):
        assert_same_bits(got, ref, f"fork {name}")
    assert_same_bits(a.get_filter_params(), pfp0, "parameter records after fork")
    assert len({r.tobytes() for r in pfp0}) == B                              # they are what tells the members apart
    # with_params: the parameter records of a snapshot travel
    snap = io.snapshot(with_params=True)
    x1, P1 = a.get_state()
    other = pfp0[::-1].copy()
    a.set_filter_params(other)
    a.set_state(x0, P0)
    assert io.restore(snap) is None                                           # without with_params: the state alone
    assert_same_bits(a.get_filter_params(), _held(a, other), "parameters stay")
    for got, ref, name in zip(a.get_state(), (x1, P1), "xP"):
        assert_same_bits(got, ref, f"restore {name}")
    io.restore(snap, with_params=True)
    assert_same_bits(a.get_filter_params(), pfp0, "parameters restored")
    idx = bad_index(np.random.default_rng(B + 1), B)
    ok = (idx >= 0) & (idx < B)
    a.set_filter_params(other)
    written = host(io.restore(snap, index=dev(idx), with_params=True))[0]
    assert np.array_equal(written, ok.astype(np.uint8))
    assert_same_bits(a.get_filter_params(), np.where(ok[:, None], pfp0[np.where(ok, idx, 0)], _held(a, other)), "parameters by index")
    with pytest.raises(ValueError, match="with_params"):
        io.restore(io.snapshot(), with_params=True)
    close(io, a)


def _held(ekf, pfp):
    """pfp as the handle's compute dtype holds it"""
    return pfp.astype(np.float32).astype(np.float64) if ekf.dtype == _lib.QLE_F32 else pfp


def test_snapshot_with_params_needs_parameter_records(monkeypatch):
    (a,), _, _, _ = make_handles("f32", "full15", 70, monkeypatch, seed=610, count=1)
    io = qla.DeviceIO(a)
    with pytest.raises(qla.QleError):
        io.snapshot(with_params=True)
    close(io, a)


# ------------------------------------------------------------------------------------------------ 7. from a small handle into a large one
@pytest.mark.parametrize("dtype,kind", SMALL, ids=SMALL_IDS)
def test_a_small_handles_snapshot_restores_into_a_large_handle_by_index(dtype, kind, monkeypatch):
    (small, small_twin), xs, Ps, _ = make_handles(dtype, kind, 70, monkeypatch, seed=700)
    (big, big_twin), _, _, _ = make_handles(dtype, kind, 200, monkeypatch, seed=701)
    ios, iost, iob, iobt = (qla.DeviceIO(e) for e in (small, small_twin, big, big_twin))
    tick_plan(np.random.default_rng(702), 70, (0, 1), (ios, iost))             # the small population has run
    idx = np.random.default_rng(703).integers(0, 70, 200).astype(np.int32)
    written = iob.restore(ios.snapshot(), index=dev(idx))                      # no synchronisation in between: ordered by the streams
    assert host(written)[0].all()
    x70, P70 = small.get_state()
    for got, ref, name in zip(big.get_state(), (x70[idx], P70[idx]), "xP"):
        assert_same_bits(got, ref, f"carried {name}")
    big_twin.set_state(x70[idx], P70[idx])                                     # the only route the host path has
    tick_plan(np.random.default_rng(704), 200, (0, 1, 0), (iob, iobt))
    tick_plan(np.random.default_rng(705), 70, (0, 1, 0), (ios, iost))
    assert_states_equal(big, big_twin, "the large handle ticks on")
    assert_states_equal(small, small_twin, "the small handle ticks on")
    with pytest.raises(ValueError, match="index"):
        iob.restore(ios.snapshot())
    close(ios, iost, iob, iobt, small, small_twin, big, big_twin)


# ------------------------------------------------------------------------------------------------ 8. isolation
@pytest.mark.parametrize("dtype,kind", SMALL, ids=SMALL_IDS)
def test_a_nan_record_reaches_exactly_the_filters_that_name_it(dtype, kind, monkeypatch):
    B = 200
    (a,), x, P, _ = make_handles(dtype, kind, B, monkeypatch, seed=800, count=1)
    compact = KINDS[kind][1]
    io = qla.DeviceIO(a)
    words = raw(io)
    k = 67                                                                     # one filter's record: NaN with a payload, every record word
    T, U = (np.float32, np.uint32) if dtype == "f32" else (np.float64, np.uint64)
    nan = np.array([0x7FC01234 if dtype == "f32" else 0x7FF8000000ABCDEF], U).view(T)[0]
    rec = su.record_offsets(B, dtype, su.RECORD_WORDS[compact])
    words[rec[k]] = nan
    su.raw_write(io._view(), words)
    idx = np.arange(B, dtype=np.int32)[::-1].copy()
    named = np.zeros(B, bool); named[[3, 64, 130, 199]] = True
    idx[named] = k
    assert idx[B - 1 - k] == k
    named[B - 1 - k] = True
    io.gather(dev(idx))
    got = raw(io)
    want, _ = su.expected_copy(words, words, B, B, dtype, compact, idx, None)
    assert_same_bits(got, want, "the whole array")
    is_nan = np.isnan(got[rec]).any(axis=1)
    assert np.array_equal(is_nan, named) and np.isnan(got[rec][named]).all()
    assert (su.bits(got[rec][named]) == su.bits(np.array([nan]))[0]).all()    # payload and all
    close(io, a)


@pytest.mark.parametrize("dtype,kind", SMALL, ids=SMALL_IDS)
def test_a_retired_filters_snapshot_restores_as_retired(dtype, kind, monkeypatch):
    B = 200
    (a,), x, P, _ = make_handles(dtype, kind, B, monkeypatch, seed=810, count=1)
    io = qla.DeviceIO(a)
    gone = np.zeros(B, np.uint8); gone[[0, 63, 64, 150, 199]] = 1
    io.retire(dev(gone))
    snap = io.snapshot()
    a.set_state(x, P)                                                          # every filter has a state again
    assert host(io.health(return_summary=True)[2])[0][2] == 0
    io.restore(snap)
    summary = host(io.health(return_summary=True)[2])[0]
    assert summary[2] == gone.sum() and summary[0] == B - gone.sum()           # uninitialised, evaluated
    assert host(snap.health(return_summary=True)[2])[0][2] == gone.sum()
    tick_plan(np.random.default_rng(811), B, (0, 1), (io,))
    xg, Pg = a.get_state()
    assert not xg[gone != 0].any() and not Pg[gone != 0].any()                # the ticks skipped them
    assert np.abs(xg[gone == 0] - x[gone == 0]).max() > 0 and a.count_nonfinite() == 0
    close(io, a)


# ------------------------------------------------------------------------------------------------ 9. multirate
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_multirate_whole_batch_writes_restart_the_history_as_the_host_set_state(dtype, monkeypatch):
    B = 200
    kw = dict(limit_measurement_freq=1, **MR)
    (a, twin), x, P, _ = make_handles(dtype, "full15", B, monkeypatch, seed=900, with_state=False, **kw)
    for e in (a, twin):
        e.enable_gating(True)
    io, it = qla.DeviceIO(a), qla.DeviceIO(twin)
    twin.set_state(x, P)
    io.set_state(dev(x), dev(P))
    tick_plan(np.random.default_rng(901), B, (0, 1, 0, 0), (io, it))           # filter_update ticks: the handles gate
    assert_states_equal(a, twin, "4 filter_update ticks after set_state")
    for got, ref, name in zip(a.tick_flags(), twin.tick_flags(), ("performed_correction", "consumed", "upds_since_correction")):
        assert_same_bits(got, ref, name)
    # a snapshot is the state, not the history: restoring it is the host's set_state(*get_state()) at the same tick
    snap = io.snapshot()
    io.restore(snap)
    twin.set_state(*twin.get_state())
    tick_plan(np.random.default_rng(902), B, (0, 1, 0, 0, 0, 1), (io, it))
    assert_states_equal(a, twin, "ticks after a whole-batch restore")
    idx = np.arange(B, dtype=np.int32)[::-1].copy()
    io.gather(dev(idx))                                                        # whole-batch gather: served
    x1, P1 = twin.get_state()
    twin.set_state(x1[idx], P1[idx])
    tick_plan(np.random.default_rng(903), B, (0, 1, 0), (io, it))
    assert_states_equal(a, twin, "ticks after a whole-batch gather")
    mask = dev(np.ones(B, np.uint8))
    for call in (lambda: io.set_state(dev(x), dev(P), mask=mask), lambda: io.restore(snap, mask=mask), lambda: io.gather(dev(idx), mask=mask),
                 lambda: a.gather_state(idx, np.ones(B, np.uint8))):
        with pytest.raises(qla.QleError, match="multirate_ekf") as e:
            call()
        assert e.value.code == _lib.QLE_ERR_STATE
    close(io, it, a, twin)


# ------------------------------------------------------------------------------------------------ 10. launches
def test_one_launch_per_call_and_two_per_gather(monkeypatch):
    B = 70
    (a,), x, P, _ = make_handles("f32", "pfp15", B, monkeypatch, seed=1000, count=1)
    io = qla.DeviceIO(a)
    count = stateio.stateio_lib().qsi_launch_count
    idx = dev(np.arange(B, dtype=np.int32)[::-1].copy())
    snap = io.snapshot()
    for call, n in ((lambda: io.set_state(dev(x), dev(P)), 1), (lambda: io.set_state(dev(x)), 1), (io.snapshot, 1),
                    (lambda: io.snapshot(with_params=True), 1), (lambda: io.restore(snap), 1), (lambda: io.restore(snap, index=idx), 1),
                    (lambda: io.gather(idx), 2), (lambda: io.fork(2), 2), (lambda: a.gather_state(np.arange(B)[::-1]), 2)):
        before = count()
        call()
        assert count() - before == n, n
    v = io._view()
    assert stateio.scheck(stateio.stateio_lib().qsi_workspace_bytes(C.byref(v))) == 128 * 144 * 4 == snap.workspace.numel()
    close(io, a)
