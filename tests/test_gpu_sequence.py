"""The sequence boundary on the GPU (quadrotor_landing_amd/sequence.py, DeviceIO.sequence / run, libqle_sequence.so): K ticks of torch
tensors packed in ceil(K / 32) launches and run from one native call.  The new path must produce the bits of the per-tick path
(DeviceIO.tick, report, nees called tick by tick), so EVERY comparison here is exact equality of bits; no tolerance appears.

Sizes: B = 2391 (ragged, 38 tiles, the cooperative kernels, every slab of a float32 tensor misaligned) and B = 4133 (ragged, lane
kernels, compact records with est_bias = 0); K = 70 ticks with tag slots at {0, 3, 31, 32, 33, 64, 69}: three chunks of the pack, with
slots on both sides of both chunk edges.
"""
import ctypes as C

import numpy as np
import pytest

import oracle
import quadrotor_landing_amd as qla
from gate_util import displaced_tag_poses
from quadrotor_landing_amd import _lib, devio, gate, sequence
from test_gpu_devio import assert_same_bits, rand_imu, rand_pose

pytestmark = pytest.mark.gpu

K = 70
TAGS = [0, 3, 31, 32, 33, 64, 69]
M = len(TAGS)
KW = dict(update_freq=400.0, measurement_freq=30.0, direct_orien_method=1, Q_a=[0.0005] * 3, Q_w=[0.00005] * 3,
          R_r=[0.015, 0.015, 0.020], R_ang=[0.0015, 0.0015, 0.04], ab_static=[0.2, -0.09, -0.03], wb_static=[-0.02, -0.01, 0.003],
          r_cov_init=0.01, ang_cov_init=0.01)
CHI2 = 16.81


def _torch():
    import torch as t
    return t


@pytest.fixture(autouse=True)
def torch_first():
    """torch is imported before the first handle of a test exists: a torch first imported after the engine has initialised the HIP
    runtime reports no GPU."""
    return _torch()


def dev(a, dtype=None):
    t = _torch()
    x = t.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        x = x.to(getattr(t, dtype))
    return x.to("cuda:0")


def host(x):
    _torch().cuda.synchronize()
    return x.cpu().numpy()


class Flight:
    """K ticks of inputs as device tensors of `src` (reference data, made once per (B, src) and left unchanged): U [K,B,6], Z [M,B,7]
    near the seed pose z0, masks [M,B], a truth [K,B,16] for the NEES, per-filter parameters."""

    def __init__(self, B, src):
        rng = np.random.default_rng(B + len(src))
        self.B, self.src = B, src
        self.z0 = rand_pose(rng, B)
        self.U = dev(np.stack([rand_imu(rng, B) for _ in range(K)]), src)
        Z = np.stack([self.z0.copy() for _ in range(M)])
        Z[:, :, :3] += rng.normal(0.0, 0.01, (M, B, 3))
        self.Z = dev(Z, src)
        self.mask = rng.uniform(size=(M, B)) < 0.7
        self.pfp_noise = rng.normal(0.0, 0.05, (B, 6))
        self._x_true = None

    @property
    def x_true(self):
        if self._x_true is None:
            rng, B = np.random.default_rng(self.B + 1), self.B
            xt = np.zeros((K, B, 16))
            xt[:, :, 0:3] = rng.uniform(-1.0, 1.0, (K, B, 3)) + [0.0, 0.0, 2.5]
            xt[:, :, 3:6] = rng.normal(0.0, 0.3, (K, B, 3))
            q = rng.normal(size=(K, B, 4)) * [0.2, 0.2, 0.2, 0.0] + [0.0, 0.0, 0.0, 1.0]
            xt[:, :, 6:10] = q / np.linalg.norm(q, axis=2, keepdims=True)
            xt[:, :, 10:16] = rng.normal(0.0, 0.05, (K, B, 6))
            self._x_true = dev(xt, self.src)
        return self._x_true

    def masks(self, kind):
        return None if kind is None else dev(self.mask.astype(np.uint8) if kind == "uint8" else self.mask)


_flights = {}


def flight(B, src="float32"):
    if (B, src) not in _flights:
        _flights[(B, src)] = Flight(B, src)
    return _flights[(B, src)]


def handle(f, dtype, pfp=False, gating=False, **over):
    """A handle seeded from the flight's z0 through io.seed: every handle made with the same arguments starts in the same state."""
    ekf = qla.BatchedRelativePoseEKF(f.B, dtype, **dict(KW, **over))
    if pfp:
        p = np.tile(np.concatenate([list(ekf.derived.Q), KW["ab_static"], KW["wb_static"], list(ekf.derived.R)]), (f.B, 1))
        p[:, 12:18] += f.pfp_noise
        ekf.set_filter_params(p)
    if gating:
        ekf.enable_gating(True)
    io = qla.DeviceIO(ekf)
    io.seed(dev(f.z0, "float64"))
    return ekf, io


def slot_of(k):
    return TAGS.index(k) if k in TAGS else None


def tick_loop(io, U, Z, masks, t0=0, n=K, chi2=None, every=None, trace=(), x_true=None):
    """The per-tick path: n calls of io.tick from slices of the sequence tensors (copies: a slice is not 16-byte aligned), with what
    io.run interleaves taken by io.report / io.nees."""
    acc, nis, rep, nees, summ = [], [], [], [], []
    for k in range(t0, t0 + n):
        s = slot_of(k)
        u = U[k].clone()
        if s is None:
            io.tick(u)
        else:
            z, m = Z[s].clone(), None if masks is None else masks[s].clone()
            if chi2 is None:
                io.tick(u, z, m)
            else:
                a, ni, _, _ = io.tick(u, z, m, chi2_max=chi2, return_nis=True)
                acc.append(a); nis.append(ni)
        if every and (k - t0 + 1) % every == 0:
            j = (k - t0 + 1) // every - 1
            if "report" in trace:
                rep.append(io.report())
            if "nees" in trace:
                ne, su = io.nees(x_true[j].clone())
                nees.append(ne); summ.append(su)
    return acc, nis, rep, nees, summ


def same_state(a, b, what):
    for (x, y), name in zip(zip(a.state(), b.state()), ("x", "P")):
        assert_same_bits(host(x), host(y), f"{what}: {name}")


# ------------------------------------------------------------------------------------------------ 1. pack
def _pack_twin(io, twin, view, f, U, Z, masks, ticks):
    """Ticks `ticks` of `twin` filled by one qdv_pack_inputs call each, from copies of the per-tick slices."""
    t = _torch()
    D = devio.devio_lib()
    s = 0
    for i, k in enumerate(ticks):
        iv = _lib.QleInputsView(); iv.struct_size = C.sizeof(iv)
        _lib.check(qla.lib().qle_inputs_get_device_view(twin._h, k, C.byref(iv)))
        u = U[i].clone()
        z = m = None
        if k in TAGS:
            z, m = Z[s].clone(), None if masks is None else masks[s].clone()
            s += 1
        devio._dcheck(D.qdv_wait_stream(C.byref(view), int(t.cuda.current_stream().cuda_stream)))   # the copies are made on torch's stream
        devio._dcheck(D.qdv_pack_inputs(C.byref(view), C.byref(iv), u.data_ptr(), None if z is None else z.data_ptr(),
                                        None if m is None else m.data_ptr(), devio._FLOATS[f.src]))
        t.cuda.synchronize()   # u, z, m die here


def _all_ticks(seq):
    return [seq.download_tick(k) for k in range(K)]


@pytest.mark.parametrize("B", [2391, 4133])
@pytest.mark.parametrize("src", ["float32", "float64"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_pack_equals_per_tick_packs(dtype, src, B):
    """Every tick of a sequence packed by ONE qsq_pack call reads back (download_tick) with the bits of a twin sequence filled by 70
    qdv_pack_inputs calls, for a uint8, a bool and no mask; a refill of ticks [5, 38) changes those ticks and no other; the launch
    count is ceil(n / 32)."""
    t = _torch()
    f = flight(B, src)
    if src == "float32":   # the slabs this size exists for: none of the odd ticks' starts on a 16-byte boundary
        assert (f.U[1].data_ptr() % 16, f.Z[1].data_ptr() % 16) != (0, 0)
    ekf = qla.BatchedRelativePoseEKF(B, dtype, **KW)
    io = qla.DeviceIO(ekf)
    view = io._view()
    S = sequence.sequence_lib()
    has = [int(k in TAGS) for k in range(K)]
    rng = np.random.default_rng(1)
    U2 = dev(np.stack([rand_imu(rng, B) for _ in range(33)]), src)
    Z2 = dev(np.stack([rand_pose(rng, B) for _ in range(3)]), src)
    for kind in ("uint8", "bool", None):
        masks = f.masks(kind)
        n0 = S.qsq_launch_count()
        mine = io.sequence(f.U, f.Z, TAGS, masks)
        assert S.qsq_launch_count() - n0 == 3
        assert mine.n_ticks == K and mine.meas_ticks == TAGS
        twin = ekf.make_inputs(K, has)
        _pack_twin(io, twin, view, f, f.U, f.Z, masks, range(K))
        ekf.synchronize()
        got, ref = _all_ticks(mine.inputs), _all_ticks(twin)
        for k in range(K):
            for g, r, name in zip(got[k], ref[k], "uzm"):
                assert_same_bits(g, r, f"mask {kind}, tick {k} {name}")
        assert all(ref[k][2].any() == (k in TAGS) for k in range(K))
        # refill [5, 38): slots 31, 32, 33
        M2 = None if masks is None else ~masks[1:4] if kind == "bool" else 1 - masks[1:4]
        n0 = S.qsq_launch_count()
        mine.pack(U2, Z2, M2, t0=5)
        assert S.qsq_launch_count() - n0 == 2
        _pack_twin(io, twin, view, f, U2, Z2, M2, range(5, 38))
        ekf.synchronize()
        got2, ref2 = _all_ticks(mine.inputs), _all_ticks(twin)
        for k in range(K):
            for g, r, b, name in zip(got2[k], ref2[k], got[k], "uzm"):
                assert_same_bits(g, r, f"mask {kind}, after the refill, tick {k} {name}")
                if not 5 <= k < 38:
                    assert_same_bits(g, b, f"mask {kind}, tick {k} {name} outside the refilled window")
        assert not np.array_equal(got2[20][0], got[20][0])
        mine.close(); twin.close()
    # the native entry refuses a range beyond the sequence, and tag poses for a range without a slot
    seq = io.sequence(f.U, f.Z, TAGS)
    assert S.qsq_pack(C.byref(view), seq.inputs._h, 60, 11, f.U.data_ptr(), None, None, devio._FLOATS[src]) == _lib.QLE_ERR_INVALID
    assert S.qsq_pack(C.byref(view), seq.inputs._h, 4, 10, f.U.data_ptr(), f.Z.data_ptr(), None, devio._FLOATS[src]) == _lib.QLE_ERR_INVALID
    assert S.qsq_pack(C.byref(view), seq.inputs._h, 0, 10, f.U.data_ptr(), None, None, devio._FLOATS[src]) == _lib.QLE_ERR_INVALID
    t.cuda.synchronize()
    seq.close(); ekf.close()


# ------------------------------------------------------------------------------------------------ 2. run equals the tick loop
MODES = {
    "full_records": (2391, dict(est_bias=1), dict()),
    "compact_records": (4133, dict(est_bias=0), dict()),
    "per_filter_params": (2391, dict(est_bias=1), dict(pfp=True)),
    "device_gating": (2391, dict(limit_measurement_freq=1, corner_margin_enbl=1), dict(gating=True)),
    "multirate_fixed_delay": (2391, dict(multirate_ekf=1, measurement_delay=12 / 400.0, limit_measurement_freq=1, corner_margin_enbl=1),
                              dict(gating=True)),
}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_run_equals_the_tick_loop(dtype, mode):
    """Two handles built and seeded identically, one driven by 70 io.tick calls, one by io.sequence + ONE io.run: state and tick flags
    are equal bit for bit, and the tick library's launch census names the same kernels."""
    B, over, how = MODES[mode]
    f = flight(B)
    masks = f.masks("uint8")
    a, ioa = handle(f, dtype, **how, **over)
    b, iob = handle(f, dtype, **how, **over)
    if mode == "compact_records":
        assert a.policy()["record_words"] == 64   # the compact case cannot silently test full records
    x0 = host(ioa.state()[0])
    ioa.tick(f.U[0].clone()); iob.tick(f.U[0].clone())   # the private two-tick sequences exist now; both handles alike
    with qla.launch_census() as loop:
        tick_loop(ioa, f.U, f.Z, masks)
    seq = iob.sequence(f.U, f.Z, TAGS, masks)
    with qla.launch_census() as run:
        res = iob.run(seq)
    assert res.accepted is None and res.report is None and res.nees is None
    same_state(ioa, iob, mode)
    assert np.abs(host(ioa.state()[0]) - x0).max() > 1e-3 and np.isfinite(host(ioa.state()[1])).all()
    if how.get("gating"):
        for p, q, what in zip(a.tick_flags(), b.tick_flags(), ("performed_correction", "consumed", "upds_since_correction")):
            assert_same_bits(p, q, f"{mode}: {what}")
    assert loop == run and len(run) >= 1, (loop, run)
    seq.close(); a.close(); b.close()


# ------------------------------------------------------------------------------------------------ 3. gated run
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_gated_run_equals_gated_ticks_and_leaves_the_accepted_masks(dtype):
    B = 2391
    f = flight(B)
    t = _torch()
    po = oracle.make_params(**KW)
    rng = np.random.default_rng(9)
    a, ioa = handle(f, dtype)
    b, iob = handle(f, dtype)
    c, ioc = handle(f, dtype)
    G = gate.gate_lib()
    # the twin first, tick by tick: its tag poses are made around its own state, 30 % of them displaced
    Z, acc, nis = [], [], []
    for k in range(K):
        u = f.U[k].clone()
        if k in TAGS:
            z, _ = displaced_tag_poses(rng, po, a.get_state()[0])
            Z.append(dev(z, "float32"))
            ak, nk, _, _ = ioa.tick(u, Z[-1], chi2_max=CHI2, return_nis=True)
            acc.append(ak); nis.append(nk)
        else:
            ioa.tick(u)
    Zs = t.stack(Z)
    acc_ref, nis_ref = host(t.stack(acc)), host(t.stack(nis))
    for m in range(M):   # a condition on the input, not a result: both outcomes occur at every tag tick
        assert acc_ref[m].any() and not acc_ref[m].all(), (m, acc_ref[m].mean())
    seq = iob.sequence(f.U, Zs, TAGS)
    g0 = G.qgt_launch_count()
    res = iob.run(seq, chi2_max=CHI2, return_nis=True)
    assert G.qgt_launch_count() - g0 == M
    assert tuple(res.accepted.shape) == (M, B) and tuple(res.nis.shape) == (M, B)
    assert_same_bits(host(res.accepted), acc_ref, "accepted")
    assert_same_bits(host(res.nis), nis_ref, "nis")
    same_state(ioa, iob, "gated run")
    # the sequence now holds the accepted masks: the spent sequence, ungated, on a third handle seeded alike
    for m, k in enumerate(TAGS):
        assert np.array_equal(seq.inputs.download_tick(k)[2] != 0, acc_ref[m] != 0)
    ins = ioc.ekf.make_inputs(K, [int(k in TAGS) for k in range(K)])
    for k in range(K):   # a sequence belongs to its handle: the spent records, read back and uploaded to the third handle's own
        u, z, m = seq.inputs.download_tick(k)
        ins.upload_tick(k, u, z if k in TAGS else None, m if k in TAGS else None)
    g0 = G.qgt_launch_count()
    c.run(ins, 0, K)
    assert G.qgt_launch_count() == g0
    same_state(ioa, ioc, "ungated replay of the spent sequence")
    seq.close(); ins.close(); a.close(); b.close(); c.close()


def test_spent_sequence_replays_on_its_own_handle():
    """The same through io.run alone: a gated run, the handle seeded again, the spent sequence run without a gate."""
    B = 2391
    f = flight(B)
    t = _torch()
    po = oracle.make_params(**KW)
    rng = np.random.default_rng(10)
    a, io = handle(f, "f32")
    Zs = t.stack([dev(displaced_tag_poses(rng, po, a.get_state()[0])[0], "float32") for _ in range(M)])
    seq = io.sequence(f.U, Zs, TAGS)
    res = io.run(seq, chi2_max=CHI2)
    acc = host(res.accepted)
    assert acc.any() and not acc.all() and res.nis is None
    x1, P1 = (host(v) for v in io.state())
    io.seed(dev(f.z0, "float64"), reinit_bias=True)   # the start state again: a fresh handle's bias words are zero
    assert io.run(seq).accepted is None
    x2, P2 = (host(v) for v in io.state())
    assert_same_bits(x1, x2, "x"); assert_same_bits(P1, P2, "P")
    seq.close(); a.close()


# ------------------------------------------------------------------------------------------------ 4. trace
@pytest.mark.parametrize("every", [1, 7])
@pytest.mark.parametrize("dtype,B,over", [("f32", 2391, dict(est_bias=1)), ("f64", 4133, dict(est_bias=0))])
def test_trace_equals_report_and_nees_on_the_twin(dtype, B, over, every):
    t = _torch()
    f = flight(B)
    masks = f.masks("bool")
    J = K // every
    a, ioa = handle(f, dtype, **over)
    b, iob = handle(f, dtype, **over)
    xt = f.x_true[:J]
    _, _, rep, nees, summ = tick_loop(ioa, f.U, f.Z, masks, every=every, trace=("report", "nees"), x_true=xt)
    assert len(rep) == len(nees) == J
    # the pitched buffers are written with a sentinel before the run (they are what io._alloc hands out)
    SENT = {"float32": -7.5, "float64": -7.5, "uint8": 0xA5}
    alloc = iob._alloc
    iob._alloc = lambda shapes, dn: [x.fill_(SENT[dn]) for x in alloc(shapes, dn)]
    seq = iob.sequence(f.U, f.Z, TAGS, masks)
    res = iob.run(seq, trace_every=every, trace=("report", "nees"), x_true_seq=xt)
    iob._alloc = alloc
    Bp = -(-B // 64) * 64
    assert tuple(res.nees.shape) == (J, B) and tuple(res.summary.shape) == (J, 8)
    for j in range(J):
        for key in ("pose", "pose_cov", "vel", "bias"):
            assert_same_bits(host(res.report[key][j]), host(rep[j][key]), f"slice {j} {key}")
        assert_same_bits(host(res.nees[j]), host(nees[j]), f"slice {j} nees")
        assert_same_bits(host(res.summary[j]), host(summ[j]), f"slice {j} summary")
    assert host(res.summary)[:, 0].min() > 0
    for name, v in list(res.report.items()) + [("nees", res.nees)]:
        base = v._base
        assert base is not None and base.shape[1] == Bp and base.shape[0] == J, name
        pad = host(base[:, B:])
        assert pad.size > 0 and (pad == -7.5).all(), f"{name}: padding rows were written"
    same_state(ioa, iob, "traced run")
    seq.close(); a.close(); b.close()


def test_trace_selection_and_gate_together():
    """trace=("nees",) with a block selection and a bound, in a gated run of a window [5, 38): slices, gate outputs and padding."""
    t = _torch()
    B, every, t0, n = 2391, 7, 5, 33
    f = flight(B)
    J = n // every
    a, ioa = handle(f, "f32")
    b, iob = handle(f, "f32")
    xt = f.x_true[:J]
    acc, nis, rep, nees, summ = [], [], [], [], []
    s0 = sum(1 for k in TAGS if k < t0)
    for k in range(t0, t0 + n):
        if k in TAGS:
            r = ioa.tick(f.U[k].clone(), f.Z[TAGS.index(k)].clone(), chi2_max=CHI2, return_nis=True)
            acc.append(r[0]); nis.append(r[1])
        else:
            ioa.tick(f.U[k].clone())
        if (k - t0 + 1) % every == 0:
            ne, su = ioa.nees(xt[(k - t0 + 1) // every - 1].clone(), blocks="pose", chi2_hi=12.0)
            nees.append(ne); summ.append(su)
    seq = iob.sequence(f.U, f.Z, TAGS)
    res = iob.run(seq, t0, n, chi2_max=CHI2, return_nis=True, trace_every=every, trace="nees", x_true_seq=xt, blocks="pose", chi2_hi=12.0)
    assert res.report is None and tuple(res.accepted.shape) == (3, B) and s0 == 2
    assert_same_bits(host(res.accepted), host(t.stack(acc)), "accepted")
    assert_same_bits(host(res.nis), host(t.stack(nis)), "nis")
    assert_same_bits(host(res.nees), host(t.stack(nees)), "nees")
    assert_same_bits(host(res.summary), host(t.stack(summ)), "summary")
    assert host(res.summary)[:, 7].tolist() == [6.0] * J
    same_state(ioa, iob, "gated, traced window")
    seq.close(); a.close(); b.close()


# ------------------------------------------------------------------------------------------------ 5. partial runs
@pytest.mark.parametrize("dtype,mode", [("f32", "full_records"), ("f64", "multirate_fixed_delay")])
def test_partial_runs_add_up(dtype, mode):
    B, over, how = MODES[mode]
    f = flight(B)
    masks = f.masks("uint8")
    a, ioa = handle(f, dtype, **how, **over)
    b, iob = handle(f, dtype, **how, **over)
    sa, sb = ioa.sequence(f.U, f.Z, TAGS, masks), iob.sequence(f.U, f.Z, TAGS, masks)
    ioa.run(sa, 0, 70)
    iob.run(sb, 0, 33); iob.run(sb, 33, 37)
    same_state(ioa, iob, "run(0, 33) + run(33, 37) against run(0, 70)")
    with pytest.raises(qla.QleError):   # no wrap here
        S = sequence.sequence_lib()
        sequence.scheck(S.qsq_run(b._h, sb.inputs._h, 60, 11, None))
    sa.close(); sb.close(); a.close(); b.close()


# ------------------------------------------------------------------------------------------------ 6. stream ordering
def test_stream_ordering_without_synchronisation():
    """Source tensors overwritten on the caller's stream right after io.sequence returns do not change the packed records, and trace
    outputs read on the caller's stream right after io.run returns are complete: no explicit synchronisation in between, on a
    non-default stream, against the same calls with a device synchronisation after each."""
    t = _torch()
    B, every = 16384 + 37, 10
    f = flight(B)
    masks = f.masks("uint8")
    out = []
    for sync in (False, True):
        ekf, io = handle(f, "f32")
        s = t.cuda.Stream(device=0)
        t.cuda.synchronize()
        with t.cuda.stream(s):
            U, Z, Mk = f.U * 1.0, f.Z + 0.0, masks.clone()      # produced on s right before the pack
            seq = io.sequence(U, Z, TAGS, Mk)
            if sync:
                t.cuda.synchronize()
            U.zero_(); Z.fill_(3.0); Mk.zero_()                  # overwritten on s right after it
            if sync:
                t.cuda.synchronize()
            res = io.run(seq, trace_every=every)
            if sync:
                t.cuda.synchronize()
            pose = res.report["pose"].clone()                    # consumed on s right after the run
            tot = res.report["pose_cov"].sum(dim=(1, 2, 3), dtype=t.float64)
            x, P = io.state()
        s.synchronize()
        out.append((pose.cpu().numpy(), tot.cpu().numpy(), x.cpu().numpy(), P.cpu().numpy(), seq.inputs.download_tick(69)[1],
                    seq.inputs.download_tick(37)[0]))
        seq.close(); ekf.close()
    assert np.isfinite(out[0][0]).all() and np.abs(out[0][1]).min() > 0
    assert np.abs(out[0][4] - 3.0).max() > 0.1 and np.abs(out[0][5]).max() > 1.0   # the records hold the sources as they were
    for p, q, what in zip(out[0], out[1], ("pose trace", "pose_cov sums", "x", "P", "z of tick 69", "u of tick 37")):
        assert_same_bits(p, q, what)


# ------------------------------------------------------------------------------------------------ 7. the native entry's refusals
def test_native_run_refuses_before_any_launch_and_carries_the_callee_message():
    """qsq_run on a live handle: every refusal leaves the state as it was, a gate with multirate_ekf is QLE_ERR_STATE, and the message
    of a callee that fails (here qle_run, given another handle's sequence) arrives in qsq_last_error()."""
    t = _torch()
    f = flight(2391)
    a, io = handle(f, "f32")
    b, iob = handle(f, "f32", multirate_ekf=1, measurement_delay=12 / 400.0)
    seq, seqb = io.sequence(f.U, f.Z, TAGS), iob.sequence(f.U, f.Z, TAGS)
    S, G = sequence.sequence_lib(), gate.gate_lib()
    buf = t.zeros(4096, dtype=t.float32, device="cuda:0")
    x0, P0 = (host(v) for v in io.state())

    def run(h=a, s=seq, t0=0, n=K, **kw):
        o = sequence.QsqRunOpts()
        o.struct_size = C.sizeof(o)
        o.params = C.pointer(h.params)
        for k, v in kw.items():
            setattr(o, k, v)
        return S.qsq_run(h._h, s.inputs._h, t0, n, C.byref(o)), S.qsq_last_error().decode()

    g0, c0 = G.qgt_launch_count(), S.qsq_launch_count()
    with qla.launch_census() as launched:
        for kw, word in ((dict(chi2_max=-1.0), "chi2_max"), (dict(chi2_max=float("nan")), "chi2_max"), (dict(pose=buf.data_ptr()), "trace_every"),
                         (dict(nees=buf.data_ptr(), x_true_seq=buf.data_ptr()), "trace_every"), (dict(accepted=buf.data_ptr()), "gate"),
                         (dict(t0=60, n=11), "beyond"), (dict(t0=-1), "t0"), (dict(struct_size=8), "struct_size"),
                         (dict(trace_every=7, nees=buf.data_ptr()), "x_true_seq"), (dict(trace_every=7, pose=buf.data_ptr() + 4), "aligned"),
                         (dict(trace_every=7, nees=buf.data_ptr(), x_true_seq=buf.data_ptr(), blocks=0, chi2_hi=1.0), "blocks"),
                         (dict(trace_every=7, pose=buf.data_ptr(), dst_dtype=5), "dst_dtype")):
            rc, msg = run(**kw)
            assert rc == _lib.QLE_ERR_INVALID and word in msg, (kw, rc, msg)
        rc, msg = run(h=b, s=seqb, chi2_max=CHI2)
        assert rc == _lib.QLE_ERR_STATE and "multirate_ekf" in msg, (rc, msg)
        rc, msg = run(h=b, s=seq, n=1)   # another handle's sequence: the tick library refuses, its words are carried over
        assert rc == _lib.QLE_ERR_INVALID and msg.startswith("qle_run at tick 0") and "do not belong to this handle" in msg, (rc, msg)
    assert launched == [] and G.qgt_launch_count() == g0 and S.qsq_launch_count() == c0
    x1, P1 = (host(v) for v in io.state())
    assert_same_bits(x0, x1, "x"); assert_same_bits(P0, P1, "P")
    seq.close(); seqb.close(); a.close(); b.close()
