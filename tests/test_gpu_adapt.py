"""Noise adaptation on the GPU (include/qle_adapt.h, libqle_adapt.so: k_adapt_observe, k_adapt_apply; DeviceIO.adapter(),
BatchedRelativePoseEKF.adapt_noise).

Reference: adapt_util.reference_run -- per tag tick the dense oracle's prediction_step followed by the numpy restatement of the innovation
(gate_util.predict_then_innovation), N as innovation_util builds it, a and c by numpy.linalg.solve, plain fp64 sums, the apply formula in
numpy -- stepped by oracle.run_batch with per_filter_params carrying the current R.  In fp32 the free-running state drifts from the oracle
over 24 ticks, so there the reference is teacher-forced: in front of every tag tick it takes the state the GPU holds.  For the apply step
the reference applies the GPU's own accumulators, so that the apply is checked on its own and not through accumulated drift.  Counts are
exact; the sums are held to adapt_util.TOL["gpu"], the applied R to adapt_util.APPLY_TOL, measured and stated in
tests/tolerances_adapt.md.  Batches of 100 (a ragged second tile) and 65; K = 24 ticks with a tag slot every third: 8 tag ticks, window
4, two applies.
"""
import ctypes as C

import numpy as np
import pytest

import oracle
import quadrotor_landing_amd as qla
from adapt_util import APPLY_TOL, COUNTS, TOL, apply_error, apply_ref, deviations, reference_run
from oracle import ekf_np
from quadrotor_landing_amd import adapt
from score_util import make_sequence
from test_gpu_innovation import Case, _same

pytestmark = pytest.mark.gpu

K = 24
MEAS = list(range(2, K, 3))   # 8 tag ticks
WINDOW, N_MIN = 4, 2


def _torch():
    import torch as t
    return t


@pytest.fixture(autouse=True)
def torch_first():
    """torch is imported before the first handle of a test exists: a torch that is first imported after the engine has initialised the
    HIP runtime reports no GPU."""
    return _torch()


def dev(c, a):
    """a numpy array as a device tensor of the handle's compute dtype (what the device then holds, exactly)"""
    t = _torch()
    if a.dtype == np.uint8 or a.dtype == bool:
        return t.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    return t.from_numpy(np.ascontiguousarray(a.astype(np.float32 if c.dtype == "f32" else np.float64))).to("cuda:0")


def held(c, a):
    return a.astype(np.float32).astype(np.float64) if c.dtype == "f32" else a


def host(t):
    _torch().cuda.synchronize()
    return t.cpu().numpy()


def acc_of(ad):
    """the accumulators as the reference holds them: [B, 24] on the host"""
    return np.ascontiguousarray(host(ad.acc)[:, :ad.io.ekf.batch].T)


class Run:
    """A handle, K ticks of inputs built around the oracle's own run, per-filter parameters in force, and the packed sequence."""

    def __init__(self, dtype, direct, est_bias, use_pfp, batch, mask=None, pos=0.02):
        c = self.c = Case(dtype, direct, est_bias, use_pfp, batch=batch, cov_scale=0.05)
        self.x0, self.P0 = c.ekf.get_state()
        U, Z = make_sequence(c.rng, c.po, self.x0, self.P0, K, MEAS, c.pfp, pos=pos)
        self.U, self.Z = held(c, U), held(c, Z)
        self.M = np.ones((len(MEAS), batch), np.uint8) if mask is None else mask
        self.io = qla.DeviceIO(c.ekf)
        self.R0 = np.array(list(c.po.R))
        self.pfp0 = None

    def adapter(self, **kw):
        """a fresh Adapter (window 4 unless said); the first one puts per-filter parameters in force where the case has none"""
        kw.setdefault("window", WINDOW)
        ad = self.io.adapter(**kw)
        if self.pfp0 is None:
            self.pfp0 = self.c.ekf.get_filter_params()
        return ad

    def pack(self, Z=None, M=None):
        c = self.c
        return self.io.sequence(dev(c, self.U), dev(c, self.Z if Z is None else Z), MEAS, dev(c, self.M if M is None else M))

    def restart(self, x=None, P=None):
        self.c.ekf.set_state(self.x0 if x is None else x, self.P0 if P is None else P)
        self.c.ekf.set_filter_params(self.pfp0)

    def tick_args(self, t, Z=None, M=None):
        c = self.c
        if t not in MEAS:
            return (dev(c, self.U[t]),)
        j = MEAS.index(t)
        return dev(c, self.U[t]), dev(c, (self.Z if Z is None else Z)[j]), dev(c, (self.M if M is None else M)[j])

    def close(self):
        self.io.close()
        self.c.close()


def layout(monkeypatch, est_bias):
    """est_bias = 0 runs on compact records (forced: by default these small batches keep full records for the workgroup-cooperative
    kernel, which est_bias = 1 runs on), so that both layouts' instantiations of k_adapt_observe are held"""
    if not est_bias:
        monkeypatch.setenv("QLE_COMPACT", "1")


def end_state(r, ad):
    x, P = r.c.ekf.get_state()
    return acc_of(ad), r.c.ekf.get_filter_params(), x, P


def same_end(a, b):
    return all(_same(p, q) for p, q in zip(a, b))


GRID = [(d, o, e) for d in ("f64", "f32") for o in (1, 0) for e in (1, 0)]
grid = pytest.mark.parametrize("dtype,direct,est_bias", GRID, ids=[f"{d}-direct{o}-bias{e}" for d, o, e in GRID])


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("batch", [100, 65])
@grid
def test_adapted_run_matches_the_step_loop_the_pieces_and_the_reference(dtype, direct, est_bias, batch, monkeypatch):
    layout(monkeypatch, est_bias)
    r = Run(dtype, direct, est_bias, batch == 100, batch)   # batch 100: per-filter noise spread over 0.3 .. 3 x nominal; 65: the shared record
    c, io = r.c, r.io
    assert bool(io._view().compact) == (est_bias == 0)
    seq = r.pack()
    lo, hi = r.R0 / 100, r.R0 * 100
    # (a) one native call
    whole = r.adapter()
    assert whole.cfg.n_min == N_MIN
    whole.run(seq)
    end = end_state(r, whole)
    # (b) the loop of step from Python
    r.restart()
    loop = r.adapter()
    outs = [loop.step(*r.tick_args(t)) for t in range(K)]
    assert same_end(end_state(r, loop), end)
    assert [o is not None for o in outs] == [t in (MEAS[3], MEAS[7]) for t in range(K)]
    # (c) in pieces of whole windows
    r.restart()
    pieces = r.adapter()
    pieces.run(seq, 0, 12)
    pieces.run(seq, 12)
    assert same_end(end_state(r, pieces), end)
    # (d) observe, tick and apply by hand, with the state the GPU holds in front of every tag tick (the teacher of the fp32 reference), the
    # accumulators in front of every apply and the R behind it
    r.restart()
    hand = r.adapter()
    forced, gpu, applied = {}, {}, []
    for t in range(K):
        args = r.tick_args(t)
        if t in MEAS:
            forced[t] = c.ekf.get_state()
            hand.observe(*args)
        io.tick(*args)
        if t in (MEAS[3], MEAS[7]):
            before = acc_of(hand)
            R, ap = hand.apply()
            R, ap = host(R), host(ap)
            assert _same(R, c.ekf.get_filter_params()[:, 18:24])
            gpu[len(applied)] = (before, R)
            applied.append(ap)
    assert same_end(end_state(r, hand), end)
    for o, ap, (_, R) in zip([o for o in outs if o is not None], applied, gpu.values()):
        assert _same(host(o[0]), R) and np.array_equal(host(o[1]), ap)
    # against the reference
    acc = end[0]
    ref, applies = reference_run(c.po, c.p, r.x0, r.P0, r.U, r.Z, r.M, MEAS, r.pfp0, WINDOW, 1.0, N_MIN, lo, hi, dtype,
                                 forced=forced if dtype == "f32" else None, gpu=gpu)
    np.testing.assert_array_equal(acc[:, COUNTS], ref.acc[:, COUNTS])
    assert (acc[:, 20] == 8).all() and (acc[:, 21] == 2).all() and not acc[:, [0, 1, 22, 23]].any() and not acc[:, 2:20].any()
    worst = {g: 0.0 for g in TOL["gpu"][dtype]}
    for j, (ref_before, R_np, ref_applied, clamped) in enumerate(applies):
        before, R = gpu[j]
        np.testing.assert_array_equal(before[:, COUNTS], ref_before.acc[:, COUNTS])
        assert np.array_equal(applied[j] != 0, ref_applied) and np.array_equal(applied[j] != 0, before[:, 0] >= N_MIN) and applied[j].all()
        d = deviations(before, ref_before)
        worst = {g: max(worst[g], d[g]) for g in d}
        rel, eq = apply_error(R, R_np, clamped)
        print(f"apply {j}: worst relative deviation of R from the numpy apply {rel:.2e}, {int(clamped.sum())} clamped")
        assert rel <= APPLY_TOL[dtype] and eq, (rel, eq)
    print(f"{dtype} direct={direct} bias={est_bias} B={batch}: " + " ".join(f"{g} {v:.2e}" for g, v in worst.items()))
    tol = TOL["gpu"][dtype]
    assert all(worst[g] < tol[g] for g in worst), (worst, tol)
    Rend = end[1][:, 18:24]
    assert np.isfinite(Rend).all() and (Rend > 0).all() and _same(end[1][:, :18], r.pfp0[:, :18])
    # result(): the statistics of the words
    res = hand.result()
    np.testing.assert_array_equal(host(res.n_total), acc[:, 20])
    assert tuple(res.r_hat.shape) == (batch, 6) and tuple(res.ratio.shape) == (batch, 6)
    seq.close()
    r.close()


# ------------------------------------------------------------------------------------------------ 2. read-only and write set
@pytest.mark.parametrize("dtype,est_bias,batch", [("f32", 1, 65), ("f64", 0, 100)])
def test_observe_is_read_only_and_apply_writes_the_noise_words_of_applied_filters_alone(dtype, est_bias, batch, monkeypatch):
    layout(monkeypatch, est_bias)
    rng = np.random.default_rng(5)
    r = Run(dtype, 1, est_bias, True, batch, mask=(rng.uniform(size=(len(MEAS), batch)) < 0.5).astype(np.uint8))
    c, io = r.c, r.io
    ad = r.adapter()
    Q = adapt.adapt_lib()
    for t in range(MEAS[0]):
        io.tick(*r.tick_args(t))
    for j in range(3):   # three observed tag ticks with random masks: n = 0 .. 3
        args = r.tick_args(MEAS[j])
        ad.observe(*args)
        if j < 2:
            io.tick(*args)
    # the slot holds the third tag tick, packed; the kernel once more, on its own
    x0, P0 = c.ekf.get_state()
    rec0, pfp0 = io._seq.download_tick(1), c.ekf.get_filter_params()
    n0 = Q.qad_launch_count()
    view, iv = io._view(), io._inputs_view(1)
    adapt.qcheck(Q.qad_observe_tick(C.byref(view), C.byref(iv), C.byref(c.ekf.params), ad.acc.data_ptr(), float("inf")))
    assert Q.qad_launch_count() - n0 == 1
    x1, P1 = c.ekf.get_state()
    assert _same(x0, x1) and _same(P0, P1) and _same(pfp0, c.ekf.get_filter_params())
    for a, b in zip(io._seq.download_tick(1), rec0):   # IMU record, tag record, mask word
        assert _same(a, b)
    assert np.array_equal(rec0[2] != 0, r.M[2] != 0)
    acc = acc_of(ad)
    np.testing.assert_array_equal(acc[:, 0], r.M[0].astype(float) + r.M[1] + 2.0 * r.M[2])
    n0 = Q.qad_launch_count()
    R, applied = ad.apply()
    assert Q.qad_launch_count() - n0 == 1
    R, applied = host(R), host(applied)
    pfp1, acc1 = c.ekf.get_filter_params(), acc_of(ad)
    assert np.array_equal(applied != 0, acc[:, 0] >= N_MIN) and 0 < applied.sum() < batch
    off = applied == 0
    assert _same(pfp1[:, :18], pfp0[:, :18]) and _same(pfp1[off], pfp0[off]) and _same(acc1[off], acc[off])
    assert _same(R, pfp1[:, 18:24]) and not (pfp1[~off, 18:24] == pfp0[~off, 18:24]).all(axis=1).any()
    want, _, _, _ = apply_ref(acc, pfp0[:, 18:24], 1.0, N_MIN, r.R0 / 100, r.R0 * 100, dtype)
    np.testing.assert_array_equal(acc1[:, COUNTS], want[:, COUNTS])
    assert not acc1[~off, 2:20].any() and _same(acc1[:, 20], acc[:, 20])
    x2, P2 = c.ekf.get_state()
    assert _same(x0, x2) and _same(P0, P2)
    r.close()


# ------------------------------------------------------------------------------------------------ 3. the tick uses what apply wrote
@pytest.mark.parametrize("dtype,direct,est_bias", [("f32", 1, 1), ("f64", 0, 0)])
def test_the_tick_behind_an_apply_uses_the_noise_it_wrote(dtype, direct, est_bias, monkeypatch):
    layout(monkeypatch, est_bias)
    batch = 100
    r = Run(dtype, direct, est_bias, False, batch)
    c, io = r.c, r.io
    ad = r.adapter()
    for t in range(MEAS[3] + 1):
        ad.step(*r.tick_args(t))
    pfp = c.ekf.get_filter_params()
    assert not (pfp[:, 18:24] == r.pfp0[:, 18:24]).any()
    for t in range(MEAS[3] + 1, MEAS[4]):
        io.tick(*r.tick_args(t))
    x, P = c.ekf.get_state()
    other = Case(dtype, direct, est_bias, False, batch=batch, cov_scale=0.05)
    other.ekf.set_state(x, P)
    other.ekf.set_filter_params(pfp)
    io2 = qla.DeviceIO(other.ekf)
    args = r.tick_args(MEAS[4])
    io.tick(*args)
    io2.tick(*args)
    for a, b in zip(c.ekf.get_state(), other.ekf.get_state()):
        assert _same(a, b)
    io2.close()
    other.close()
    r.close()


# ------------------------------------------------------------------------------------------------ 4. masks, lifecycle, isolation
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_filters_that_are_off_accumulate_nothing_and_a_nan_pose_stays_in_its_filter(dtype):
    t = _torch()
    B, Bp = 100, 128
    UNSEEDED, RETIRED, MASKED, NANPOSE = 3, 70, 64, 99
    SENTINEL = -7.0
    r = Run(dtype, 1, 1, True, B)
    c, io = r.c, r.io
    x0 = r.x0.copy(); x0[UNSEEDED] = 0.0
    M = r.M.copy(); M[:, MASKED] = 0
    Znan = r.Z.copy(); Znan[7, NANPOSE, 1] = np.nan   # on the last tag tick: the tick behind it takes the pose in, nothing follows it
    retire = np.zeros(B, np.uint8); retire[RETIRED] = 1
    ends = []
    for Z in (r.Z, Znan):
        ad = r.adapter()
        r.restart(x0)
        io.retire(dev(c, retire))
        ad.acc[:, B:] = SENTINEL   # the columns of the lanes beyond the ragged end: a guard region
        for tick in range(K - 1):
            ad.step(*r.tick_args(tick, Z, M))
        args = r.tick_args(K - 1, Z, M)
        ad.observe(*args)
        full = host(ad.acc).copy()
        # the last apply by hand, into outputs with sentinel rows behind the batch
        R_out = t.full((Bp, 6), SENTINEL, dtype=t.float64, device="cuda:0")
        flags = t.full((Bp,), 77, dtype=t.uint8, device="cuda:0")
        view = io._view()
        with io._ordered(view, ad.acc, R_out, flags):
            adapt.qcheck(adapt.adapt_lib().qad_apply(C.byref(view), ad.acc.data_ptr(), C.byref(ad.cfg), flags.data_ptr(), R_out.data_ptr()))
        R_out, flags = host(R_out), host(flags)
        assert (R_out[B:] == SENTINEL).all() and (flags[B:] == 77).all() and (full[:, B:] == SENTINEL).all() and (host(ad.acc)[:, B:] == SENTINEL).all()
        ends.append((full[:, :B].T.copy(), acc_of(ad), c.ekf.get_filter_params(), flags[:B], R_out[:B]))
    for before, acc, pfp, flags, R_out in ends:
        for i in (UNSEEDED, RETIRED, MASKED):
            assert not before[i].any() and not acc[i].any() and _same(pfp[i], r.pfp0[i]) and flags[i] == 0 and _same(R_out[i], r.pfp0[i, 18:24])
    live = np.setdiff1d(np.arange(B), [UNSEEDED, RETIRED, MASKED])
    before, acc, pfp, flags, _ = ends[0]
    assert (before[live, 0] == 4).all() and (before[live, 20] == 8).all() and (acc[live, 21] == 2).all() and flags[live].all() and not before[:, [1, 22]].any()
    nan_before, nan_acc, nan_pfp, nan_flags, _ = ends[1]
    assert nan_before[NANPOSE, 1] == 1 and nan_before[NANPOSE, 0] == 3 and nan_before[NANPOSE, 20] == 7 and nan_flags[NANPOSE] == 1
    assert np.isfinite(nan_pfp[NANPOSE]).all()
    rest = np.setdiff1d(np.arange(B), [NANPOSE])
    assert _same(nan_before[rest], before[rest]) and _same(nan_acc[rest], acc[rest]) and _same(nan_pfp[rest], pfp[rest])
    r.close()


# ------------------------------------------------------------------------------------------------ 5. clamps
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_applied_noise_lies_within_the_bounds_and_sits_on_them_where_clamped(dtype):
    B = 100
    r = Run(dtype, 1, 1, False, B, pos=0.2)
    c = r.c
    lo, hi = 0.9 * r.R0, 1.1 * r.R0
    ad = r.adapter(R_lo=lo, R_hi=hi)
    seq = r.pack()
    ad.run(seq)
    acc, R = acc_of(ad), c.ekf.get_filter_params()[:, 18:24]
    assert (acc[:, 21] == 2).all()
    lo_t, hi_t = held(c, lo), held(c, hi)
    assert (R >= lo_t).all() and (R <= hi_t).all()
    assert (R == hi_t).any(), "tag poses 0.2 m off drive the position noise to its upper bound"
    print(f"{dtype}: {int((R == hi_t).sum())} components on R_hi, {int((R == lo_t).sum())} on R_lo of {R.size}")
    seq.close()
    r.close()


# ------------------------------------------------------------------------------------------------ 6. direction
KD, BD, WD = 300, 128, 20
_direction_reference = {}


def _direction_inputs(ekf, scale):
    thm = np.zeros(KD, np.uint8); thm[2::3] = 1
    inputs = ekf.make_inputs(KD, thm)
    ekf.set_filter_params(None)
    ekf.synth_generate(inputs, seed=0xADA97, meas_noise_scale=scale)   # seeds the filters from the generator's first tag pose
    return inputs, [t for t in range(KD) if thm[t]]


def _median_ratio(R_hi_noise, R_lo_noise):
    return np.median(R_hi_noise, axis=0) / np.median(R_lo_noise, axis=0)


@pytest.mark.parametrize("direct", [1, 0])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_estimate_follows_the_noise_of_the_generator(dtype, direct):
    """128 filters at 100 Hz over 300 ticks of synth_generate with a tag pose every third, once with meas_noise_scale 2 and once with
    0.5 (same seed): window 20, gain 1, bounds nominal / 1000 and x 1000.  The ratio of the two runs' batch medians of R_k / R_nominal
    lies in [4, 64] for every k -- the true variance ratio is 16, a factor of four either way.  The reference alone (fp64, computed once
    per method) is held to the same condition; it measured 6.0 .. 40.6 at exactly this shape."""
    kw = dict(update_freq=100.0, direct_orien_method=direct, est_bias=1)
    ekf = qla.BatchedRelativePoseEKF(BD, dtype, params=qla.make_params(**kw))
    po = oracle.make_params(**kw)
    p = ekf_np.Params.from_orc(po)
    R0 = np.array(list(po.R))
    lo, hi = R0 / 1000, R0 * 1000
    got, want = {}, {}
    for scale in (2.0, 0.5):
        inputs, meas = _direction_inputs(ekf, scale)
        x0, P0 = ekf.get_state()
        if direct not in _direction_reference:
            ticks = [inputs.download_tick(t) for t in range(KD)]
            U = np.stack([u for u, _, _ in ticks]); Z = np.stack([ticks[t][1] for t in meas]); M = np.stack([ticks[t][2] for t in meas])
            pfp = np.tile(np.array(adapt.shared_record(ekf)), (BD, 1))
            _, applies = reference_run(po, p, x0, P0, U, Z, M, meas, pfp, WD, 1.0, WD // 2, lo, hi, "f64")
            want[scale] = applies[-1][1] / R0
        out = ekf.adapt_noise(inputs, 0, KD, window=WD, gain=1.0, R_lo=lo, R_hi=hi)
        assert np.isfinite(out["R"]).all() and (out["R"] > 0).all()
        assert (out["windows"] == 5).all() and not out["n_bad"].any() and not out["n_rejected"].any()
        assert _same(out["R"], ekf.get_filter_params()[:, 18:24])
        got[scale] = out["R"] / R0
        inputs.close()
    if want:
        _direction_reference[direct] = _median_ratio(want[2.0], want[0.5])
    for name, ratio in (("reference", _direction_reference[direct]), ("gpu", _median_ratio(got[2.0], got[0.5]))):
        print(f"{dtype} direct={direct} {name}: ratio of the medians of R / R_nominal " + " ".join(f"{v:.1f}" for v in ratio))
        assert (ratio >= 4).all() and (ratio <= 64).all(), (name, ratio)
    ekf.close()


# ------------------------------------------------------------------------------------------------ 7. host-array form
@pytest.mark.parametrize("dtype,est_bias,batch", [("f32", 0, 100), ("f64", 1, 65)])
def test_host_array_form_is_the_adapted_run(dtype, est_bias, batch, monkeypatch):
    layout(monkeypatch, est_bias)
    r = Run(dtype, 1, est_bias, True, batch)
    c = r.c
    seq = r.pack()
    ad = r.adapter()
    ad.run(seq)
    acc, pfp, x, P = end_state(r, ad)
    r.restart()
    out = c.ekf.adapt_noise(seq.inputs, 0, K, window=WINDOW)
    assert _same(np.ascontiguousarray(out["acc"].T), acc) and _same(out["R"], pfp[:, 18:24]) and _same(c.ekf.get_filter_params(), pfp)
    for a, b in zip(c.ekf.get_state(), (x, P)):
        assert _same(a, b)
    np.testing.assert_array_equal(out["windows"], acc[:, 21])
    for t0, n in ((0, K + 1), (K, 1), (-1, 2)):
        with pytest.raises(qla.QleError) as e:
            c.ekf.adapt_noise(seq.inputs, t0, n)
        assert e.value.code == qla._lib.QLE_ERR_INVALID
    seq.close()
    r.close()
