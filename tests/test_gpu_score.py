"""Innovation scoring on the GPU (include/qle_score.h, libqle_score.so: k_score, k_score_tiles, k_score_reduce; DeviceIO.scorer(),
BatchedRelativePoseEKF.score).

Reference: score_util.reference_run -- per tag tick the dense oracle's prediction_step followed by the numpy restatement of the innovation
(gate_util.predict_then_innovation), numpy's slogdet, plain fp64 sums -- stepped by oracle.run_batch from the same start.  In fp32 the
free-running state drifts from the oracle over 24 ticks, so there the reference is teacher-forced: in front of every tag tick it takes the
state the GPU holds.  Counts are exact; the sums are held to score_util.TOL["gpu"], measured and stated in tests/tolerances_score.md.
Batches of 100 (a ragged second tile) and 65; K = 24 ticks with a tag slot every third: 8 tag ticks, 7 lag pairs.
"""
import numpy as np
import pytest

import oracle
import quadrotor_landing_amd as qla
from oracle import ekf_np
from quadrotor_landing_amd import score
from score_util import COUNTS, PREV, TOL, deviations, loglik, make_sequence, reference_run
from test_gpu_innovation import Case, _same, grid

pytestmark = pytest.mark.gpu

K = 24
MEAS = list(range(2, K, 3))   # 8 tag ticks


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


def acc_of(scorer):
    """the accumulators as the reference holds them: [B, 40] on the host"""
    _torch().cuda.synchronize()
    return np.ascontiguousarray(scorer.acc.cpu().numpy()[:, :scorer.io.ekf.batch].T)


class Run:
    """A handle, K ticks of inputs built around the oracle's own run, and the packed sequence."""

    def __init__(self, dtype, direct, est_bias, use_pfp, batch, mask=None):
        c = self.c = Case(dtype, direct, est_bias, use_pfp, batch=batch, cov_scale=0.05)
        self.x0, self.P0 = c.ekf.get_state()
        U, Z = make_sequence(c.rng, c.po, self.x0, self.P0, K, MEAS, c.pfp)
        self.U, self.Z = held(c, U), held(c, Z)
        self.M = np.ones((len(MEAS), batch), np.uint8) if mask is None else mask
        self.io = qla.DeviceIO(c.ekf)

    def pack(self, Z=None, M=None):
        c = self.c
        return self.io.sequence(dev(c, self.U), dev(c, self.Z if Z is None else Z), MEAS, dev(c, self.M if M is None else M))

    def restart(self, x=None, P=None):
        self.c.ekf.set_state(self.x0 if x is None else x, self.P0 if P is None else P)

    def close(self):
        self.io.close()
        self.c.close()


def layout(monkeypatch, est_bias):
    """est_bias = 0 runs on compact records (forced, as test_gpu_adapt.layout does: by default these small batches keep full records for
    the workgroup-cooperative kernel, which est_bias = 1 runs on), so that both layouts' instantiations of k_score are held here; the
    9-state full records are a row of tests/side_variant_table.py"""
    if not est_bias:
        monkeypatch.setenv("QLE_COMPACT", "1")


# ------------------------------------------------------------------------------------------------ 1. configuration matrix
@pytest.mark.parametrize("batch", [100, 65])
@grid
def test_scored_run_matches_the_tick_loop_and_the_reference(dtype, direct, est_bias, use_pfp, batch, monkeypatch):
    layout(monkeypatch, est_bias)
    r = Run(dtype, direct, est_bias, use_pfp, batch)
    c, io = r.c, r.io
    assert bool(io._view().compact) == (est_bias == 0)
    seq = r.pack()
    # (a) one native call
    whole = io.scorer()
    whole.run(seq)
    acc = acc_of(whole)
    # (b) the same ticks as observe + tick from Python
    r.restart()
    loop = io.scorer()
    j = 0
    for t in range(K):
        u = dev(c, r.U[t])
        if t in MEAS:
            z, m = dev(c, r.Z[j]), dev(c, r.M[j])
            loop.observe(u, z, m)
            io.tick(u, z, m)
            j += 1
        else:
            io.tick(u)
    assert _same(acc_of(loop), acc)
    # (c) in pieces, with the state the GPU holds in front of every tag tick: bit for bit the one call, and the teacher of the fp32 reference
    r.restart()
    pieces = io.scorer()
    forced, t0 = {}, 0
    for t in MEAS:
        pieces.run(seq, t0, t - t0)
        forced[t] = c.ekf.get_state()
        t0 = t
    pieces.run(seq, t0)
    assert _same(acc_of(pieces), acc)
    ref = reference_run(c.po, c.p, r.x0, r.P0, r.U, r.Z, r.M, MEAS, c.pfp, forced=forced if dtype == "f32" else None)
    np.testing.assert_array_equal(acc[:, COUNTS], ref.acc[:, COUNTS])
    assert (acc[:, 0] == 8).all() and (acc[:, 5] == 7).all() and not acc[:, 4].any() and not acc[:, 36:].any()
    d = deviations(acc, ref)
    print(f"{dtype} direct={direct} bias={est_bias} pfp={use_pfp} B={batch}: " + " ".join(f"{g} {v:.2e}" for g, v in d.items()))
    tol = TOL["gpu"][dtype]
    assert all(d[g] < tol[g] for g in d), (d, tol)
    assert np.abs(acc[:, PREV] - ref.acc[:, PREV]).max() <= tol["nu"] * np.abs(ref.acc[:, PREV]).max()
    # result(): the statistics of the words
    _torch().cuda.synchronize()
    s = whole.result()
    np.testing.assert_allclose(s.loglik.cpu().numpy(), loglik(acc), rtol=1e-13)
    np.testing.assert_array_equal(s.n.cpu().numpy(), acc[:, 0])
    np.testing.assert_allclose(s.var_ratio.cpu().numpy(), acc[:, 12:18] / acc[:, 18:24], rtol=1e-15)
    np.testing.assert_allclose(s.rho1.cpu().numpy(), acc[:, 24:30] / acc[:, 12:18], rtol=1e-15)
    assert tuple(s.nu_mean.shape) == (batch, 6) and tuple(s.nis_mean.shape) == (batch,)
    seq.close()
    r.close()


# ------------------------------------------------------------------------------------------------ 2. state untouched
@pytest.mark.parametrize("dtype,est_bias,batch", [("f32", 1, 65), ("f64", 0, 100)])
def test_scored_run_leaves_the_bits_of_the_plain_run(dtype, est_bias, batch, monkeypatch):
    layout(monkeypatch, est_bias)
    rng = np.random.default_rng(3)
    r = Run(dtype, 1, est_bias, True, batch, mask=(rng.uniform(size=(len(MEAS), batch)) < 0.8).astype(np.uint8))
    c, io = r.c, r.io
    assert bool(io._view().compact) == (est_bias == 0)
    seq = r.pack()
    io.run(seq)
    x1, P1 = c.ekf.get_state()
    ticks1 = [seq.inputs.download_tick(t) for t in MEAS]
    r.restart()
    Q = score.score_lib()
    n0 = Q.qsc_launch_count()
    sc = io.scorer()
    sc.run(seq)
    assert Q.qsc_launch_count() - n0 == len(MEAS)
    x2, P2 = c.ekf.get_state()
    assert _same(x1, x2) and _same(P1, P2)
    for j, t in enumerate(MEAS):   # the records of the tag ticks, mask words included, are what the plain run left
        for a, b in zip(seq.inputs.download_tick(t), ticks1[j]):
            assert _same(a, b)
        assert np.array_equal(ticks1[j][2] != 0, r.M[j] != 0)
    np.testing.assert_array_equal(acc_of(sc)[:, 0], r.M.sum(axis=0))
    # the host-array form: the same accumulators from the same start, and a window outside the sequence is refused
    r.restart()
    out = c.ekf.score(seq.inputs, 0, K)
    assert _same(np.ascontiguousarray(out["acc"].T), acc_of(sc))
    x3, P3 = c.ekf.get_state()
    assert _same(x1, x3) and _same(P1, P3)
    for t0, n in ((0, K + 1), (K, 1), (-1, 2)):
        with pytest.raises(qla.QleError) as e:
            c.ekf.score(seq.inputs, t0, n)
        assert e.value.code == qla._lib.QLE_ERR_INVALID
    with pytest.raises(ValueError):
        sc.run(seq, 3, K)
    seq.close()
    r.close()


# ------------------------------------------------------------------------------------------------ 3. bookkeeping
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_bookkeeping_of_filters_that_are_off_gapped_or_unscorable(dtype):
    B = 100
    UNSEEDED, RETIRED, GAPPED, NANPOSE = 3, 70, 64, 99
    r = Run(dtype, 1, 1, False, B)
    c, io = r.c, r.io
    x0 = r.x0.copy(); x0[UNSEEDED] = 0.0
    M = r.M.copy(); M[2, GAPPED] = M[5, GAPPED] = 0
    Z = r.Z.copy(); Z[7, NANPOSE, 1] = np.nan   # on the last tag tick: the tick behind it takes the pose in, nothing is scored after it
    seq = r.pack(Z, M)
    r.restart(x0)
    retire = np.zeros(B, np.uint8); retire[RETIRED] = 1
    io.retire(dev(c, retire))
    sc = io.scorer()
    forced, t0 = {}, 0
    for t in MEAS:
        sc.run(seq, t0, t - t0)
        forced[t] = c.ekf.get_state()
        t0 = t
    sc.run(seq, t0)
    acc = acc_of(sc)
    assert not acc[UNSEEDED].any() and not acc[RETIRED].any()
    assert acc[GAPPED, 0] == 6 and acc[GAPPED, 5] == 5 and acc[GAPPED, 4] == 0
    assert acc[NANPOSE, 0] == 7 and acc[NANPOSE, 4] == 1 and acc[NANPOSE, 5] == 6
    rest = np.setdiff1d(np.arange(B), [UNSEEDED, RETIRED, GAPPED, NANPOSE])
    assert (acc[rest, 0] == 8).all() and (acc[rest, 5] == 7).all() and not acc[rest, 4].any()
    # every sum is the reference's, which leaves those filters and ticks out
    Mref = M.copy(); Mref[:, [UNSEEDED, RETIRED]] = 0
    ref = reference_run(c.po, c.p, x0, r.P0, r.U, Z, Mref, MEAS, None, forced=forced if dtype == "f32" else None)
    live = np.setdiff1d(np.arange(B), [UNSEEDED, RETIRED])
    np.testing.assert_array_equal(acc[live][:, COUNTS], ref.acc[live][:, COUNTS])
    ref.acc, ref.scale, acc = ref.acc[live], ref.scale[live], acc[live]
    d = deviations(acc, ref)
    print(f"{dtype} bookkeeping: " + " ".join(f"{g} {v:.2e}" for g, v in d.items()))
    tol = TOL["gpu"][dtype]
    assert all(d[g] < tol[g] for g in d), (d, tol)
    seq.close()
    r.close()


# ------------------------------------------------------------------------------------------------ 4. summary
@pytest.mark.parametrize("dtype,batch", [("f32", 100), ("f64", 65)])
def test_summary_is_deterministic_and_the_sum_of_the_filters(dtype, batch):
    t = _torch()
    rng = np.random.default_rng(9)
    r = Run(dtype, 0, 1, False, batch, mask=(rng.uniform(size=(len(MEAS), batch)) < 0.7).astype(np.uint8))
    c, io = r.c, r.io
    seq = r.pack()
    sc = io.scorer()
    sc.run(seq)
    s1, s2 = sc.summary(), sc.summary()
    t.cuda.synchronize()
    s1, s2 = s1.cpu().numpy(), s2.cpu().numpy()
    assert s1.shape == (30,) and _same(s1, s2)
    acc = acc_of(sc)

    def check(s, rows):
        want, scale = acc[rows][:, :30].sum(axis=0), np.abs(acc[rows][:, :30]).sum(axis=0)
        assert (np.abs(s - want) <= 1e-12 * scale).all(), (s, want)
        assert s[0] == acc[rows, 0].sum() and s[4] == 0 and s[5] == acc[rows, 5].sum()

    check(s1, np.arange(batch))
    pick = rng.uniform(size=batch) < 0.5
    sm = sc.summary(dev(c, pick.astype(np.uint8)))
    t.cuda.synchronize()
    check(sm.cpu().numpy(), np.flatnonzero(pick))
    assert sm.cpu().numpy()[0] < s1[0]
    sc.reset()
    assert not acc_of(sc).any()
    seq.close()
    r.close()


# ------------------------------------------------------------------------------------------------ 5. the purpose: ranking a sweep
SCALES = (1.0 / 16, 1.0 / 4, 1.0, 4.0)   # of R_r; the generator draws its tag-pose noise from the handle's R: scale 1
KS, BURN, REPLICAS = 192, 96, 16


def _nearness(var_ratio):
    """distance from 1 of a group's var_ratio[:, :3]: the largest |log| of its mean over the replicas"""
    return float(np.abs(np.log(var_ratio[:, :3].mean(axis=0))).max())


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_sweep_over_position_noise_ranks_the_generators_first(dtype):
    """4 scalings of R_r x 16 replicas from synth_generate: the same 16 generated filters (same seed, same global indices) run once per
    scaling, so that the groups differ in R_r alone.  The mean log-likelihood is highest, and var_ratio[:, :3] nearest to 1, for scale 1.

    What the CPU reference alone says decides the size and the configuration (profiles of the reference, 16 replicas, seed as below):
    at the issue's K = 24 from the seeding tag pose it ranks nothing right -- the prior (cov_init) is one to two orders of magnitude wider
    than the seeding error, and the first innovations measure that, not R.  With the conventional orientation method, K lengthened to 192
    and the first 96 ticks run unscored (the filter has converged from its prior), the reference gives mean loglik 169.8 for scale 1
    against 144.3 (1/4), 144.6 (4) and -22.1 (1/16), and nearness 0.90 against 1.14, 1.67, 2.16.  With the direct orientation method
    the reference puts scale 4 first on loglik at every length tried (24 .. 480 ticks, with and without the unscored start, IMU noise
    and true biases on or off; the gap grows with the length): at scale 1 its mean NIS is 10.6 per tag pose where a consistent filter has
    6, while the per-component var_ratio is 0.93 .. 1.06 -- the cross terms of the direct method's R_k are not those of the generator's
    noise, which is independent per component in the measurement frame.  That is a property of the reference's model and of the
    generator, not of the scoring; the sweep here therefore runs the conventional method."""
    kw = dict(update_freq=400.0, direct_orien_method=0, est_bias=1)
    ekf = qla.BatchedRelativePoseEKF(REPLICAS, dtype, params=qla.make_params(**kw))
    po = oracle.make_params(**kw)
    p = ekf_np.Params.from_orc(po)
    thm = np.zeros(KS, np.uint8); thm[2::3] = 1
    meas = [t for t in range(KS) if thm[t]]
    inputs = ekf.make_inputs(KS, thm)
    base = np.zeros((REPLICAS, 24))
    base[:, 0:12] = list(po.Q); base[:, 12:15] = list(po.ab_static); base[:, 15:18] = list(po.wb_static); base[:, 18:24] = list(po.R)
    got, want = {}, {}
    U = Z = M = None
    for sc in SCALES:
        ekf.set_filter_params(None)
        ekf.synth_generate(inputs, seed=0x5C0DE)   # the same data every time; seeds the filters from the generator's first tag pose
        pfp = base.copy(); pfp[:, 18:21] *= sc
        ekf.set_filter_params(pfp)
        pfp = ekf.get_filter_params()
        x0, P0 = ekf.get_state()
        if U is None:
            ticks = [inputs.download_tick(t) for t in range(KS)]
            U = np.stack([u for u, _, _ in ticks]); Z = np.stack([ticks[t][1] for t in meas]); M = np.stack([ticks[t][2] for t in meas])
        ekf.run(inputs, 0, BURN)
        out = ekf.score(inputs, BURN, KS - BURN)
        assert (out["n"] == len([t for t in meas if t >= BURN])).all() and not out["n_bad"].any()
        got[sc] = (float(out["loglik"].mean()), _nearness(out["var_ratio"]))
        if dtype == "f64":
            ref = reference_run(po, p, x0, P0, U, Z, M, meas, pfp, score_from=BURN)
            want[sc] = (float(loglik(ref.acc).mean()), _nearness(ref.acc[:, 12:18] / ref.acc[:, 18:24]))
    for name, table in (("reference", want), ("gpu", got)):
        if not table:
            continue
        print(f"{dtype} {name}: " + "  ".join(f"x{sc:g}: loglik {ll:.1f} nearness {nr:.2f}" for sc, (ll, nr) in table.items()))
        assert max(table, key=lambda s: table[s][0]) == 1.0, (name, table)
        assert min(table, key=lambda s: table[s][1]) == 1.0, (name, table)
    inputs.close()
    ekf.close()
