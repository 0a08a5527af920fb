"""Filter banks on the GPU (DeviceIO.bank, bank.Bank.fuse, bank.Fused, BatchedRelativePoseEKF.fuse_banks; libqle_bank.so: k_bank_fuse).

Shapes chosen so that the layout can go wrong: M = 2 with G = 70 banks (B = 140: three ragged input tiles, two output tiles), M = 8 with
G = 11 (B = 88) and M = 64 with G = 3 (B = 192: a bank is a whole tile).  Truth and how a deviation is measured: bank_util.py
(`fuse_ref`, a numpy float64 restatement with plain sums, on the values the handle holds); tolerances: bank_util.TOL, measured and stated
in tests/tolerances_bank.md.  The measured deviations are printed (`pytest -s`, lines `BANK gpu ...`) before anything is asserted.  The
other comparisons are exact equality of bits: one-hot weights, isolation of banks, placement, the handle unchanged, the consumers, the
host-array form.

One-hot weights and the sign of zero: a fused word is x_ref + m (or 1 * (P + 0 * 0)) formed in IEEE arithmetic, so a stored -0.0 comes
back as +0.0 -- the same value.  `same_words` therefore asks for equal bits except where both words are zero.
"""
import numpy as np
import pytest

import bank_util as bu
import lookahead_util as lu
import quadrotor_landing_amd as qla
from quadrotor_landing_amd import bank, health
from test_gpu_devio import assert_same_bits, bits, dev, rand_imu

pytestmark = pytest.mark.gpu

SHAPES = [(2, 70), (8, 11), (64, 3)]
MR = dict(multirate_ekf=1, measurement_delay=3 / 400.0)
GRID = [(M, G, d, r) for M, G in SHAPES for d in ("f32", "f64") for r in bu.RECORDS]
SUBSET = [(2, 70, "f64", "compact9"), (8, 11, "f32", "full15"), (64, 3, "f64", "full9"), (64, 3, "f32", "full15")]
ids = lambda grid: [f"M{M}-G{G}-{d}-{r}" for M, G, d, r in grid]   # noqa: E731


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


def same_words(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    same = (bits(a) == bits(b)) | ((a == 0) & (b == 0))
    assert same.all(), f"{what}: {int((~same).sum())} of {same.size} words differ, first at {np.argwhere(~same)[0]}"


class Case:
    """A handle of G banks of M members after a few predict ticks from util.rand_states, with the special members of
    bank_util.make_case applied to what the ticks left (specials=True), and the log-weights and the mask that go with them."""

    def __init__(self, M, G, dtype, record, monkeypatch, seed, specials=True, empty_bank=True, **kw):
        self.M, self.G, self.B, self.dtype = M, G, M * G, dtype
        self.n, compact = bu.RECORDS[record]
        monkeypatch.setenv("QLE_COMPACT", "1" if compact else "0")   # read at handle creation, as tests/test_gpu_compact.py sets it
        monkeypatch.setenv("QLE_QUAD", "0")
        self.kw = dict(lu.KW, est_bias=int(self.n == 15), **kw)
        rng = self.rng = np.random.default_rng(seed)
        ekf = self.ekf = qla.BatchedRelativePoseEKF(self.B, dtype, **self.kw)
        assert ekf.num_states == self.n and ekf.policy()["record_words"] == (64 if compact else 136)
        x0, P0, _, _ = bu.make_case(rng, M, G, self.n, dtype, specials=False, empty_bank=False)
        ekf.set_state(x0, P0)
        for _ in range(3):
            ekf.predict(rand_imu(rng, self.B))
        xg, Pg = ekf.get_state()
        self.x, self.P, self.logw, self.mask = bu.make_case(rng, M, G, self.n, dtype, x=xg, P=Pg, specials=specials, empty_bank=empty_bank)
        ekf.set_state(self.x, self.P)
        self.io = qla.DeviceIO(ekf)

    def held(self):
        """(x, P) as the handle holds them, in double"""
        return host(*self.io.state(dtype="float64"))

    def fuse(self, logw=None, mask="case"):
        mask = self.mask if isinstance(mask, str) else mask
        return self.io.bank(self.M).fuse(dev(self.logw if logw is None else logw), None if mask is None else dev(mask))

    def close(self):
        self.io.close()
        self.ekf.close()


# ------------------------------------------------------------------------------------------------ 1. against the truth
@pytest.mark.parametrize("M,G,dtype,record", GRID, ids=ids(GRID))
def test_fused_estimate_matches_the_truth(M, G, dtype, record, monkeypatch):
    c = Case(M, G, dtype, record, monkeypatch, seed=2000 + M)
    x, P = c.held()
    ref = bu.fuse_ref(x, P, c.logw, c.mask, M)
    assert ref.best[-1] == -1 and (ref.best[:-1] >= 0).all()
    f = c.fuse()
    assert (f.members, f.banks) == (M, G) and tuple(f.w.shape) == (c.B,) and tuple(f.best.shape) == (G,)
    xf, Pf = host(*f.state(dtype="float64"))
    w, best = host(f.w, f.best)
    assert xf.shape == (G, 16) and Pf.shape == (G, c.n, c.n) and w.dtype == np.float64 and best.dtype == np.int32
    dev_ = bu.deviations(w, xf, Pf, ref)
    tol = bu.TOL[dtype]
    print(f"BANK gpu M={M} G={G} {dtype} {record}: " + " ".join(f"{k} {v:.2e} ({v / tol[k]:.3f} of {tol[k]:.0e})" for k, v in dev_.items()))
    np.testing.assert_array_equal(best, ref.best)                            # exact: best, the zero weights, the empty bank's record
    np.testing.assert_array_equal(w == 0, ref.w == 0)
    assert not xf[-1].any() and not Pf[-1].any() and not w[-M:].any()
    assert np.array_equal(Pf, Pf.transpose(0, 2, 1)) and np.isfinite(xf).all() and np.isfinite(Pf).all()
    assert all(dev_[k] <= tol[k] for k in dev_), (dev_, tol)
    for g in range(G - 1):
        assert abs(w[g * M:(g + 1) * M].sum() - 1.0) < 4e-16
    c.close()


# ------------------------------------------------------------------------------------------------ 2. one-hot weights
@pytest.mark.parametrize("M,G,dtype,record", SUBSET, ids=ids(SUBSET))
def test_one_hot_weights_return_the_member(M, G, dtype, record, monkeypatch):
    c = Case(M, G, dtype, record, monkeypatch, seed=2100 + M, specials=False, empty_bank=False)
    pick = np.arange(G) * M + c.rng.integers(M, size=G)
    logw = np.full(c.B, -np.inf); logw[pick] = 0.0
    f = c.fuse(logw, mask=None)
    x, P = host(*c.io.state())                                               # the handle's dtype: the stored words
    xf, Pf = host(*f.state())
    w, best = host(f.w, f.best)
    np.testing.assert_array_equal(best, pick)
    want = np.zeros(c.B); want[pick] = 1.0
    np.testing.assert_array_equal(w, want)
    keep = [k for k in range(16) if not 6 <= k < 10]
    same_words(xf[:, keep], x[pick][:, keep], "r, v and the biases")
    same_words(Pf, P[pick], "every covariance word")
    q, qr = xf[:, 6:10].astype(np.float64), x[pick, 6:10].astype(np.float64)
    dq = np.minimum(np.abs(q - qr).max(axis=1), np.abs(q + qr).max(axis=1)).max()
    print(f"BANK gpu one-hot M={M} {dtype} {record}: q {dq:.2e}")
    assert dq <= bu.TOL[dtype]["q"]
    c.close()


# ------------------------------------------------------------------------------------------------ 3. isolation and placement
@pytest.mark.parametrize("M,G,dtype,record", SUBSET[:3], ids=ids(SUBSET[:3]))
def test_banks_are_isolated_and_do_not_depend_on_their_place(M, G, dtype, record, monkeypatch):
    c = Case(M, G, dtype, record, monkeypatch, seed=2200 + M, empty_bank=False)
    f0 = c.fuse()
    x0, P0, w0, b0 = host(*f0.state(), f0.w, f0.best)
    # (a) every member of the odd banks becomes NaN or Inf with a huge log-weight: the even banks keep their bits
    odd = (np.arange(c.B) // M) % 2 == 1
    x1, P1, logw1 = c.x.copy(), c.P.copy(), c.logw.copy()
    x1[odd] = np.where(np.arange(c.B)[odd, None] % 2 == 0, np.nan, np.inf)
    P1[odd] = np.nan
    logw1[odd] = 1e300
    mask1 = c.mask.copy(); mask1[odd] = 1
    c.ekf.set_state(x1, P1)
    f1 = c.fuse(logw1, mask1)
    xa, Pa, wa, ba = host(*f1.state(), f1.w, f1.best)
    even_g, even_i = np.arange(G) % 2 == 0, ~odd
    assert_same_bits(xa[even_g], x0[even_g], "x of the even banks"); assert_same_bits(Pa[even_g], P0[even_g], "P of the even banks")
    assert_same_bits(wa[even_i], w0[even_i], "w of the even banks"); assert_same_bits(ba[even_g], b0[even_g], "best of the even banks")
    assert not np.isfinite(xa[~even_g][:, :6]).any()                          # the non-finite words reached their own bank's record ...
    status, _ = host(*f1.health())
    assert (status[~even_g] & health.NONFINITE).all() and not (status[even_g] & health.NONFINITE).any()   # ... where health() flags them
    # (b) the same members at another bank index of another handle: the same bits
    k = G // 2 + 1 if G > 3 else 1                                            # M = 2: 36 banks on, into the other tiles
    roll = lambda a: np.roll(a.reshape((G, M) + a.shape[1:]), k, axis=0).reshape(a.shape)   # noqa: E731
    twin = qla.BatchedRelativePoseEKF(c.B, dtype, **c.kw)
    twin.set_state(roll(c.x), roll(c.P))
    io2 = qla.DeviceIO(twin)
    f2 = io2.bank(M).fuse(dev(roll(c.logw)), dev(roll(c.mask)))
    xb, Pb, wb, bb = host(*f2.state(), f2.w, f2.best)
    assert_same_bits(xb, np.roll(x0, k, axis=0), "x at another bank index"); assert_same_bits(Pb, np.roll(P0, k, axis=0), "P at another bank index")
    assert_same_bits(wb, roll(w0), "w at another bank index")
    moved = np.roll(b0, k)
    moved = np.where(moved >= 0, (moved + k * M) % c.B, -1).astype(np.int32)
    assert_same_bits(bb, moved, "best at another bank index")
    io2.close(); twin.close(); c.close()


# ------------------------------------------------------------------------------------------------ 4. read-only, one launch
@pytest.mark.parametrize("M,G,dtype,record", SUBSET[1:3], ids=ids(SUBSET[1:3]))
def test_fuse_is_read_only_and_one_launch(M, G, dtype, record, monkeypatch):
    c = Case(M, G, dtype, record, monkeypatch, seed=2300 + M)
    K = bank.bank_lib()
    x0, P0 = host(*c.io.state())
    rep0 = host(*c.io.report().values())
    lw, mk = dev(c.logw), dev(c.mask)
    b = c.io.bank(M)
    n0 = K.qbk_launch_count()
    with qla.launch_census() as ticked:
        f = b.fuse(lw, mk)
        assert K.qbk_launch_count() - n0 == 1
        g = b.fuse(lw)
        assert K.qbk_launch_count() - n0 == 2
        _torch().cuda.synchronize()
    assert ticked == [], ticked                                              # the tick library launched nothing: its census stays closed
    x1, P1 = host(*c.io.state())
    assert_same_bits(x1, x0, "x after fuse"); assert_same_bits(P1, P0, "P after fuse")
    for r0, r1, name in zip(rep0, host(*c.io.report().values()), ("pose", "pose_cov", "vel", "bias")):
        assert_same_bits(r1, r0, f"report {name} after fuse")
    assert f.view.state != c.io._view().state and f.view.batch == G and f.view.padded_batch == -(-G // 64) * 64 and not f.view.filter_params
    assert f.workspace.data_ptr() != g.workspace.data_ptr()
    c.close()


# ------------------------------------------------------------------------------------------------ 5. the consumers
@pytest.mark.parametrize("M,G,dtype,record", [SUBSET[0], SUBSET[3]], ids=ids([SUBSET[0], SUBSET[3]]))
def test_consumers_read_the_fused_view(M, G, dtype, record, monkeypatch):
    c = Case(M, G, dtype, record, monkeypatch, seed=2400 + M)
    f = c.fuse()
    xf, Pf = host(*f.state(dtype="float64"))
    # report(): the existing definition, run by a handle of G filters that holds the fused state
    plain = qla.BatchedRelativePoseEKF(G, dtype, **c.kw)
    plain.set_state(xf, Pf)
    iop = qla.DeviceIO(plain)
    assert_same_bits(host(*iop.state())[0], host(*f.state())[0], "the fused state, held by a handle")
    for (name, got), want in zip(f.report().items(), iop.report().values()):
        assert tuple(got.shape)[0] == G
        assert_same_bits(*host(got, want), f"report {name}")
    # health(): no finite member, no covariance that is not positive definite; the empty bank is uninitialised
    status, flagged, summary = host(*f.health(return_summary=True))
    assert status.shape == (G,) and not (status & (health.NOT_PD | health.NONFINITE)).any()
    s = dict(zip(health.SUMMARY_FIELDS, summary))
    assert s["uninitialised"] == 1 and s["evaluated"] == G - 1 and s["n_not_pd"] == 0 and status[-1] == 0
    # nees(): runs against a truth [G,16]
    xt = xf.copy(); xt[:, 0:3] += 0.01
    nees, summ = host(*f.nees(dev(xt)))
    assert nees.shape == (G,) and np.isfinite(nees[:-1]).all() and (nees[:-1] > 0).all() and np.isnan(nees[-1])
    assert summ[0] == G - 1
    with pytest.raises(ValueError):
        f.nees(dev(np.zeros((c.B, 16))))                                      # a truth per member is not what a fused view takes
    assert not hasattr(f, "lookahead")
    iop.close(); plain.close(); c.close()


# ------------------------------------------------------------------------------------------------ 6. with the scorer
SCALES = (1.0 / 16, 1.0 / 4, 1.0, 4.0)   # of R_r, the members of a bank
REPLICAS, KS = 16, 24
MEAS = list(range(2, KS, 3))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_scorer_weights_choose_the_member_of_the_largest_likelihood(dtype):
    """4 scalings of R_r x 16 replicas, laid out as 16 banks of 4: the members of a bank start from one state and are fed identical
    inputs (the generator's, for 16 filters), and differ in R_r alone."""
    import oracle
    kw = dict(update_freq=400.0, direct_orien_method=0, est_bias=1)
    M, B = len(SCALES), len(SCALES) * REPLICAS
    gen = qla.BatchedRelativePoseEKF(REPLICAS, dtype, params=qla.make_params(**kw))
    thm = np.zeros(KS, np.uint8); thm[MEAS] = 1
    inputs = gen.make_inputs(KS, thm)
    gen.synth_generate(inputs, seed=0x5C0DE)
    x0, P0 = gen.get_state()
    ticks = [inputs.download_tick(t) for t in range(KS)]
    rep = lambda a: np.repeat(a, M, axis=1)   # noqa: E731
    U, Z, Mk = rep(np.stack([u for u, _, _ in ticks])), rep(np.stack([ticks[t][1] for t in MEAS])), rep(np.stack([ticks[t][2] for t in MEAS]))
    inputs.close(); gen.close()
    po = oracle.make_params(**kw)
    pfp = np.zeros((B, 24))
    pfp[:, 0:12] = list(po.Q); pfp[:, 12:15] = list(po.ab_static); pfp[:, 15:18] = list(po.wb_static); pfp[:, 18:24] = list(po.R)
    pfp[:, 18:21] *= np.tile(SCALES, REPLICAS)[:, None]
    ekf = qla.BatchedRelativePoseEKF(B, dtype, params=qla.make_params(**kw))
    ekf.set_state(np.repeat(x0, M, axis=0), np.repeat(P0, M, axis=0))
    ekf.set_filter_params(pfp)
    io = qla.DeviceIO(ekf)
    t = _torch()
    td = t.float32 if dtype == "f32" else t.float64
    seq = io.sequence(dev(U, td), dev(Z, td), MEAS, dev(Mk))
    sc = io.scorer()
    sc.run(seq)
    f = io.bank(M).fuse(sc)
    loglik, w, best = host(sc.result().loglik, f.w, f.best)
    assert np.isfinite(loglik).all()
    np.testing.assert_array_equal(best, np.arange(REPLICAS) * M + loglik.reshape(REPLICAS, M).argmax(axis=1))
    assert (np.abs(w.reshape(REPLICAS, M).sum(axis=1) - 1.0) < 4e-16).all() and (w >= 0).all()
    ref = bu.fuse_ref(*host(*io.state(dtype="float64")), loglik, None, M)
    assert (np.abs(w - ref.w) <= bu.TOL[dtype]["w"] * ref.w).all()
    xf, _ = host(*f.state())
    assert np.isfinite(xf).all()
    seq.close(); io.close(); ekf.close()


# ------------------------------------------------------------------------------------------------ 7. the host-array form
@pytest.mark.parametrize("M,G,dtype", [(8, 11, "f32"), (2, 70, "f64")])
def test_host_array_form_has_the_bits_of_the_device_form_on_a_multirate_handle(M, G, dtype, monkeypatch):
    c = Case(M, G, dtype, "full15", monkeypatch, seed=2600 + M, **MR)
    assert c.ekf.params.multirate_ekf
    f = c.fuse()
    xd, Pd, wd, bd = host(*f.state(dtype="float64"), f.w, f.best)
    xh, Ph, wh, bh = c.ekf.fuse_banks(M, c.logw, c.mask)
    for got, want, name in ((xh, xd, "x"), (Ph, Pd, "P"), (wh, wd, "w"), (bh, bd, "best")):
        assert_same_bits(got, want, f"{name}: host-array form against the device form")
    x2, P2, w2, b2 = c.ekf.fuse_banks(M, c.logw)                              # no mask: all
    f2 = c.fuse(mask=None)
    assert_same_bits(x2, host(*f2.state(dtype="float64"))[0], "x without a mask"); assert_same_bits(w2, host(f2.w)[0], "w without a mask")
    for bad in (3, 128):
        with pytest.raises(ValueError):
            c.ekf.fuse_banks(bad, c.logw)
    c.close()
