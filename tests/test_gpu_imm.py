"""IMM mixing and mode probabilities on the GPU (DeviceIO.imm, imm.Imm, BatchedRelativePoseEKF.mix_banks; libqle_imm.so: k_imm_mix,
k_imm_update).

The shapes are those of tests/test_gpu_bank.py, each a way the kernel can go wrong: M = 2 with G = 70 banks (B = 140: a ragged last
tile), M = 8 with G = 11 (B = 88: banks beside an unused half tile) and M = 64 with G = 3 (B = 192: one bank per tile).  Truth and how a
deviation is measured: imm_util.py (`mix_ref` / `update_ref`, numpy float64 restatements with plain sums, on the values the handle holds,
pinned on the CPU by tests/test_imm_cpu.py); tolerances: imm_util.TOL, measured on the host-compiled arithmetic and stated in
tests/tolerances_imm.md.  The measured deviations are printed (`pytest -s`, lines `IMM gpu ...`) before anything is asserted.  The other
comparisons are exact equality of bits: which members are mixed, every unmixed record, an identity Pi, isolation, placement, the
host-array form.
"""
import numpy as np
import pytest

import bank_util as bu
import imm_util as iu
import quadrotor_landing_amd as qla
from quadrotor_landing_amd import imm
from test_gpu_bank import Case, host
from test_gpu_devio import assert_same_bits, dev
from util import quat_err

pytestmark = pytest.mark.gpu

GRID = [(M, G, d, r) for M, G in iu.SHAPES for d in ("f32", "f64") for r in iu.RECORDS]
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


def stored(c):
    """(x, P) in the handle's dtype: the stored words"""
    return host(*c.io.state())


def mixer(c, Pi, logmu=None, **kw):
    return c.io.imm(c.M, Pi, logmu0=c.logw if logmu is None else logmu, **kw)


# ------------------------------------------------------------------------------------------------ 1. against the truth
@pytest.mark.parametrize("M,G,dtype,record", GRID, ids=ids(GRID))
def test_mixing_matches_the_truth(M, G, dtype, record, monkeypatch):
    c = Case(M, G, dtype, record, monkeypatch, seed=4000 + M)
    Pi = iu.make_Pi(c.rng, M)
    x, P = c.held()
    x0, P0 = stored(c)
    ref = iu.mix_ref(x, P, c.logw, Pi, c.mask, M)
    assert not ref.mixed[-M:].any() and ref.mixed.sum() >= (G - 1) // 2       # the all-invalid bank; the others mix
    im = mixer(c, Pi)
    logc, mixed = host(*im.mix(dev(c.mask)))
    assert im.logc is not None and logc.dtype == np.float64 and mixed.dtype == np.uint8 and logc.shape == mixed.shape == (c.B,)
    xm, Pm = c.held()
    x1, P1 = stored(c)
    d = iu.deviations(logc, xm, Pm, ref)
    tol = iu.TOL[dtype]
    print(f"IMM gpu M={M} G={G} {dtype} {record}: " + " ".join(f"{k} {v:.2e} ({v / tol[k]:.3f} of {tol[k]:.0e})" for k, v in d.items()))
    np.testing.assert_array_equal(mixed != 0, ref.mixed)                     # exact: which members are mixed, where logc is -inf,
    np.testing.assert_array_equal(np.isneginf(logc), np.isneginf(ref.logc))
    assert_same_bits(x1[~ref.mixed], x0[~ref.mixed], "x of the unmixed records")   # ... and the bits of every unmixed record
    assert_same_bits(P1[~ref.mixed], P0[~ref.mixed], "P of the unmixed records")
    assert np.array_equal(Pm, Pm.transpose(0, 2, 1)) and np.isfinite(xm).all() and np.isfinite(Pm).all()
    assert all(d[k] <= tol[k] for k in d), (d, tol)
    c.close()


# ------------------------------------------------------------------------------------------------ 2. an identity Pi
@pytest.mark.parametrize("M,G,dtype,record", SUBSET, ids=ids(SUBSET))
def test_identity_Pi_is_a_bit_exact_no_op_and_one_launch(M, G, dtype, record, monkeypatch):
    c = Case(M, G, dtype, record, monkeypatch, seed=4100 + M)
    K = imm.imm_lib()
    x0, P0 = stored(c)
    im = mixer(c, np.eye(M))
    mk = dev(c.mask)
    n0 = K.qim_launch_count()
    with qla.launch_census() as ticked:
        logc, mixed = im.mix(mk)
        assert K.qim_launch_count() - n0 == 1
        im.mix()
        assert K.qim_launch_count() - n0 == 2
        im.update(dev(np.zeros(c.B)), mk)
        assert K.qim_launch_count() - n0 == 3
        _torch().cuda.synchronize()
    assert ticked == [], ticked                                              # the tick library launched nothing: its census stays closed
    x1, P1 = stored(c)
    assert_same_bits(x1, x0, "x after mixing under the identity"); assert_same_bits(P1, P0, "P after mixing under the identity")
    logc, mixed = host(logc, mixed)
    assert not mixed.any()
    ref = iu.mix_ref(*c.held(), c.logw, np.eye(M), c.mask, M)
    np.testing.assert_array_equal(np.isneginf(logc), np.isneginf(ref.logc))
    fin = np.isfinite(ref.logc)
    assert fin.any() and bu._rel(np.abs(logc[fin] - ref.logc[fin]), np.abs(ref.logc[fin])) <= iu.TOL[dtype]["logc"]   # the normalised logmu
    c.close()


# ------------------------------------------------------------------------------------------------ 3. isolation
@pytest.mark.parametrize("M,G,dtype,record", SUBSET[:3], ids=ids(SUBSET[:3]))
def test_a_nan_stays_in_its_bank_and_behind_a_zero_of_Pi(M, G, dtype, record, monkeypatch):
    """A NaN planted in the covariance of member s of bank 1 reaches the mixed members j of that bank with Pi[s][j] > 0, no member with
    Pi[s][j] == 0, and no record outside the bank; filters outside the mask keep their bits."""
    c = Case(M, G, dtype, record, monkeypatch, seed=4200 + M, specials=False, empty_bank=False)
    Pi = iu.make_Pi(c.rng, M)
    mask = np.ones(c.B, np.uint8); mask[2 * M:3 * M:2] = 0                   # bank 2: every other member is outside the mask
    s = 1
    x, P = c.x.copy(), c.P.copy()
    P[M + s, 0, 1] = P[M + s, 1, 0] = np.nan
    c.ekf.set_state(x, P)
    x0, P0 = stored(c)
    im = mixer(c, Pi)
    logc, mixed = host(*im.mix(dev(mask)))
    x1, P1 = stored(c)
    ref = iu.mix_ref(x, np.where(np.isnan(P), 0.0, P), c.logw, Pi, mask, M)   # which members are mixed does not depend on P
    np.testing.assert_array_equal(mixed != 0, ref.mixed)
    bank1 = np.arange(M, 2 * M)
    reached = bank1[(Pi[s] > 0) & ref.mixed[bank1]]
    spared = bank1[Pi[s] == 0]                                                # M = 2: s itself, re-initialised from the other member alone
    assert len(reached) and len(spared) == 1 and ref.mixed[spared].all()
    assert np.isnan(P1[reached][:, 0, 1]).all()                               # the NaN arrived where Pi lets it,
    assert np.isfinite(P1[spared]).all() and np.isfinite(x1[spared]).all()    # ... not behind the zero,
    outside = np.ones(c.B, bool); outside[bank1] = False
    assert np.isfinite(P1[outside]).all() and np.isfinite(x1[outside]).all() and not np.isnan(logc[outside]).any()   # ... and in no other bank
    off = mask == 0
    assert_same_bits(x1[off], x0[off], "x outside the mask"); assert_same_bits(P1[off], P0[off], "P outside the mask")
    assert not mixed[off].any() and np.isneginf(logc[off]).all()
    # the same mixing without the NaN: every record outside bank 1 has the same bits
    clean = Case(M, G, dtype, record, monkeypatch, seed=4200 + M, specials=False, empty_bank=False)
    mixer(clean, Pi).mix(dev(mask))
    x2, P2 = stored(clean)
    assert_same_bits(x1[outside], x2[outside], "x of the other banks"); assert_same_bits(P1[outside], P2[outside], "P of the other banks")
    assert_same_bits(x1[spared], x2[spared], "x behind the zero of Pi"); assert_same_bits(P1[spared], P2[spared], "P behind the zero of Pi")
    clean.close(); c.close()


# ------------------------------------------------------------------------------------------------ 4. position independence
@pytest.mark.parametrize("M,G,dtype,record", SUBSET[:3], ids=ids(SUBSET[:3]))
def test_mixing_does_not_depend_on_where_the_bank_sits(M, G, dtype, record, monkeypatch):
    c = Case(M, G, dtype, record, monkeypatch, seed=4300 + M, empty_bank=False)
    Pi = iu.make_Pi(c.rng, M)
    k = G // 2 + 1 if G > 3 else 1                                            # M = 2: 36 banks on, into another lane offset of another tile
    roll = lambda a: np.roll(a.reshape((G, M) + a.shape[1:]), k, axis=0).reshape(a.shape)   # noqa: E731
    twin = qla.BatchedRelativePoseEKF(c.B, dtype, **c.kw)
    twin.set_state(roll(c.x), roll(c.P))
    io2 = qla.DeviceIO(twin)
    la, ma = host(*mixer(c, Pi).mix(dev(c.mask)))
    lb, mb = host(*io2.imm(M, Pi, logmu0=roll(c.logw)).mix(dev(roll(c.mask))))
    xa, Pa = stored(c)
    xb, Pb = host(*io2.state())
    assert ma.any()
    assert_same_bits(xb, roll(xa), "x at another bank index"); assert_same_bits(Pb, roll(Pa), "P at another bank index")
    assert_same_bits(lb, roll(la), "logc at another bank index"); assert_same_bits(mb, roll(ma), "mixed at another bank index")
    io2.close(); twin.close(); c.close()


# ------------------------------------------------------------------------------------------------ 5. the recursion
@pytest.mark.parametrize("M,G", iu.SHAPES, ids=[f"M{M}-G{G}" for M, G in iu.SHAPES])
def test_update_matches_the_truth(M, G, monkeypatch):
    c = Case(M, G, "f32", "full15", monkeypatch, seed=4400 + M, specials=False, empty_bank=False)
    logc, loglik, mask = iu.update_case(c.rng, M, G)
    x0, P0 = stored(c)
    for lo in (np.log(1e-12), -np.inf, -3.0):
        ref, scale = iu.update_ref(logc, loglik, mask, lo, M)
        im = c.io.imm(M, np.eye(M), logmu_min=lo)
        im.logc = dev(logc)
        got = host(im.update(dev(loglik), dev(mask)))[0]
        assert got is not None and host(im.logmu)[0].tobytes() == got.tobytes()
        fin = np.isfinite(ref)
        d = bu._rel(np.abs(got[fin] - ref[fin]), scale[fin])
        print(f"IMM gpu update M={M} logmu_min={lo:.3g}: {d:.2e} ({d / iu.TOL_UPDATE:.3f} of {iu.TOL_UPDATE:.1e})")
        np.testing.assert_array_equal(np.isneginf(got), np.isneginf(ref))
        np.testing.assert_array_equal(got == lo, ref == lo)
        if lo > -np.inf:
            assert (ref == lo).any()                                         # the floor is applied
        else:
            assert np.isneginf(got[np.isneginf(loglik) & (mask != 0) & np.isfinite(logc)]).all()   # -inf leaves -inf
        assert d <= iu.TOL_UPDATE
        mu = host(im.mu())[0].reshape(G, M)
        live = np.isfinite(got).reshape(G, M).any(axis=1)
        assert (np.abs(mu[live].sum(axis=1) - 1.0) < 1e-14).all() and not mu[~live].any()
    x1, P1 = stored(c)
    assert_same_bits(x1, x0, "x after update"); assert_same_bits(P1, P0, "P after update")
    c.close()


# ------------------------------------------------------------------------------------------------ 6. the cycle, end to end
SCALES = (1.0 / 16, 1.0 / 4, 1.0, 4.0)   # of R_r and R_ang, the members of a bank
B_CYCLE, TICKS, EVERY = 128, 12, 3


BLOCKS = (("r", 0), ("v", 3), ("ab", 10), ("wb", 13))   # first word of the vector blocks of x


def block_devs(x, P, xr, Pr, sx, sP):
    """(x, q, P): the groups and relative measures of test 1 -- the worst deviation of a block r, v, ab, wb relative to the block's sum of
    absolute terms sx [B,16], of the quaternion absolutely up to sign, and of a 3 x 3 covariance block relative to the block's sum of
    absolute terms sP [B,n,n]"""
    dx = np.stack([np.abs(x[:, b:b + 3] - xr[:, b:b + 3]).max(axis=1) for _, b in BLOCKS], axis=1)
    bx = np.stack([sx[:, b:b + 3].sum(axis=1) for _, b in BLOCKS], axis=1)
    nb = Pr.shape[1] // 3
    dP = np.abs(P - Pr).reshape(-1, nb, 3, nb, 3).max(axis=(2, 4))
    bP = sP.reshape(-1, nb, 3, nb, 3).sum(axis=(2, 4))
    return bu._rel(dx, bx), float(quat_err(x[:, 6:10], xr[:, 6:10])), bu._rel(dP, bP)


def test_the_cycle_equals_the_cycle_made_of_its_parts():
    """fp64, B = 128, M = 4, 12 ticks with a tag pose every third.  Handle A runs `Imm.step`; handle B the same cycle from parts that have
    tests of their own: get_state -> mix_ref -> set_state, Scorer.observe, DeviceIO.tick, update_ref.  The members differ in R_r / R_ang
    (set_filter_params).  Final states, logmu and the fused estimate agree to the tolerance of test 1 times the number of mixing steps;
    handle B's own logmu moves by more than 100 x that over the run (checked on the numpy side alone), so the comparison cannot pass
    vacuously.

    The groups and relative measures are those of test 1: a block's deviation is taken relative to the block's sum of absolute terms.  In
    test 1 that is |x_j| + sum mu_{i|j} |d_ij|, what the mixing step starts from and what it adds.  A state at the end of the run was
    formed from the initial state by the increments of twelve ticks and four mixing steps, so its sum of absolute terms is |x_0| plus the
    absolute increments of every tick and every mixing step, taken from handle B's own trajectory (get_state after every step, the numpy
    side alone); the covariance likewise; a fused word's is the weighted sum of its members'; logmu is taken relative to |logc| + |loglik|
    + |lse| of its last update (imm_util.update_ref).

    MI355X, the figures of this test against the bound, 4 x the tolerance of test 1: logmu 5.1e-15 of 2.8e-14, x 5.5e-15 of 1.2e-14,
    quaternion 3.2e-16 of 8e-15, covariance 4.2e-15 of 1.2e-14; fused x 4.9e-15, quaternion 2.0e-16, covariance 3.7e-15.  The line
    `IMM gpu cycle blocks` also prints every deviation relative to handle B's FINAL words alone, without the increments, which is NOT
    the convention's scale and is not asserted: r 3.7e-16, v 1.0e-14, ab 1.3e-14, wb 1.1e-14, covariance 1.1e-14, fused x 1.2e-14, fused
    covariance 7.0e-15.  On that scale the accelerometer-bias block reads 1.08 of the bound: an absolute difference of 3.5e-18 in a
    bias whose block sum is 2.7e-4."""
    import oracle
    t = _torch()
    kw = dict(update_freq=400.0, direct_orien_method=0, est_bias=1)
    M, B, R = len(SCALES), B_CYCLE, B_CYCLE // len(SCALES)
    gen = qla.BatchedRelativePoseEKF(R, "f64", params=qla.make_params(**kw))
    thm = np.zeros(TICKS, np.uint8); thm[EVERY - 1::EVERY] = 1
    inputs = gen.make_inputs(TICKS, thm)
    gen.synth_generate(inputs, seed=0x1AA0)
    x0, P0 = gen.get_state()
    ticks = [inputs.download_tick(k) for k in range(TICKS)]
    inputs.close(); gen.close()
    rep = lambda a: np.repeat(a, M, axis=0)   # noqa: E731
    po = oracle.make_params(**kw)
    pfp = np.zeros((B, 24))
    pfp[:, 0:12] = list(po.Q); pfp[:, 12:15] = list(po.ab_static); pfp[:, 15:18] = list(po.wb_static); pfp[:, 18:24] = list(po.R)
    pfp[:, 18:24] *= np.tile(SCALES, R)[:, None]
    rng = np.random.default_rng(46)
    Pi = iu.make_Pi(rng, M) * 0.2 + np.eye(M) * 0.8
    lo = float(np.log(1e-12))
    handles = []
    for _ in range(2):
        ekf = qla.BatchedRelativePoseEKF(B, "f64", params=qla.make_params(**kw))
        ekf.set_state(rep(x0), rep(P0))
        ekf.set_filter_params(pfp)
        handles.append((ekf, qla.DeviceIO(ekf)))
    (ea, ioa), (eb, iob) = handles
    ima = ioa.imm(M, Pi, logmu_min=lo)
    scorer = iob.scorer()
    logmu = np.full(B, -np.log(M))
    first, steps = logmu.copy(), 0
    xb, Pb = eb.get_state()
    sx, sP = np.abs(xb), np.abs(Pb)                                          # handle B's sums of absolute terms: |x_0|, |P_0| ...

    def moved_to(xn, Pn):
        """... plus the absolute increments of a step of handle B"""
        nonlocal xb, Pb, sx, sP
        sx, sP = sx + np.abs(xn - xb), sP + np.abs(Pn - Pb)
        xb, Pb = xn, Pn

    for k, (u, z, mk) in enumerate(ticks):
        u, z, mk = rep(u), rep(z), rep(mk)
        if not thm[k]:
            assert ima.step(dev(u, t.float64)) is None
            iob.tick(dev(u, t.float64))
            moved_to(*eb.get_state())
            continue
        ima.step(dev(u, t.float64), dev(z, t.float64), dev(mk))
        ref = iu.mix_ref(xb, Pb, logmu, Pi, None, M)
        assert ref.mixed.all()
        eb.set_state(ref.x, ref.P)
        moved_to(ref.x, ref.P)
        scorer.reset()
        scorer.observe(dev(u, t.float64), dev(z, t.float64), dev(mk))
        iob.tick(dev(u, t.float64), dev(z, t.float64), dev(mk))
        moved_to(*eb.get_state())
        logmu, scale = iu.update_ref(ref.logc, host(scorer.result().loglik)[0], None, lo, M)
        steps += 1
    assert steps == TICKS // EVERY
    tol = {k: v * steps for k, v in iu.TOL["f64"].items()}
    moved = np.abs(logmu - first).max()
    assert moved > 100 * tol["logc"] and np.ptp(logmu.reshape(R, M), axis=1).min() > 100 * tol["logc"], moved   # the numpy side alone
    la = host(ima.logmu)[0]
    xa, Pa = ea.get_state()
    xfa, Pfa = host(*ima.fuse().state())
    xfb, Pfb = host(*iob.bank(M).fuse(dev(logmu)).state())
    w = bu.fuse_ref(xb, Pb, logmu, None, M).w.reshape(R, M)
    sxf, sPf = (w[:, :, None] * sx.reshape(R, M, 16)).sum(axis=1), (w[:, :, None, None] * sP.reshape(R, M, 15, 15)).sum(axis=1)
    d = {"logmu": bu._rel(np.abs(la - logmu), scale)}
    d["x"], d["q"], d["P"] = block_devs(xa, Pa, xb, Pb, sx, sP)
    d["fused x"], d["fused q"], d["fused P"] = block_devs(xfa, Pfa, xfb, Pfb, sxf, sPf)
    held = {"logmu": tol["logc"], "x": tol["x"], "q": tol["q"], "P": tol["P"], "fused x": tol["x"], "fused q": tol["q"], "fused P": tol["P"]}
    final = block_devs(xa, Pa, xb, Pb, np.abs(xb), np.abs(Pb)), block_devs(xfa, Pfa, xfb, Pfb, np.abs(xfb), np.abs(Pfb))
    per = {n: bu._rel(np.abs(xa[:, k:k + 3] - xb[:, k:k + 3]).max(axis=1), np.abs(xb[:, k:k + 3]).sum(axis=1)) for n, k in BLOCKS}
    mags = {n: float(np.abs(xb[:, k:k + 3]).sum(axis=1).min()) for n, k in BLOCKS}
    print("IMM gpu cycle blocks, relative to the final words alone (not asserted): " + " ".join(f"{n} {v:.2e} (smallest block sum {mags[n]:.2e})" for n, v in per.items())
          + f" P {final[0][2]:.2e} fused x {final[1][0]:.2e} fused P {final[1][2]:.2e}")
    print(f"IMM gpu cycle: logmu moved {moved:.2f}; A against B: " + " ".join(f"{k} {v:.2e} ({v / held[k]:.3f} of {held[k]:.0e})" for k, v in d.items()))
    assert np.isfinite(xa).all() and np.isfinite(Pa).all() and np.isfinite(la).all() and np.isfinite(xfa).all()
    assert all(d[k] <= held[k] for k in d), (d, held)
    for e, io in handles:
        io.close(); e.close()


# ------------------------------------------------------------------------------------------------ 7. the host-array form
@pytest.mark.parametrize("M,G,dtype", [(8, 11, "f32"), (2, 70, "f64")])
def test_host_array_form_has_the_bits_of_the_device_form(M, G, dtype, monkeypatch):
    c = Case(M, G, dtype, "full15", monkeypatch, seed=4600 + M)
    d = Case(M, G, dtype, "full15", monkeypatch, seed=4600 + M)
    Pi = iu.make_Pi(c.rng, M)
    la, ma = host(*mixer(c, Pi).mix(dev(c.mask)))
    lb, mb = d.ekf.mix_banks(M, d.logw, Pi, d.mask)
    assert ma.any() and lb.dtype == np.float64 and mb.dtype == np.uint8
    assert_same_bits(lb, la, "logc: host-array form against the device form"); assert_same_bits(mb, ma, "mixed")
    for got, want, name in zip(stored(d), stored(c), ("x", "P")):
        assert_same_bits(got, want, f"{name}: host-array form against the device form")
    l2, m2 = d.ekf.mix_banks(M, d.logw, np.eye(M).tolist())                  # no mask, a nested list: nothing to mix
    assert not m2.any() and l2.shape == (d.B,)
    for bad in (3, 128):
        with pytest.raises(ValueError):
            d.ekf.mix_banks(bad, d.logw, Pi)
    d.close(); c.close()
