"""Filter consistency against a truth on the GPU (include/qle_consistency.h, libqle_consistency.so: k_nees, k_nees_reduce;
DeviceIO.nees, BatchedRelativePoseEKF.nees / synth_nees).

Reference and tolerance: consistency_util.py -- float64 numpy on get_state() and on the truth as the compute dtype holds it,
`np.linalg.solve` on the sliced marginal, |nees - ref| <= 16 n kappa(C_i) u ref per filter, err to 8 u of its block's norm (the attitude
block to 8 u pi).  Everything the kernels decide rather than compute (off filters, counts, the read-only property, determinism, the two
entry points) is compared exactly.  Shapes: B = 197 (four tiles, ragged end), B = 1 and B = 65 once each.

Every test prints the worst deviation / tolerance it saw before it asserts (must be <= 1); tests/tolerances_consistency.md is
the table for them (the host-compiled arithmetic is recorded there; the device figures are not measured yet).
"""
import numpy as np
import pytest

import consistency_util as cu
import oracle
import quadrotor_landing_amd as qla
from quadrotor_landing_amd import consistency
from test_gpu_innovation import _same
from util import meas_near

pytestmark = pytest.mark.gpu

B = 197
AB_STATIC, WB_STATIC = [0.2, -0.09, -0.03], [-0.02, -0.01, 0.003]
RECORDS = {"full15": (15, False), "compact9": (9, True), "full9": (9, False)}
F = consistency.SUMMARY_FIELDS


def _torch():
    import torch as t
    return t


@pytest.fixture(autouse=True)
def torch_first():
    """torch is imported before the first handle of a test exists: a torch that is first imported after the engine has initialised the
    HIP runtime reports no GPU."""
    return _torch()


def dev(a, dtype=None):
    t = _torch()
    a = np.ascontiguousarray(a if dtype is None else a.astype(dtype))
    return t.from_numpy(a).to("cuda:0")


def host(*ts):
    _torch().cuda.synchronize()
    return tuple(x.cpu().numpy().astype(np.float64) if x.dtype.is_floating_point else x.cpu().numpy() for x in ts)


def held(dtype, a):
    return a.astype(np.float32).astype(np.float64) if dtype == "f32" else a


class Case:
    """A handle whose states carry P = D C D (kappa(C) <= 100) and a truth displaced by errors drawn from that P."""

    def __init__(self, dtype, record, use_pfp, monkeypatch, batch=B, seed=77, **kw):
        self.dtype, (self.n, compact), self.B = dtype, RECORDS[record], batch
        monkeypatch.setenv("QLE_COMPACT", "1" if compact else "0")   # read at handle creation, as tests/test_gpu_compact.py sets it
        monkeypatch.setenv("QLE_QUAD", "0")
        self.kw = dict(update_freq=400.0, direct_orien_method=1, est_bias=int(self.n == 15), ab_static=AB_STATIC, wb_static=WB_STATIC, **kw)
        self.ekf = qla.BatchedRelativePoseEKF(batch, dtype, **self.kw)
        assert self.ekf.num_states == self.n and self.ekf.policy()["record_words"] == (64 if compact else 136)
        rng = self.rng = np.random.default_rng(seed + self.n + 3 * use_pfp + (dtype == "f32"))
        if use_pfp:   # different static biases per filter: a bias read from the wrong record (or the shared ones) fails
            pfp = np.zeros((batch, 24))
            pfp[:, 0:12] = np.array(list(self.ekf.derived.Q))
            pfp[:, 12:15] = np.array(AB_STATIC) + 0.05 * rng.normal(size=(batch, 3))
            pfp[:, 15:18] = np.array(WB_STATIC) + 0.005 * rng.normal(size=(batch, 3))
            pfp[:, 18:24] = np.array(list(self.ekf.derived.R))
            self.ekf.set_filter_params(pfp)
            static = self.ekf.get_filter_params()[:, 12:18]
        else:
            static = np.broadcast_to(held(dtype, np.array(AB_STATIC + WB_STATIC)), (batch, 6))
        self.ab, self.wb = static[:, 0:3], static[:, 3:6]
        x, P, self.xt = cu.make_case(rng, batch, self.n, "f64", self.ab, self.wb)
        self.ekf.set_state(x, P)
        self.x, self.P = self.ekf.get_state()          # what the device holds
        self.io = qla.DeviceIO(self.ekf)

    def reference(self, xt_given, blocks):
        """numpy on get_state() and the truth as the compute dtype holds it"""
        eref = cu.err_ref(self.x, held(self.dtype, xt_given), self.ab, self.wb, self.n)
        return cu.nees_ref(self.P, eref, blocks), eref

    def close(self):
        self.io.close()
        self.ekf.close()


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("use_pfp", [False, True], ids=["shared", "pfp"])
@pytest.mark.parametrize("record", list(RECORDS))
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_nees_matches_the_dense_solve(dtype, record, use_pfp, monkeypatch):
    c = Case(dtype, record, use_pfp, monkeypatch)
    worst_n = worst_e = 0.0
    for tdt in (np.float32, np.float64):
        xt_given = c.xt.astype(tdt).astype(np.float64)
        xt_dev = dev(c.xt, tdt)
        eref = None
        for name, bits in cu.NAMED_BLOCKS.items():
            if c.n == 9 and name != "all" and bits & ~7:
                with pytest.raises(ValueError, match="bias block"):
                    c.io.nees(xt_dev, blocks=name)
                continue
            nees, err, summ = host(*c.io.nees(xt_dev, blocks=name, return_err=True))
            ref, eref = c.reference(xt_given, 7 if (name == "all" and c.n == 9) else bits)
            rn, re_ = cu.nees_ratio(nees, ref, c.P, dtype), cu.err_ratio(err, eref, dtype)
            print(f"{dtype} {record} pfp={use_pfp} truth={tdt.__name__} blocks={name}: |nees - ref| / tol {rn:.3g}, err / bar {re_:.3g}")
            worst_n, worst_e = max(worst_n, rn), max(worst_e, re_)
            assert err.shape == (c.B, c.n) and np.isfinite(nees).all()
            assert rn <= 1.0 and re_ <= 1.0, (name, rn, re_)
            s = dict(zip(F, summ))
            assert s["count"] == c.B and s["n_not_pd"] == 0 and s["n_above"] == 0 and s["dof"] == 3 * bin(bits & (31 if c.n == 15 else 7)).count("1")
    print(f"WORST {dtype} {record} pfp={use_pfp}: nees {worst_n:.3g} err {worst_e:.3g}")
    c.close()


@pytest.mark.parametrize("batch", [1, 65])
def test_single_filter_and_one_filter_past_a_tile(batch, monkeypatch):
    c = Case("f32", "full15", False, monkeypatch, batch=batch)
    nees, err, summ = host(*c.io.nees(dev(c.xt, np.float64), return_err=True))
    ref, eref = c.reference(c.xt, 31)
    assert cu.nees_ratio(nees, ref, c.P, "f32") <= 1.0 and cu.err_ratio(err, eref, "f32") <= 1.0
    assert summ[0] == batch and abs(summ[1] - nees.sum()) <= batch * 2.0 ** -52 * nees.sum()
    c.close()


# ------------------------------------------------------------------------------------------------ 2. the two entry points
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_host_entry_and_tensor_entry_agree_bit_for_bit(dtype, monkeypatch):
    c = Case(dtype, "full15", True, monkeypatch)
    mask = (c.rng.uniform(size=c.B) < 0.8).astype(np.uint8)
    for blocks in ("all", "pose"):
        h = c.ekf.nees(c.xt, mask=mask, blocks=blocks, chi2_hi=20.0)
        nees, err, summ = host(*c.io.nees(dev(c.xt, np.float64), mask=dev(mask), blocks=blocks, chi2_hi=20.0, return_err=True, dtype="float64"))
        assert _same(h["nees"], nees) and _same(h["err"], err)
        assert _same(np.array([h[k] for k in F]), summ)
        assert h["count"] == mask.sum() and h["mean_nees"] == h["sum_nees"] / h["count"]
    c.close()


# ------------------------------------------------------------------------------------------------ 3. after a real run
def test_nees_after_a_synthetic_run_fp64():
    """256 fp64 filters, 56 ticks of the generator, then synth_nees: every finite NEES against numpy on get_state() and
    synth_get_truth, to the formula tolerance (fp64 keeps it meaningful for whatever kappa a converged P has).  The batch mean is
    recorded, not asserted: it is a finding about the filter."""
    kw = dict(update_freq=400.0, measurement_freq=30.0, limit_measurement_freq=1, direct_orien_method=1,
              Q_a=[0.0005] * 3, Q_w=[0.00005] * 3, R_r=[0.015, 0.015, 0.020], R_ang=[0.0015, 0.0015, 0.04])
    Bn, T = 256, 56
    thm = np.zeros(T, np.uint8); thm[13::14] = 1
    ekf = qla.BatchedRelativePoseEKF(Bn, "f64", **kw)
    seq = ekf.make_inputs(T, thm)
    ekf.synth_generate(seq, seed=0xE4F00001)
    ekf.run(seq, 0, T)
    out = ekf.synth_nees(seq, chi2_hi=30.0)
    x, P = ekf.get_state()
    pose, bias = ekf.synth_truth(seq)
    n = ekf.num_states
    ab, wb = np.array(list(ekf.params.ab_static)), np.array(list(ekf.params.wb_static))
    xt = np.zeros((Bn, 16)); xt[:, 0:3] = pose[:, 0:3]; xt[:, 6:10] = pose[:, 3:7]; xt[:, 10:13] = bias[:, 0:3] + ab; xt[:, 13:16] = bias[:, 3:6] + wb
    bits = 29 if n == 15 else 5
    eref = cu.err_ref(x, xt, ab, wb, n)
    ref = cu.nees_ref(P, eref, bits)
    fin = np.isfinite(out["nees"])
    assert fin.sum() == out["count"] > 0 and out["dof"] == 3 * bin(bits).count("1")
    ratio = cu.nees_ratio(out["nees"][fin], ref[fin], P[fin], "f64")
    print(f"synthetic run: {int(fin.sum())} finite of {Bn}, mean NEES {out['mean_nees']:.4g} over dof {out['dof']:.0f}, kappa up to "
          f"{cu.kappa_scaled(P[fin]).max():.3g}, worst |nees - ref| / tol {ratio:.3g}, n_above(30) {out['n_above']:.0f}")
    assert ratio <= 1.0
    # the generator keeps no velocity: that block is blanked on both sides, in place, so that err_ratio still finds every block
    # (theta, with its absolute bar, among them) at its own columns
    err, eref = out["err"][fin].copy(), eref[fin].copy()
    err[:, 3:6] = eref[:, 3:6] = 0.0
    re_ = cu.err_ratio(err, eref, "f64")
    print(f"synthetic run: err / bar {re_:.3g}")
    assert re_ <= 1.0
    assert out["n_above"] == (out["nees"][fin] > 30.0).sum()
    ekf.close()


# ------------------------------------------------------------------------------------------------ 4. off filters, read-only
@pytest.mark.parametrize("multirate", [0, 1], ids=["single-rate", "multirate"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_off_filters_and_no_state_write(dtype, multirate, monkeypatch):
    mr = dict(multirate_ekf=1, measurement_delay=0.03) if multirate else {}
    c = Case(dtype, "full15", False, monkeypatch, **mr)
    po = oracle.make_params(update_freq=400.0, direct_orien_method=1)
    seeded = (np.arange(c.B) % 2 == 0).astype(np.uint8)
    c.ekf.set_state(np.zeros((c.B, 16)), np.zeros((c.B, 15, 15)))
    c.ekf.initialize_state(meas_near(c.rng, po, c.x, ang=0.2, pos=0.05), mask=seeded)
    assert np.array_equal(c.ekf.state_initialized(), seeded)
    x0, P0 = c.ekf.get_state()
    mask = np.ones(c.B, np.uint8); mask[[0, 2, 64, 130, 196]] = 0          # cleared on some seeded filters
    on = (seeded != 0) & (mask != 0)
    e = np.sqrt(np.einsum("bii->bi", np.where(seeded[:, None, None] != 0, P0, 1.0))) * c.rng.normal(size=(c.B, 15))
    xt = cu.displace(np.where(seeded[:, None] != 0, x0, c.x), e, c.ab, c.wb)
    nees, err, summ = host(*c.io.nees(dev(xt, np.float64), mask=dev(mask), return_err=True))
    h = c.ekf.nees(xt, mask=mask)
    x1, P1 = c.ekf.get_state()
    assert _same(x0, x1) and _same(P0, P1)                                  # nothing was written
    assert np.isnan(nees[~on]).all() and not err[~on].any() and np.isfinite(nees[on]).all() and err[on].any(axis=1).all()
    assert summ[0] == on.sum() == h["count"] and summ[4] == 0
    eref = cu.err_ref(x0[on], held(dtype, xt)[on], c.ab[on], c.wb[on], 15)
    assert cu.nees_ratio(nees[on], cu.nees_ref(P0[on], eref, 31), P0[on], dtype) <= 1.0
    c.close()


# ------------------------------------------------------------------------------------------------ 5. the batch summary
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_summary_sums_counts_determinism_and_additivity(dtype, monkeypatch):
    c = Case(dtype, "full15", False, monkeypatch)
    xt = dev(c.xt, np.float64)
    nees, err, s1 = host(*c.io.nees(xt, return_err=True, dtype="float64"))
    srt = np.sort(nees)
    chi2 = 0.5 * (srt[150] + srt[151])                                       # between two sorted values
    nees2, s2 = host(*c.io.nees(xt, chi2_hi=chi2, dtype="float64"))
    nees3, s3 = host(*c.io.nees(xt, chi2_hi=chi2, dtype="float64"))
    assert _same(nees, nees2) and _same(s2, s3) and _same(nees2, nees3)      # deterministic
    s = dict(zip(F, s2))
    bound = c.B * 2.0 ** -52
    assert s["count"] == c.B and s["n_above"] == c.B - 151 and s["n_not_pd"] == 0 and s["dof"] == 15 and s1[3] == 0
    assert abs(s["sum_nees"] - nees.sum()) <= bound * nees.sum()
    assert abs(s["sum_nees_sq"] - (nees ** 2).sum()) <= bound * (nees ** 2).sum()
    er, et = (err[:, 0:3] ** 2).sum(), (err[:, 6:9] ** 2).sum()
    assert abs(s["sum_r_err_sq"] - er) <= bound * er and abs(s["sum_theta_err_sq"] - et) <= bound * et
    # two half-batch handles add up to the whole batch
    tot = np.zeros(8)
    for lo, hi in ((0, 100), (100, c.B)):
        e = qla.BatchedRelativePoseEKF(hi - lo, dtype, **c.kw)
        e.set_state(c.x[lo:hi], c.P[lo:hi])
        io = qla.DeviceIO(e)
        n_h, s_h = host(*io.nees(dev(c.xt[lo:hi], np.float64), chi2_hi=chi2, dtype="float64"))
        assert _same(n_h, nees[lo:hi])
        tot += s_h
        io.close(); e.close()
    assert tot[0] == s["count"] and tot[3] == s["n_above"] and tot[4] == 0
    for k in (1, 2, 5, 6):
        assert abs(tot[k] - s2[k]) <= bound * s2[k], (F[k], tot[k], s2[k])
    c.close()


# ------------------------------------------------------------------------------------------------ 6. not positive definite
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_not_positive_definite_filter_is_flagged_and_alone(dtype, monkeypatch):
    c = Case(dtype, "full15", False, monkeypatch)
    xt = dev(c.xt, np.float64)
    base, sb = host(*c.io.nees(xt))
    bad = 70                                                                 # mid-wave, second tile
    P = c.P.copy(); P[bad, 4, 4] = -P[bad, 4, 4]
    c.ekf.set_state(c.x, P)
    nees, s = host(*c.io.nees(xt))
    assert np.isnan(nees[bad]) and s[4] == 1 and s[0] == c.B - 1 and sb[4] == 0 and sb[0] == c.B
    keep = np.arange(c.B) != bad
    assert _same(nees[keep], base[keep])                                     # its tile neighbours are unchanged
    c.close()


# ------------------------------------------------------------------------------------------------ 7. launches
def test_two_launches_per_call_and_none_in_the_tick_library(monkeypatch):
    c = Case("f32", "full15", False, monkeypatch)
    xt = dev(c.xt, np.float32)
    c.io.nees(xt)
    K = consistency.consistency_lib()
    n0 = K.qcs_launch_count()
    with qla.launch_census() as names:
        c.io.nees(xt)
        assert K.qcs_launch_count() - n0 == 2
        c.io.nees(xt, blocks="pose", return_err=True)
        assert K.qcs_launch_count() - n0 == 4
    assert names == [], names                                                # the tick library's census sees no new kernel
    c.ekf.synchronize()
    c.close()
