"""Every filter is independent of its wave neighbours.

In the reference every filter is its own RelativePoseEKF object: nothing one filter sees can change another's numbers.  The engine
runs 64 filters per wave (16 per workgroup in the cooperative kernel) and several of its kernels decide by a vote across lanes
(half_angle_sinc_cos's halving count, k_step_mr's chain bounds and fp32 early ballot, the cooperative kernel's "nobody corrects"
skip, wave-tile addressing, masked seeding).  These tests hold every healthy filter BIT FOR BIT across neighbourhoods:

  a. the same healthy filters alone and next to "disturbers" (huge rotations, Inf / NaN in IMU samples or states, uninitialised
     filters, 170-degree innovations, all-zero tag records, noise four decades off) at lane 0, lane 63, mid-wave, the 16th filter of
     a cooperative workgroup and the ragged tail, through every entry point, both dtypes and all three kernel families;
  b. mixed waves of per-tick rotations from 1e-12 to 40 rad against the oracle (the device counterpart of the host-only
     test_engine_quaternion_exp_large_angles_halving_and_doubling);
  c. Inf / NaN disturbers stay in their own filters over a free run, every other filter matches the oracle;
  d. a mixed population run as laid out and under a permutation across waves and workgroups.

Non-finite values go only into IMU samples, states and per-filter parameters: never into timestamps, tick indices, masks or anything
else that feeds an index or an address.
"""
import numpy as np
import pytest

import oracle
import quadrotor_landing_amd as qla
import test_gpu_parity as tp
from util import assert_state_close, meas_near, oracle_predict_batch, qmul, rand_imu, rand_states

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["default", "lanes-only", "coop-forced"])
def kernel_family(request, monkeypatch):
    """As in test_gpu_parity: the default policy, the one-lane kernels only (QLE_QUAD=0) and the cooperative kernel forced for every
    single-rate tick (QLE_QUAD=3); QLE_QUAD is read at handle creation."""
    if request.param == "lanes-only":
        monkeypatch.setenv("QLE_QUAD", "0")
    elif request.param == "coop-forced":
        monkeypatch.setenv("QLE_QUAD", "3")
    else:
        monkeypatch.delenv("QLE_QUAD", raising=False)
    return request.param


B = 64 * 6 + 23                                    # six waves and a ragged tail
DIST = np.array([0, 63, 64 + 32, 2 * 64 + 15, 64 * 6 + 9])   # lane 0, lane 63, mid-wave, 16th filter of a workgroup, ragged tail
HEALTHY = np.setdiff1d(np.arange(B), DIST)
BASE = dict(update_freq=400.0, direct_orien_method=1, measurement_freq=30.0, limit_measurement_freq=1, corner_margin_enbl=0,
            ab_static=[0.2, -0.09, -0.03], wb_static=[-0.02, -0.01, 0.0])
ENTRY_KW = {
    "predict": {}, "update": {}, "step": {}, "run": {}, "run_resident": {},
    "fu_gated": dict(update_freq=100.0),
    "mr_fixed": dict(update_freq=100.0, multirate_ekf=1, dynamic_meas_delay=0, measurement_delay=0.030),
    "mr_dynamic": dict(update_freq=100.0, multirate_ekf=1, dynamic_meas_delay=1, measurement_delay=0.030, measurement_delay_max=0.200,
                       dyn_measurement_delay_offset=0.005),
    "compact": dict(est_bias=0),
}
TICKS = {"predict": 1, "update": 1, "step": 1, "run": 12, "run_resident": 12, "fu_gated": 12, "mr_fixed": 20, "mr_dynamic": 20, "compact": 8}
NO_IMU = {"update"}                               # entry points that take no IMU sample
NO_CORR = {"predict"}                             # entry points that take no tag record
DISTURBERS = ["rot2p5", "rot1e3", "wb_inf", "imu_nan", "state_nan", "uninit", "corr170", "zero_tag_on", "zero_tag_off", "noise4"]


def _cases():
    out = []
    for e in ENTRY_KW:
        for d in DISTURBERS:
            if e in NO_IMU and d in ("rot2p5", "rot1e3", "imu_nan"):
                continue
            if e in NO_CORR and d in ("corr170", "zero_tag_on", "zero_tag_off"):
                continue
            out.append((e, d))
    return out


def _rot_meas(po, x, ang, rng):
    """Tag records whose attitude is `ang` rad away from the state's (exactly), position near."""
    z = meas_near(np.random.default_rng(rng.integers(1 << 30)), po, x, ang=0.0, pos=0.05)
    ax = rng.normal(size=(x.shape[0], 3)); ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    dq = np.concatenate([ax * np.sin(ang / 2), np.full((x.shape[0], 1), np.cos(ang / 2))], axis=1)
    z[:, 3:7] = qmul(z[:, 3:7], dq)
    return z


def _scenario(entry, seed=4242):
    """Healthy inputs for every filter: state, IMU per tick, tag record / mask per tick, camera stamps, per-filter parameters."""
    kw = dict(BASE, **ENTRY_KW[entry])
    po = oracle.make_params(**kw)
    n = po.num_states
    rng = np.random.default_rng(seed)
    T = TICKS[entry]
    x, P = rand_states(rng, B, n, cov_scale=0.3)
    if n == 9:
        x[:, 10:16] = 0.0
    U = np.stack([rand_imu(rng, B) * np.array([0.05, 0.05, 1, 0.2, 0.2, 0.2]) for _ in range(T)])
    Z = np.stack([meas_near(rng, po, x, ang=0.3, pos=0.05) for _ in range(T)])
    M = (rng.uniform(size=(T, B)) < 0.5).astype(np.uint8)
    M[:, 64:128] = 1                                  # one wave that corrects throughout
    M[:, 192:256] = 0                                 # one that never does
    stamps = np.stack([0.01 * t - rng.uniform(0.0, 0.12, size=B) for t in range(T)])   # measurement ages vary within every wave
    pfp = np.zeros((B, 24))
    pfp[:, 0:12] = np.array(list(po.Q)); pfp[:, 12:15] = kw["ab_static"]; pfp[:, 15:18] = kw["wb_static"]; pfp[:, 18:24] = np.array(list(po.R))
    return dict(kw=kw, po=po, n=n, T=T, x=x, P=P, U=U, Z=Z, M=M, stamps=stamps, pfp=pfp, rng=rng)


def _disturb(s, kind, lanes=DIST):
    """A copy of scenario s with disturber `kind` in `lanes`.  Non-finite values only in IMU samples, states and parameters."""
    s = dict(s, x=s["x"].copy(), P=s["P"].copy(), U=s["U"].copy(), Z=s["Z"].copy(), M=s["M"].copy(), pfp=s["pfp"].copy())
    rng = np.random.default_rng(99)
    dT = 1.0 / s["kw"]["update_freq"]
    L = np.asarray(lanes)
    if kind in ("rot2p5", "rot1e3"):                  # per-tick rotation dT (w - wb - wb_static) of 2.5 rad / 1000 rad
        ang = 2.5 if kind == "rot2p5" else 1e3
        ax = rng.normal(size=(len(L), 3)); ax /= np.linalg.norm(ax, axis=1, keepdims=True)
        s["U"][:, L, 3:6] = s["x"][L, 13:16] + np.array(s["kw"]["wb_static"]) + ax * (ang / dT)
    elif kind == "wb_inf":
        s["x"][L, 13:16] = np.inf
    elif kind == "imu_nan":
        s["U"][:, L, :] = np.nan
    elif kind == "state_nan":
        s["x"][L] = np.nan
        s["P"][L] = np.nan
    elif kind == "uninit":                            # never seeded: zero attitude quaternion (qle_get_state_initialized)
        s["x"][L] = 0.0
    elif kind == "corr170":                           # 170-degree innovation: |delta theta| > pi/2 through the correction
        s["P"][L] *= 10.0
        for t in range(s["T"]):
            s["Z"][t, L] = _rot_meas(s["po"], s["x"][L], np.deg2rad(170.0), rng)
        s["M"][:, L] = 1
    elif kind in ("zero_tag_on", "zero_tag_off"):
        s["Z"][:, L] = 0.0
        s["M"][:, L] = 1 if kind == "zero_tag_on" else 0
    elif kind == "noise4":                            # per-filter noise four decades off
        s["pfp"][L, 0:12] *= 1e4
        s["pfp"][L, 18:24] *= 1e-4
    else:
        raise ValueError(kind)
    return s


def _drive(entry, dtype, s, use_pfp, monkeypatch):
    """Run scenario s through one entry point.  Returns (x, P, extras) with extras the aux outputs / tick flags the entry has."""
    if entry == "compact":
        monkeypatch.setenv("QLE_COMPACT", "1")
    ekf = qla.BatchedRelativePoseEKF(B, dtype, params=qla.make_params(**s["kw"]))
    if use_pfp:
        ekf.set_filter_params(s["pfp"])
    ekf.set_state(s["x"], s["P"])
    U, Z, M, T = s["U"], s["Z"], s["M"], s["T"]
    extras = []
    if entry in ("predict", "update", "step", "compact"):
        ekf.enable_aux(True)
        for t in range(T):
            if entry == "predict":
                ekf.predict(U[t])
            elif entry == "update":
                ekf.update(Z[t], M[t])
            else:
                ekf.step(U[t], Z[t], M[t])
            extras += list(ekf.get_aux())
    elif entry in ("run", "run_resident"):
        thm = np.zeros(T, np.uint8); thm[2::3] = 1
        seq = ekf.make_inputs(T, thm)
        for t in range(T):
            seq.upload_tick(t, U[t], Z[t] if thm[t] else None, M[t] if thm[t] else None)
        (ekf.run if entry == "run" else ekf.run_resident)(seq, 0, T)
        seq.close()
    else:
        ekf.enable_gating(True)
        pending = np.zeros(B, np.uint8)
        for t in range(T):
            pending |= M[t]
            if entry == "mr_dynamic":
                ekf.filter_update(U[t], Z[t], pending, t_curr=0.01 * t, apriltag_time=s["stamps"][t])
            else:
                ekf.filter_update(U[t], Z[t], pending)
            flags = ekf.tick_flags()
            pending &= (1 - flags[1])
            extras += list(flags)
    x, P = ekf.get_state()
    ekf.close()
    return x, P, extras


# The one path that is not bit-identical across neighbourhoods: the multirate replay (k_step_mr) picks its code path per WAVE --
# fp32: the early correction (all valid lanes correct at the entry their chain starts from: `early` ballot) or the correction inside the
# replay loop; both dtypes: which replayed predict ticks run in the loop copy that carries the correction (up to the wave-uniform t_cmax)
# and which in the copy without it.  The arithmetic is the same source in each copy, but each copy is inlined separately and the backend
# contracts products and sums into FMAs per copy (read from the code, not yet confirmed in the ISA), so the last bits of a filter's
# replay follow its neighbours' measurements (measured on
# an MI355X: 1.9e-6 absolute in an fp32 state word, 8.7e-19 in an fp64 covariance entry).  A neighbour that changes
# which of its wave's lanes correct is what moves the choice.  Those filters are held against the oracle at the multirate tolerances
# (test_population_is_permutation_invariant) and, where no oracle replay of the scenario exists, run B against run A at the same bounds.
MR_TOL = {"f64": dict(rtol=1e-10, atol=1e-12, qtol=1e-10), "f32": dict(rtol=2e-5, atol=2e-5, qtol=5e-6, ptol=5e-5)}
MR_PATH_MOVERS = {"zero_tag_off"}      # disturbers that change which lanes of a wave correct: they move the wave's path choice


# ----------------------------------------------------------------------------------------------- a. neighbour invariance
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("entry,kind", _cases())
def test_healthy_filters_do_not_see_their_neighbours(entry, kind, dtype, monkeypatch):
    """The same healthy filters alone (run A) and next to disturbers (run B): identical bits in x, P and the aux outputs / tick
    flags of every healthy filter."""
    s = _scenario(entry)
    use_pfp = kind == "noise4"
    xa, Pa, ea = _drive(entry, dtype, s, use_pfp, monkeypatch)
    xb, Pb, eb = _drive(entry, dtype, _disturb(s, kind), use_pfp, monkeypatch)
    h = HEALTHY
    assert np.isfinite(xa).all() and np.isfinite(Pa).all()
    if entry.startswith("mr_") and kind in MR_PATH_MOVERS:   # the multirate replay's wave-level path choice (MR_TOL above)
        assert_state_close(xb[h], Pb[h], xa[h], Pa[h], **MR_TOL[dtype])
    else:
        np.testing.assert_array_equal(xb[h], xa[h])
        np.testing.assert_array_equal(Pb[h], Pa[h])
    for a, b in zip(ea, eb):
        np.testing.assert_array_equal(b[h], a[h])


# ------------------------------------------------------------------------ b. large angles in mixed waves, against the oracle
def _mixed_angles(rng, n):
    """Per-tick rotation angles from 1e-12 to 40 rad, large ones scattered through every wave."""
    ang = 10 ** rng.uniform(-12, -0.5, n)
    big = rng.uniform(size=n) < 0.25
    ang[big] = rng.uniform(1.6, 40.0, int(big.sum()))
    return ang, big


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_predict_mixed_wave_large_angles_against_oracle(dtype):
    """One predict per filter with per-tick rotations 1e-12 .. 40 rad mixed inside every wave.  Every lane against the oracle at the
    predict tolerances; only the fp32 large-angle lanes get a looser quaternion / covariance bound (see below)."""
    kw = dict(BASE)
    po, pq = tp.both(**kw)
    rng = np.random.default_rng(515)
    x, P = rand_states(rng, B, 15, cov_scale=0.3)
    u = rand_imu(rng, B)
    ang, big = _mixed_angles(rng, B)
    ax = rng.normal(size=(B, 3)); ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    u[:, 3:6] = x[:, 13:16] + np.array(kw["wb_static"]) + ax * (ang / (1.0 / kw["update_freq"]))[:, None]
    if dtype == "f32":   # the inputs the fp32 engine sees
        x = x.astype(np.float32).astype(np.float64); P = P.astype(np.float32).astype(np.float64); u = u.astype(np.float32).astype(np.float64)
    ekf = qla.BatchedRelativePoseEKF(B, dtype, params=pq)
    xg, Pg, _ = ekf.prediction_step(x, P, u)
    ekf.close()
    xr, Pr, _ = oracle_predict_batch(po, x, P, u)
    tol = tp.F64 if dtype == "f64" else tp.F32
    assert_state_close(xg[~big], Pg[~big], xr[~big], Pr[~big], **tol)
    # large-angle lanes: fp64 at the standard bounds (measured on an MI355X: 3.8e-15 quaternion, 8.7e-15 covariance).  fp32 loosens the
    # quaternion and covariance bounds only: |phi|^2 carries 1e-7 relative before any series, i.e. 1.5e-6 rad at 30 rad per tick, as in
    # the host test (which allows 5e-6 on quaternion_exp).  Measured 1.43e-6 (quaternion) and 3.4e-6 (covariance); bounds ~3x that.
    lt = tol if dtype == "f64" else dict(tol, qtol=5e-6, ptol=1e-5)
    assert_state_close(xg[big], Pg[big], xr[big], Pr[big], **lt)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_fused_tick_mixed_wave_large_corrections_against_oracle(dtype):
    """The fused tick with predict rotations 1e-12 .. 40 rad and attitude innovations up to 170 degrees (|delta theta| > pi/2 through
    quaternion_exp) mixed inside every wave, every filter correcting: every lane against the oracle at the correction tolerances."""
    kw = dict(BASE)
    po, pq = tp.both(**kw)
    rng = np.random.default_rng(616)
    x, P = rand_states(rng, B, 15, cov_scale=0.3)
    u = rand_imu(rng, B)
    ang, big = _mixed_angles(rng, B)
    ax = rng.normal(size=(B, 3)); ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    u[:, 3:6] = x[:, 13:16] + np.array(kw["wb_static"]) + ax * (ang / (1.0 / kw["update_freq"]))[:, None]
    if dtype == "f32":
        x = x.astype(np.float32).astype(np.float64); P = P.astype(np.float32).astype(np.float64); u = u.astype(np.float32).astype(np.float64)
    xp = oracle_predict_batch(po, x, P, u)[0]
    inn = np.where(rng.uniform(size=B) < 0.3, np.deg2rad(rng.uniform(100.0, 170.0, B)), rng.uniform(0.0, 0.3, B))
    z = np.concatenate([_rot_meas(po, xp[i:i + 1], inn[i], rng) for i in range(B)])
    if dtype == "f32":
        z = z.astype(np.float32).astype(np.float64)
    mask = np.ones(B, np.uint8)
    ekf = qla.BatchedRelativePoseEKF(B, dtype, params=pq)
    ekf.set_state(x, P)
    ekf.step(u, z, mask)
    xg, Pg = ekf.get_state()
    ekf.close()
    xr, Pr = oracle.run_batch(po, x, P, u[None], z[None], mask[None])
    tol = tp.UPD[dtype]
    assert_state_close(xg[~big], Pg[~big], xr[~big], Pr[~big], **tol)
    # the large-angle lanes need no looser bound here (measured on an MI355X: fp32 6.5e-7 quaternion, 2e-5 covariance; fp64 1e-15, 5.4e-14)
    assert_state_close(xg[big], Pg[big], xr[big], Pr[big], **tol)


# ------------------------------------------------------------------------------------------- c. non-finite containment
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_non_finite_filters_stay_contained_over_a_free_run(dtype):
    """Disturbers holding Inf / NaN (gyro bias +Inf, NaN IMU samples, NaN state) in k filters: after a 30-tick free run with
    corrections exactly those k filters are non-finite, and every other filter matches the oracle at the free-run tolerances."""
    kw = dict(BASE)
    po, pq = tp.both(**kw)
    rng = np.random.default_rng(717)
    T = 30
    x, P = rand_states(rng, B, 15, cov_scale=0.3)
    # body rates of ~10 rad/s: a neighbour forced onto the first-order exponential (k = 1/2, cos = 1) would be off by |phi|^3 / 8 ~ 2e-6
    # per tick, far above the tolerances
    U = np.stack([rand_imu(rng, B) * np.array([0.05, 0.05, 1, 25.0, 25.0, 25.0]) for _ in range(T)])
    Z = np.stack([meas_near(rng, po, x, ang=0.2, pos=0.05) for _ in range(T)])
    thm = np.zeros(T, np.uint8); thm[13::14] = 1
    M = np.zeros((T, B), np.uint8); M[thm.astype(bool)] = (rng.uniform(size=(int(thm.sum()), B)) < 0.6)
    if dtype == "f32":   # the inputs the fp32 engine sees
        x = x.astype(np.float32).astype(np.float64); P = P.astype(np.float32).astype(np.float64)
        U = U.astype(np.float32).astype(np.float64); Z = Z.astype(np.float32).astype(np.float64)
    bad = {"wb_inf": [0, 2 * 64 + 15], "imu_nan": [63, 5 * 64 + 40], "state_nan": [64 + 32, 64 * 6 + 9]}
    Ub, xb, Pb = U.copy(), x.copy(), P.copy()
    xb[bad["wb_inf"], 13:16] = np.inf
    Ub[5:, bad["imu_nan"], 3] = np.nan
    xb[bad["state_nan"]] = np.nan
    allbad = sorted(sum(bad.values(), []))
    ok = np.setdiff1d(np.arange(B), allbad)
    ekf = qla.BatchedRelativePoseEKF(B, dtype, params=pq)
    ekf.set_state(xb, Pb)
    seq = ekf.make_inputs(T, thm)
    for t in range(T):
        seq.upload_tick(t, Ub[t], Z[t] if thm[t] else None, M[t] if thm[t] else None)
    ekf.run(seq, 0, T)
    assert ekf.count_nonfinite() == len(allbad)
    xg, Pg = ekf.get_state()
    seq.close(); ekf.close()
    assert not np.isfinite(xg[allbad]).all(axis=1).any()
    xr, Pr = oracle.run_batch(po, x[ok], P[ok], U[:, ok], Z[:, ok], M[:, ok])
    if dtype == "f64":
        tp.free_run_close(xg[ok], Pg[ok], xr, Pr, 1e-9)
    else:
        tp.free_run_close(xg[ok], Pg[ok], xr, Pr, 6e-5, ftol=4e-4)


# ------------------------------------------------------------------------------------------- d. permutation invariance
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("mr", [0, 1])
def test_population_is_permutation_invariant(mr, dtype):
    """A mixed population -- per-filter parameters, mixed masks, filters seeded on their own first detection, gating with the
    13-tag hardware bundle, multirate with a dynamic delay (mr = 1) -- run as laid out and under a random permutation that moves
    filters across waves and workgroups: after undoing the permutation both runs agree bit for bit, flags and delays included
    (multirate states: the replay's wave-level path choice moves their last bits, see MR_TOL; they are held against the oracle's
    filter objects at the multirate tolerances instead, and everything is compared with the oracle in both layouts)."""
    kw = dict(BASE, update_freq=100.0, multirate_ekf=mr, dynamic_meas_delay=1, measurement_delay=0.030, measurement_delay_max=0.200,
              dyn_measurement_delay_offset=0.005, limit_measurement_freq=0, corner_margin_enbl=1, **tp.HW_TAGS)
    po, pq = tp.both(**kw)
    rng = np.random.default_rng(818 + mr)
    T = 40
    pfp = np.zeros((B, 24))
    pfp[:, 0:12] = np.array(list(po.Q)) * 10 ** rng.uniform(-0.5, 0.5, size=(B, 4)).repeat(3, axis=1)
    pfp[:, 12:15] = rng.normal(size=(B, 3)) * 0.1
    pfp[:, 15:18] = rng.normal(size=(B, 3)) * 0.01
    pfp[:, 18:24] = np.array(list(po.R)) * rng.uniform(0.5, 2.0, size=(B, 6))
    z0 = np.zeros((B, 7))
    z0[:, 0:2] = rng.normal(size=(B, 2)) * 0.1; z0[:, 2] = rng.uniform(0.8, 2.0, size=B)
    z0[:, 3:7] = np.array([0.7071067811865476, -0.7071067811865476, 0.0, 0.0])
    first = rng.integers(0, 12, size=B)              # tick of each filter's first detection
    first[:64] = 0
    U = np.stack([rand_imu(rng, B) * np.array([0.05, 0.05, 1, 0.2, 0.2, 0.2]) for _ in range(T)])
    NEW = rng.uniform(size=(T, B)) < 0.4
    ZN = np.zeros((T, B, 7)); ST = np.zeros((T, B))
    for t in range(T):
        zt = z0.copy()
        zt[:, 0:3] += rng.normal(size=(B, 3)) * 0.02
        ZN[t] = zt
        ST[t] = 0.01 * t - rng.uniform(0.0, 0.15, size=B)
    perm = rng.permutation(B)
    if dtype == "f32":   # the inputs the fp32 engine sees
        z0 = z0.astype(np.float32).astype(np.float64); U = U.astype(np.float32).astype(np.float64)
        ZN = ZN.astype(np.float32).astype(np.float64)

    def seeded_state(dtype):
        """Every filter's state right after its seeding, as the engine computes it."""
        ekf = qla.BatchedRelativePoseEKF(B, dtype, params=pq)
        ekf.set_filter_params(pfp)
        ekf.initialize_state(z0, reinit_bias=True)
        xs = ekf.get_state()[0]
        ekf.close()
        return xs

    def run(p):
        ekf = qla.BatchedRelativePoseEKF(B, dtype, params=pq)
        ekf.set_filter_params(pfp[p])
        ekf.enable_gating(True)
        x0 = np.zeros((B, 16)); P0 = np.tile(np.eye(15), (B, 1, 1))
        ekf.set_state(x0, P0)                         # every filter unseeded (zero quaternion)
        pending = np.zeros(B, np.uint8); zlast = z0[p].copy(); stamp = np.zeros(B)
        out = []
        for t in range(T):
            seed = (first[p] == t).astype(np.uint8)
            if seed.any():
                ekf.initialize_state(z0[p], reinit_bias=True, mask=seed)
            new = NEW[t, p] & (first[p] < t)
            zlast[new] = ZN[t, p][new]; stamp[new] = ST[t, p][new]
            pending |= new.astype(np.uint8)
            if mr:
                ekf.filter_update(U[t, p], zlast, pending, t_curr=0.01 * t, apriltag_time=stamp)
            else:
                ekf.filter_update(U[t, p], zlast, pending)
            flags = ekf.tick_flags()
            pending &= (1 - flags[1])
            out += list(flags)
        x, P = ekf.get_state()
        out += [ekf.measurement_delay(), ekf.state_initialized()]
        ekf.close()
        return x, P, out

    ident = np.arange(B)
    xa, Pa, ea = run(ident)
    xb, Pb, eb = run(perm)
    inv = np.argsort(perm)
    assert np.isfinite(xa).all() and np.isfinite(Pa).all()
    assert sum(int(f.sum()) for f in ea[0:3 * T:3]) > B      # corrections happened
    # every filter against its own oracle filter object (the reference's logic: seeded on its first detection, gating, dynamic delay)
    xs0 = seeded_state(dtype)
    filt = []
    for i in range(B):
        q = pfp[i, 0:12]
        pi = oracle.make_params(**dict(kw, Q_a=q[0:3], Q_w=q[3:6], Q_ab=q[6:9], Q_wb=q[9:12], ab_static=pfp[i, 12:15],
                                       wb_static=pfp[i, 15:18], R_r=pfp[i, 18:21], R_ang=pfp[i, 21:24]))
        filt.append(oracle.Filter(pi))
    zlast = z0.copy(); stamp = np.zeros(B)
    for t in range(T):
        for i in np.nonzero(first == t)[0]:
            f = filt[i]
            f.set_apriltag(z0[i, :3], z0[i, 3:], -1.0)   # initialize_state (NODE.cpp:169-174)
            f.f.measurement_ready = 0
            if dtype == "f32":                            # from the engine's fp32-seeded state
                for k in range(3):
                    f.f.r_nom[k] = xs0[i, k]
                for k in range(4):
                    f.f.q_nom[k] = xs0[i, 6 + k]
                for k in range(16):
                    f.f.x_hist[k] = xs0[i, k]
        new = NEW[t] & (first < t)
        zlast[new] = ZN[t][new]; stamp[new] = ST[t][new]
        for i in range(B):
            if first[i] > t:
                continue
            filt[i].set_imu(U[t, i, :3], U[t, i, 3:])
            if new[i]:
                filt[i].set_apriltag(zlast[i, :3], zlast[i, 3:], stamp[i])
            filt[i].filter_update(0.01 * t)
    xr = np.stack([f.x() for f in filt]); Pr = np.stack([f.P() for f in filt])
    np.testing.assert_array_equal(ea[3 * (T - 1)], np.array([f.f.performed_correction for f in filt], np.uint8))
    assert_state_close(xa, Pa, xr, Pr, **MR_TOL[dtype])
    assert_state_close(xb[inv], Pb[inv], xr, Pr, **MR_TOL[dtype])
    if not mr:
        np.testing.assert_array_equal(xb[inv], xa)
        np.testing.assert_array_equal(Pb[inv], Pa)
    for a, b in zip(ea, eb):
        np.testing.assert_array_equal(b[inv], a)
