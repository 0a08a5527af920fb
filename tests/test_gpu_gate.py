"""The chi-square gate in front of the fused tick on the GPU (include/qle_gate.h, libqle_gate.so: k_pregate; DeviceIO.tick(chi2_max=...),
DeviceIO.innovation).

Reference: the dense oracle's prediction_step followed by innovation_ref (innovation_util.py), on the values the device holds
(gate_util.predict_then_innovation); tolerances gate_util.TOL -- those of test_gpu_innovation.py.  Every case runs in both dtypes, both
orientation methods, est_bias 1 / 0 (full / compact records), with and without per-filter parameters, and in the three kernel
families of test_gpu_innovation's kernel_family fixture (the tick BEHIND the gate follows the policy; the gate does not change).
Everything the gate decides rather than computes is compared bit for bit: it only clears mask words, so a gated tick must equal the
ungated tick whose mask is `accepted`.
"""
import ctypes as C

import numpy as np
import pytest

import quadrotor_landing_amd as qla
import test_gpu_parity as tp
from gate_util import TOL, clear_of_threshold, displaced_tag_poses, predict_then_innovation, rel, rot_z
from quadrotor_landing_amd import devio, gate
from test_gpu_innovation import BIG, BW, DIST, HEALTHY, Case, _same, grid, kernel_family  # noqa: F401  (kernel_family: autouse fixture)
from innovation_util import CHI2_6_099
from util import assert_state_close, meas_near, rand_imu

pytestmark = pytest.mark.gpu

RAGGED = 2391


def _torch():
    import torch as t
    return t


@pytest.fixture(autouse=True)
def torch_first():
    """torch is imported before the first handle of a test exists (as test_gpu_devio's first test does): a torch that is first imported
    after the engine has initialised the HIP runtime reports no GPU."""
    return _torch()


def dev(c, a):
    """a numpy array as a device tensor of the handle's compute dtype (what the device then holds, exactly)"""
    t = _torch()
    if a.dtype == np.uint8 or a.dtype == bool:
        return t.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    return t.from_numpy(np.ascontiguousarray(a.astype(np.float32 if c.dtype == "f32" else np.float64))).to("cuda:0")


def held(c, a):
    return a.astype(np.float32).astype(np.float64) if c.dtype == "f32" else a


def host(*ts):
    _torch().cuda.synchronize()
    return tuple(x.cpu().numpy().astype(np.float64) if x.dtype.is_floating_point else x.cpu().numpy() for x in ts)


def gated(c, io, u, z, chi2, mask=None):
    acc, nis, nu, S = host(*io.tick(dev(c, u), dev(c, z), None if mask is None else dev(c, mask), chi2_max=chi2, return_nis=True))
    return acc.astype(bool), nis, nu, S


def reference(c, u, z, mask=None):
    xd, Pd = c.ekf.get_state()
    return predict_then_innovation(c.po, c.p, xd, Pd, held(c, u), held(c, z), c.pfp, mask=mask)


# ------------------------------------------------------------------------------------------------ 1. oracle agreement
@pytest.mark.parametrize("batch", [64 * 4 + 17, RAGGED])
@grid
def test_gated_tick_matches_oracle_predict_then_restatement(dtype, direct, est_bias, use_pfp, batch):
    c = Case(dtype, direct, est_bias, use_pfp, batch=batch)
    io = qla.DeviceIO(c.ekf)
    nur, Sr, nisr, _, _ = reference(c, c.u, c.z)
    acc, nis, nu, S = gated(c, io, c.u, c.z, 40.0)
    tol = TOL[dtype]
    e_nu, e_S, e_nis = rel(nu, nur), rel(S, Sr), float(np.abs(nis / nisr - 1).max())
    print(f"{dtype} B={batch}: worst relative nu {e_nu:.2e} S {e_S:.2e} nis {e_nis:.2e}; NIS range {nisr.min():.3g} .. {nisr.max():.3g}")
    assert np.isfinite(nis).all() and np.array_equal(S, S.transpose(0, 2, 1))
    assert e_nu < tol["nu"] and e_S < tol["S"] and e_nis < tol["nis"], (e_nu, e_S, e_nis)
    clear = clear_of_threshold(nisr, 40.0)
    assert np.array_equal(acc[clear], (nisr <= 40.0)[clear]) and acc.any() and (~acc).any()
    c.close()


@grid
def test_innovation_from_tensors_matches_restatement_and_host_path(dtype, direct, est_bias, use_pfp):
    c = Case(dtype, direct, est_bias, use_pfp, batch=RAGGED)
    io = qla.DeviceIO(c.ekf)
    mask = (c.rng.uniform(size=c.B) < 0.8).astype(np.uint8)
    nu, S, nis = host(*io.innovation(dev(c, c.z), dev(c, mask)))
    nur, Sr, nisr = c.ref(c.z, mask)
    tol = TOL[dtype]
    live = mask != 0
    assert rel(nu, nur) < tol["nu"] and rel(S, Sr) < tol["S"] and float(np.abs(nis[live] / nisr[live] - 1).max()) < tol["nis"]
    assert np.isnan(nis[~live]).all() and not nu[~live].any() and not S[~live].any()
    c.close()


# ------------------------------------------------------------------------------------------------ 2. no state write
@grid
def test_gate_kernel_writes_no_state_word(dtype, direct, est_bias, use_pfp):
    t = _torch()
    c = Case(dtype, direct, est_bias, use_pfp, batch=RAGGED)
    io = qla.DeviceIO(c.ekf)
    x0, P0 = host(*io.state())
    io.innovation(dev(c, c.z))
    io.innovation(dev(c, c.z), dev(c, (c.rng.uniform(size=c.B) < 0.5).astype(np.uint8)))
    x1, P1 = host(*io.state())
    assert _same(x0, x1) and _same(P0, P1)
    # qgt_gate_tick alone, through the binding: pack, gate, no tick
    D, G = devio.devio_lib(), gate.gate_lib()
    view, iv = io._view(), io._inputs_view(1)
    u, z = dev(c, c.u), dev(c, c.z)
    acc = t.zeros(c.B, dtype=t.uint8, device="cuda:0"); nis = t.zeros(c.B, dtype=u.dtype, device="cuda:0")
    stream = int(t.cuda.current_stream().cuda_stream)
    devio._dcheck(D.qdv_wait_stream(C.byref(view), stream))
    devio._dcheck(D.qdv_pack_inputs(C.byref(view), C.byref(iv), u.data_ptr(), z.data_ptr(), None, devio._FLOATS[str(u.dtype).split(".")[-1]]))
    gate.gcheck(G.qgt_gate_tick(C.byref(view), C.byref(iv), C.byref(c.ekf.params), CHI2_6_099, nis.data_ptr(), acc.data_ptr(), None, None,
                                devio._FLOATS[str(u.dtype).split(".")[-1]]))
    devio._dcheck(D.qdv_signal_stream(C.byref(view), stream))
    x2, P2 = host(*io.state())
    assert _same(x0, x2) and _same(P0, P2)
    a, = host(acc)
    assert a.any() and not a.all()
    # the mask words of the slot are what the gate left: accepted
    _, _, m = io._seq.download_tick(1)
    assert np.array_equal(m != 0, a != 0)
    c.close()


# ------------------------------------------------------------------------------------------------ 3. an infinite threshold
@grid
def test_infinite_threshold_is_the_ungated_tick(dtype, direct, est_bias, use_pfp):
    c = Case(dtype, direct, est_bias, use_pfp, batch=RAGGED)
    io = qla.DeviceIO(c.ekf)
    mask = (c.rng.uniform(size=c.B) < 0.8).astype(np.uint8)
    io.tick(dev(c, c.u), dev(c, c.z), dev(c, mask))
    xu, Pu = c.ekf.get_state()
    c.reset()
    acc, nis, _, _ = gated(c, io, c.u, c.z, np.inf, mask)
    xg, Pg = c.ekf.get_state()
    assert np.isfinite(nis[mask != 0]).all() and np.isnan(nis[mask == 0]).all()
    assert np.array_equal(acc, mask != 0)
    assert _same(xu, xg) and _same(Pu, Pg)
    c.close()


# ------------------------------------------------------------------------------------------------ 4. displaced tag poses
@grid
def test_gate_rejects_displaced_tag_poses(dtype, direct, est_bias, use_pfp):
    c = Case(dtype, direct, est_bias, use_pfp, batch=RAGGED, cov_scale=0.05)
    io = qla.DeviceIO(c.ekf)
    xd, Pd = c.ekf.get_state()
    xp, _ = predict_then_innovation(c.po, c.p, xd, Pd, held(c, c.u), c.z, c.pfp)[3:]
    z, out = displaced_tag_poses(c.rng, c.po, xp)
    _, _, nisr, _, _ = reference(c, c.u, z)
    clear = clear_of_threshold(nisr)
    assert (~clear).mean() <= 0.01
    acc, nis, _, _ = gated(c, io, c.u, z, CHI2_6_099)
    xg, Pg = c.ekf.get_state()
    assert np.array_equal(acc[clear], (nisr <= CHI2_6_099)[clear])
    assert acc[~out].mean() > 0.9 and acc[out].mean() < 0.1
    # bit for bit the ungated tick whose mask is `accepted`
    c.reset()
    io.tick(dev(c, c.u), dev(c, z), dev(c, acc.astype(np.uint8)))
    xu, Pu = c.ekf.get_state()
    assert _same(xu, xg) and _same(Pu, Pg)
    # the host path's three-launch gated tick decides the same and lands within the fused-versus-split tolerances
    c.reset()
    acc_h, nis_h = c.ekf.step_gated(held(c, c.u), held(c, z), CHI2_6_099)
    xh, Ph = c.ekf.get_state()
    assert np.array_equal(acc[clear], acc_h[clear])
    same = acc == acc_h
    assert same.mean() >= 0.99
    assert_state_close(xg[same], Pg[same], xh[same], Ph[same], **tp.UPD[dtype])
    c.close()


# ------------------------------------------------------------------------------------------------ 5. excluded filters
@grid
def test_masked_uninitialised_and_indefinite_filters_are_excluded(dtype, direct, est_bias, use_pfp):
    c = Case(dtype, direct, est_bias, use_pfp)
    seeded = (c.rng.uniform(size=c.B) < 0.7).astype(np.uint8)
    seeded[:64] = 1
    c.ekf.set_state(np.zeros((c.B, 16)), np.zeros((c.B, c.n, c.n)))
    c.ekf.initialize_state(c.z, mask=seeded)
    x0, P0 = c.ekf.get_state()
    indef = np.zeros(c.B, bool); indef[np.flatnonzero(seeded)[3::11]] = True
    P0[indef] = -10.0 * P0[indef]                       # S = G P G^T + R_k is then not positive definite
    c.ekf.set_state(np.where(seeded[:, None] != 0, x0, 0.0), P0)
    x0, P0 = c.ekf.get_state()
    assert np.array_equal(c.ekf.state_initialized(), seeded)
    io = qla.DeviceIO(c.ekf)
    zm = meas_near(c.rng, c.po, x0, ang=0.1, pos=0.05)
    mask = (c.rng.uniform(size=c.B) < 0.6).astype(np.uint8)
    live = (mask != 0) & (seeded != 0) & ~indef
    acc, nis, nu, S = gated(c, io, c.u, zm, CHI2_6_099 * 1e6, mask)
    x1, P1 = c.ekf.get_state()
    assert not acc[~live].any() and acc[live].all()
    assert np.isnan(nis[~live]).all() and np.isfinite(nis[live]).all()
    off = (mask == 0) | (seeded == 0)
    assert not nu[off].any() and not S[off].any()
    # filters without state are untouched; every excluded filter is exactly where the tick without its tag pose leaves it
    assert _same(x1[seeded == 0], x0[seeded == 0]) and _same(P1[seeded == 0], P0[seeded == 0])
    c.ekf.set_state(x0, P0)
    io.tick(dev(c, c.u), dev(c, zm), dev(c, live.astype(np.uint8)))
    x2, P2 = c.ekf.get_state()
    assert _same(x1, x2) and _same(P1, P2)
    c.close()


# ------------------------------------------------------------------------------------------------ 6. wave neighbours
@pytest.mark.parametrize("kind", ["state_nan", "state_inf", "uninit", "corr170", "zero_tag", "huge_tag"])
@grid
def test_filters_independent_of_wave_neighbours(dtype, direct, est_bias, use_pfp, kind):
    c = Case(dtype, direct, est_bias, use_pfp, batch=BW)
    io = qla.DeviceIO(c.ekf)
    z = meas_near(c.rng, c.po, c.x, ang=0.3, pos=0.05)
    xd, Pd, zd = c.x.copy(), c.P.copy(), z.copy()
    if kind == "state_nan":
        xd[DIST] = np.nan; Pd[DIST] = np.nan
    elif kind == "state_inf":
        xd[DIST, 0:3] = np.inf; Pd[DIST, 0, 0] = np.inf
    elif kind == "uninit":
        xd[DIST] = 0.0
    elif kind == "corr170":
        Pd[DIST] *= 10.0
        zd[DIST] = rot_z(meas_near(c.rng, c.po, c.x[DIST], ang=0.0, pos=0.05), BIG, c.rng)
    elif kind == "zero_tag":
        zd[DIST] = 0.0
    elif kind == "huge_tag":
        zd[DIST, 0:3] = 1e30

    def run(x, P, zz):
        c.reset(x, P)
        nu, S, nis = host(*io.innovation(dev(c, zz)))
        acc, nis_g, nu_g, S_g = gated(c, io, c.u, zz, CHI2_6_099)
        xs, Ps = c.ekf.get_state()
        return dict(nu=nu, S=S, nis=nis, acc=acc, nis_g=nis_g, nu_g=nu_g, S_g=S_g, x=xs, P=Ps)

    base = run(c.x, c.P, z)
    dist = run(xd, Pd, zd)
    for k in base:
        assert _same(base[k][HEALTHY], dist[k][HEALTHY]), (kind, k)
    ok = np.isfinite(dist["nis_g"][DIST]) & (dist["nis_g"][DIST] <= CHI2_6_099)
    assert not (dist["acc"][DIST] & ~ok).any()
    if kind in ("state_nan", "uninit", "zero_tag"):
        assert not dist["acc"][DIST].any() and np.isnan(dist["nis_g"][DIST]).all()
    if kind == "huge_tag":
        assert not dist["acc"][DIST].any()
    c.close()


# ------------------------------------------------------------------------------------------------ 7. with the device decision logic
@grid
def test_gate_in_front_of_the_device_decision_logic(dtype, direct, est_bias, use_pfp):
    """limit_measurement_freq with upd_per_meas = 4: tag poses on ticks 4, 5, 6 and 9.  A tag pose the gate rejects is no detection:
    it is not consumed and does not reset upds_since_correction, so such a filter may correct on the next tick, while a filter that
    corrected is rate-limited.  (corner_margin_enbl is off: random tag poses do not project into the image.)"""
    c = Case(dtype, direct, est_bias, use_pfp, cov_scale=0.05)
    c.ekf.initialize_params(update_freq=400.0, measurement_freq=100.0, limit_measurement_freq=1, corner_margin_enbl=0)
    c.reset()
    assert c.ekf.derived.upd_per_meas == 4
    c.ekf.enable_gating(True)
    io = qla.DeviceIO(c.ekf)
    upds = np.zeros(c.B, np.int64)
    seen_limited = seen_retry = False
    rejected_before = np.zeros(c.B, bool)
    for k in range(10):
        u = rand_imu(c.rng, c.B)
        if k not in (4, 5, 6, 9):
            io.tick(dev(c, u))
            upds += 1
            continue
        xd, Pd = c.ekf.get_state()
        xp = predict_then_innovation(c.po, c.p, xd, Pd, held(c, u), c.z, c.pfp)[3]
        z, _ = displaced_tag_poses(c.rng, c.po, xp, frac=0.5)
        ready = (c.rng.uniform(size=c.B) < 0.8).astype(np.uint8)
        _, _, nisr, _, _ = predict_then_innovation(c.po, c.p, xd, Pd, held(c, u), held(c, z), c.pfp)
        clear = clear_of_threshold(nisr)
        acc, nis, _, _ = gated(c, io, u, z, CHI2_6_099, ready)
        assert np.array_equal(acc[clear], ((ready != 0) & (nisr <= CHI2_6_099))[clear])
        pc, co, up = c.ekf.tick_flags()
        consume = acc & (upds + 1 >= 4)          # ready = ready && accepted (EKF.cpp:147)
        perform = consume                        # no corner gate
        upds = np.where(perform, 0, upds + 1)
        assert np.array_equal(pc != 0, perform) and np.array_equal(co != 0, consume) and np.array_equal(up, upds)
        seen_limited |= bool((acc & ~consume).any())
        seen_retry |= bool((perform & rejected_before).any())
        rejected_before = (ready != 0) & ~acc
    assert seen_limited and seen_retry
    c.close()


# ------------------------------------------------------------------------------------------------ 8. launch census
@grid
def test_one_gate_launch_and_one_tick_kernel(dtype, direct, est_bias, use_pfp):
    c = Case(dtype, direct, est_bias, use_pfp, batch=RAGGED)
    io = qla.DeviceIO(c.ekf)
    u, z = dev(c, c.u), dev(c, c.z)
    io.tick(u, z, chi2_max=CHI2_6_099)   # the private sequence exists now
    G = gate.gate_lib()
    n0 = G.qgt_launch_count()
    with qla.launch_census() as names:
        io.tick(u, z, chi2_max=CHI2_6_099)
    assert G.qgt_launch_count() - n0 == 1
    assert len(names) == 1 and "k_pregate" not in names[0], names
    with qla.launch_census() as ungated:
        io.tick(u, z)
    assert names == ungated
    c.ekf.synchronize()
    c.close()
