"""The device-tensor boundary on the GPU (quadrotor_landing_amd/devio.py, libqle_devio.so): packing torch tensors into the tick
records, unpacking state and report into torch tensors, whole ticks, stream ordering and the launch census.  The kernels do no
arithmetic, so EVERY comparison here is exact equality of bits against the host path of include/qle_ekf.h; no tolerance appears.
"""
import ctypes as C

import numpy as np
import pytest

import quadrotor_landing_amd as qla
from quadrotor_landing_amd import _lib, devio

pytestmark = pytest.mark.gpu


def _torch():
    import torch as t
    return t


BATCHES = [2391, 4096, 65536 + 37]
KW = dict(update_freq=400.0, measurement_freq=30.0, direct_orien_method=1, Q_a=[0.0005] * 3, Q_w=[0.00005] * 3,
          R_r=[0.015, 0.015, 0.020], R_ang=[0.0015, 0.0015, 0.04], ab_static=[0.2, -0.09, -0.03], wb_static=[-0.02, -0.01, 0.003])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def assert_same_bits(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    same = bits(a) == bits(b)
    assert same.all(), f"{what}: {int((~same).sum())} of {same.size} words differ, first at {np.argwhere(~same)[0]}"


def dev(a, dtype=None):
    t = _torch()
    x = t.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        x = x.to(dtype)
    return x.to("cuda:0")


def rand_pose(rng, B):
    z = np.empty((B, 7))
    z[:, :3] = rng.uniform(-1.0, 1.0, (B, 3)) + [0.0, 0.0, 2.5]
    q = rng.normal(size=(B, 4)) * [0.1, 0.1, 0.1, 0.0] + [0.0, 0.0, 0.0, 1.0]
    z[:, 3:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    return z


def rand_imu(rng, B):
    return np.concatenate([rng.normal(0.0, 0.5, (B, 3)) + [0.0, 0.0, 9.8], rng.normal(0.0, 0.05, (B, 3))], axis=1)


# ------------------------------------------------------------------------------------------------ 1. pack
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("src", ["float32", "float64"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_pack_equals_upload_tick(dtype, src, B):
    """Device tensors packed into a sequence slot read back (download_tick) exactly as a twin slot filled by upload_tick with the same
    values (float32 sources widened to fp64 on the host first): without a tag slot, with z and a uint8 mask, with z and a bool mask,
    with z and no mask, and with neither (identity pose, all set)."""
    t = _torch()
    rng = np.random.default_rng(B + len(dtype + src))
    ekf = qla.BatchedRelativePoseEKF(B, dtype, **KW)
    D = devio.devio_lib()
    io = qla.DeviceIO(ekf)
    view = io._view()
    assert (view.batch, view.padded_batch, view.state_words, view.dtype) == (B, -(-B // 64) * 64, 144, ekf.dtype)
    T = 5
    mine, twin = ekf.make_inputs(T, [0, 1, 1, 1, 1]), ekf.make_inputs(T, [0, 1, 1, 1, 1])
    sd = getattr(t, src)
    for tick in range(T):
        u = rand_imu(rng, B).astype(src); z = rand_pose(rng, B).astype(src); m = (rng.uniform(size=B) < 0.5)
        zt = None if tick in (0, 4) else dev(z, sd)
        mt = None if tick in (0, 3, 4) else dev(m.astype(np.uint8) if tick == 1 else m)
        if tick == 2:
            assert mt.dtype == t.bool
        ut = dev(u, sd)
        iv = _lib.QleInputsView(); iv.struct_size = C.sizeof(iv)
        qla._lib.check(qla.lib().qle_inputs_get_device_view(mine._h, tick, C.byref(iv)))
        assert bool(iv.z) == (tick > 0) and iv.has_tag == (tick > 0)
        devio._dcheck(D.qdv_wait_stream(C.byref(view), int(t.cuda.current_stream().cuda_stream)))
        devio._dcheck(D.qdv_pack_inputs(C.byref(view), C.byref(iv), ut.data_ptr(), None if zt is None else zt.data_ptr(),
                                        None if mt is None else mt.data_ptr(), devio._FLOATS[src]))
        ident = np.tile([0, 0, 0, 0, 0, 0, 1.0], (B, 1))
        twin.upload_tick(tick, u.astype(np.float64), None if tick == 0 else (ident if tick == 4 else z.astype(np.float64)),
                         None if tick in (0, 3, 4) else m.astype(np.uint8))
        got, ref = mine.download_tick(tick), twin.download_tick(tick)
        for g, r, name in zip(got, ref, "uzm"):
            assert_same_bits(g, r, f"tick {tick} {name}")
        if tick in (3, 4):
            assert got[2].all()
    # a tick without a tag slot refuses z
    iv = _lib.QleInputsView(); iv.struct_size = C.sizeof(iv)
    qla._lib.check(qla.lib().qle_inputs_get_device_view(mine._h, 0, C.byref(iv)))
    assert D.qdv_pack_inputs(C.byref(view), C.byref(iv), ut.data_ptr(), ut.data_ptr(), None, devio._FLOATS[src]) == _lib.QLE_ERR_INVALID
    ekf.synchronize()
    ekf.close()


# ------------------------------------------------------------------------------------------------ 2. unpack
def _ticked_handle(B, dtype, est_bias, rng, pfp=False):
    ekf = qla.BatchedRelativePoseEKF(B, dtype, est_bias=est_bias, **KW)
    z0 = rand_pose(rng, B)
    seeded = rng.uniform(size=B) < 0.9
    seeded[-1] = False; seeded[0] = True
    ekf.initialize_state(z0, mask=seeded.astype(np.uint8))
    if pfp:
        p = np.tile(np.concatenate([list(ekf.derived.Q), KW["ab_static"], KW["wb_static"], list(ekf.derived.R)]), (B, 1))
        p[:, 12:18] += rng.normal(0.0, 0.05, (B, 6))
        ekf.set_filter_params(p)
    for k in range(6):
        if k == 3:
            z = z0.copy(); z[:, :3] += rng.normal(0.0, 0.01, (B, 3))
            ekf.step(rand_imu(rng, B), z, (rng.uniform(size=B) < 0.6).astype(np.uint8))
        else:
            ekf.step(rand_imu(rng, B))
    return ekf, seeded


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("est_bias", [1, 0])
@pytest.mark.parametrize("dst", ["float64", "float32"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_state_equals_get_state(dtype, dst, est_bias, B):
    t = _torch()
    ekf, seeded = _ticked_handle(B, dtype, est_bias, np.random.default_rng(7 * B + est_bias))
    compact = ekf.policy()["record_words"] == 64
    if est_bias:
        assert not compact
    elif B > 4096:
        assert compact   # the compact case cannot silently test full records (below, the handle chooses: full records on the cooperative kernels)
    n = 15 if est_bias else 9
    io = qla.DeviceIO(ekf)
    assert io._view().compact == int(compact) and io._view().num_states == n
    x, P = io.state(dtype=getattr(t, dst))
    assert x.dtype == getattr(t, dst) and tuple(P.shape) == (B, n, n) and x.device.index == 0
    t.cuda.current_stream().synchronize()
    xh, Ph = ekf.get_state()
    assert_same_bits(x.cpu().numpy(), xh.astype(dst), "x")
    assert_same_bits(P.cpu().numpy(), Ph.astype(dst), "P")
    Pn = P.cpu().numpy()
    assert_same_bits(Pn, np.ascontiguousarray(Pn.transpose(0, 2, 1)), "P symmetric")
    # filters never seeded come out as the host path reports them: all zero
    assert not x.cpu().numpy()[~seeded].any() and not Pn[~seeded].any() and np.abs(Pn[seeded]).sum() > 0
    # x alone, P alone, into given tensors
    x2 = t.full((B, 16), -1.0, dtype=getattr(t, dst), device="cuda:0"); P2 = t.full((B, n, n), -1.0, dtype=getattr(t, dst), device="cuda:0")
    D = devio.devio_lib(); view = io._view()
    devio._dcheck(D.qdv_wait_stream(C.byref(view), int(t.cuda.current_stream().cuda_stream)))
    devio._dcheck(D.qdv_unpack_state(C.byref(view), x2.data_ptr(), None, devio._FLOATS[dst]))
    devio._dcheck(D.qdv_unpack_state(C.byref(view), None, P2.data_ptr(), devio._FLOATS[dst]))
    ekf.synchronize()
    assert_same_bits(x2.cpu().numpy(), xh.astype(dst), "x alone")
    assert_same_bits(P2.cpu().numpy(), Ph.astype(dst), "P alone")
    x3, P3 = io.state(out=(x2.zero_(), P2.zero_()))
    t.cuda.current_stream().synchronize()
    assert x3 is x2 and P3 is P2
    assert_same_bits(P2.cpu().numpy(), Ph.astype(dst), "P out=")
    ekf.close()


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("est_bias", [1, 0])
@pytest.mark.parametrize("dst", ["float64", "float32"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_report_equals_get_report(dtype, dst, est_bias, B):
    t = _torch()
    ekf, _ = _ticked_handle(B, dtype, est_bias, np.random.default_rng(11 * B + est_bias), pfp=(B == 2391 and est_bias == 1))
    io = qla.DeviceIO(ekf)
    rep = io.report(dtype=getattr(t, dst))
    t.cuda.current_stream().synchronize()
    ref = ekf.report()
    assert sorted(rep) == sorted(ref)
    for k in ref:
        assert_same_bits(rep[k].cpu().numpy(), ref[k].astype(dst), k)
    assert np.abs(ref["bias"]).max() > 0.01   # the static biases are in it
    only = io.report(out={"vel": t.zeros((B, 3), dtype=getattr(t, dst), device="cuda:0")})
    t.cuda.current_stream().synchronize()
    assert list(only) == ["vel"]
    assert_same_bits(only["vel"].cpu().numpy(), ref["vel"].astype(dst), "vel alone")
    ekf.close()


# ------------------------------------------------------------------------------------------------ 3. whole ticks
MODES = {
    "explicit_masks": (dict(), False),
    "device_gating": (dict(limit_measurement_freq=1, corner_margin_enbl=1), True),
    "multirate_fixed_delay": (dict(multirate_ekf=1, measurement_delay=12 / 400.0, limit_measurement_freq=1, corner_margin_enbl=1), True),
}


def _recorded(B, dtype, kw, ticks, rng):
    """A generated 60-tick flight (tag poses every 4th tick), its seeded start state, and per-tick masks."""
    src = qla.BatchedRelativePoseEKF(B, dtype, **kw)
    thm = np.zeros(ticks, np.uint8); thm[3::4] = 1
    seq = src.make_inputs(ticks, thm)
    src.synth_generate(seq, seed=0xE4F00007, view_scale=0.3, meas_delay_ticks=12 if kw.get("multirate_ekf") else 0)
    x0, P0 = src.get_state()
    U, Z, M = [], [], []
    for k in range(ticks):
        u, z, m = seq.download_tick(k)
        U.append(u.astype(np.float32)); Z.append(z.astype(np.float32) if thm[k] else None)
        M.append((rng.uniform(size=B) < 0.7).astype(np.uint8) if thm[k] else None)
    src.close()
    return x0, P0, U, Z, M


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_ticks_from_tensors_equal_upload_and_run(dtype, mode):
    """Two handles with the same parameters and start state, 60 ticks: one by DeviceIO.tick from float32 torch tensors, one by
    upload_tick + run with the same values.  States and tick flags are identical afterwards.  A third handle driven by the host-buffer
    tick (step / filter_update) with the same values must agree as well: it launches the same kernels on the same records."""
    over, gating = MODES[mode]
    kw = dict(KW, **over)
    B, ticks = 2391, 60
    x0, P0, U, Z, M = _recorded(B, dtype, kw, ticks, np.random.default_rng(3))
    out = []
    for how in ("tensors", "upload_run", "host_step"):
        ekf = qla.BatchedRelativePoseEKF(B, dtype, **kw)
        ekf.set_state(x0, P0)
        if gating:
            ekf.enable_gating(True)
        io = qla.DeviceIO(ekf)
        seq = ekf.make_inputs(2, [0, 1])
        for k in range(ticks):
            if how == "tensors":
                io.tick(dev(U[k]), None if Z[k] is None else dev(Z[k]), None if Z[k] is None else dev(M[k]))
            elif how == "upload_run":
                s = 0 if Z[k] is None else 1
                seq.upload_tick(s, U[k].astype(np.float64), None if Z[k] is None else Z[k].astype(np.float64), M[k])
                ekf.run(seq, s, 1)
            elif gating:
                ekf.filter_update(U[k].astype(np.float64), None if Z[k] is None else Z[k].astype(np.float64), M[k])
            else:
                ekf.step(U[k].astype(np.float64), None if Z[k] is None else Z[k].astype(np.float64), M[k])
        x, P = ekf.get_state()
        flags = ekf.tick_flags() if gating else ()
        assert np.isfinite(x).all() and np.isfinite(P).all()
        out.append((x, P) + tuple(flags))
        ekf.close()
    assert np.abs(out[0][0] - x0).max() > 1e-3   # the ticks did something
    if gating:
        assert out[0][2].any() or out[0][4].max() > 0
    for other, name in ((out[1], "upload_tick + run"), (out[2], "host-buffer tick")):
        for a, b, what in zip(out[0], other, ("x", "P", "performed_correction", "consumed", "upds_since_correction")):
            assert_same_bits(a, b, f"{mode}: {what} against {name}")


# ------------------------------------------------------------------------------------------------ 4. stream ordering
def test_stream_ordering_without_synchronisation():
    """Inputs produced by a torch op on a non-default stream immediately before tick, outputs consumed by a torch reduction on that
    stream immediately after state(), no synchronisation in between: one pass of 200 ticks equals the synchronised run."""
    t = _torch()
    B, ticks, T = 65536, 200, 8
    rng = np.random.default_rng(17)
    kw = dict(KW)
    x0, P0, U, Z, M = _recorded(B, "f32", kw, T, rng)
    Ud = [dev(u) for u in U]; Zd = [None if z is None else dev(z) for z in Z]; Md = [None if m is None else dev(m) for m in M]
    res = []
    for sync in (False, True):
        ekf = qla.BatchedRelativePoseEKF(B, "f32", **kw)
        ekf.set_state(x0, P0)
        io = qla.DeviceIO(ekf)
        s = t.cuda.Stream(device=0)
        t.cuda.synchronize()
        with t.cuda.stream(s):
            acc = t.zeros(16, dtype=t.float64, device="cuda:0")
            for k in range(ticks):
                j = k % T
                u = Ud[j] * (1.0 + 1e-3 * (k // T))          # produced on s right before the tick
                z = None if Zd[j] is None else Zd[j] + 0.0
                io.tick(u, z, Md[j])
                del u, z
                x, P = io.state()
                acc += x.sum(dim=0, dtype=t.float64) + P.sum(dim=(0, 1), dtype=t.float64).sum() * 1e-3   # consumed on s right after
                del x, P
                if sync:
                    s.synchronize(); ekf.synchronize()
            xf, Pf = io.state()
        s.synchronize()
        res.append((acc.cpu().numpy(), xf.cpu().numpy(), Pf.cpu().numpy()))
        ekf.close()
    assert np.isfinite(res[0][0]).all() and np.abs(res[0][0]).max() > 0
    for a, b, what in zip(res[0], res[1], ("reduction", "x", "P")):
        assert_same_bits(a, b, what)


# ------------------------------------------------------------------------------------------------ 6. the main library is untouched
def test_census_names_only_the_tick_kernels():
    """DeviceIO.tick launches, in libqle_ekf.so, exactly the tick kernels qle_run launches and no k_pack* helper (its own kernels
    live in libqle_devio.so, which the census of the tick library does not see)."""
    B = 2391
    x0, P0, U, Z, M = _recorded(B, "f32", dict(KW), 4, np.random.default_rng(5))
    a = qla.BatchedRelativePoseEKF(B, "f32", **KW); b = qla.BatchedRelativePoseEKF(B, "f32", **KW)
    a.set_state(x0, P0); b.set_state(x0, P0)
    io = qla.DeviceIO(a)
    seq = b.make_inputs(2, [0, 1])
    seq.upload_tick(0, U[0].astype(np.float64)); seq.upload_tick(1, U[3].astype(np.float64), Z[3].astype(np.float64), M[3])
    ut, u3, z3, m3 = dev(U[0]), dev(U[3]), dev(Z[3]), dev(M[3])
    io.tick(ut)   # the private sequence exists now
    b.run(seq, 0, 1)
    with qla.launch_census() as mine:
        io.tick(ut); io.tick(u3, z3, m3)
        io.state(); io.report()
    with qla.launch_census() as ref:
        b.run(seq, 0, 1); b.run(seq, 1, 1)
    a.synchronize(); b.synchronize()
    assert mine == ref and len(mine) == 2, (mine, ref)
    assert not any("k_pack" in n or "k_unpack" in n or "k_report" in n for n in mine)
    assert_same_bits(a.get_state()[0], b.get_state()[0], "x")
    a.close(); b.close()
