"""The chunked host <-> device staging of the tick library (quadrotor_landing_amd/csrc/ekf_capi.hip): every call that moves per-filter
rows through the handle's staging buffer walks the batch in chunks of at most kStageFilters = 32 768 filters.

Every staged call is per filter, so a large batch built by tiling a small one must return the tiled small result bit for bit,
whatever the chunking.  B = 32 769 = kStageFilters + 1 is two chunks, the second holding one filter; B0 = 97 is a ragged tile; the
inputs of the large handle are np.resize of the 97 rows.  est_bias = 1 has the 15 x 15 P whose 225-double stride makes the row
packer's chunk exactly kStageFilters; est_bias = 0 has compact records.  No tolerance appears: every comparison is equality of bits.

Both handles run the lane-per-filter kernels (QLE_QUAD=0): left alone, the 97-filter handle would take the workgroup-cooperative
tick kernel that a 32 769-filter handle never does, and the comparison would be one of kernels, not of staging.

Not covered: the hipMalloc fallback of qle_get_tick_flags, taken when the batch's int32 counters do not fit the staging buffer,
needs more than 14 million filters.
"""
import numpy as np
import pytest

import quadrotor_landing_amd as qla
from test_gpu_devio import KW, assert_same_bits, rand_imu, rand_pose

pytestmark = pytest.mark.gpu

B0, B = 97, 32769          # B = kStageFilters + 1 (ekf_host.hpp)


def tiled(a):
    a = np.asarray(a)
    return np.resize(a, (B,) + a.shape[1:])


def inputs(est_bias):
    """The rows of the small handle: states with and without a filter behind them, per-filter parameters, two ticks of inputs."""
    rng = np.random.default_rng(4200 + est_bias)
    n = 15 if est_bias else 9
    x = np.zeros((B0, 16)); P = np.zeros((B0, n, n))
    has = np.arange(B0) % 5 != 3                              # every fifth filter holds no state
    k = int(has.sum())
    x[has, 0:3] = rand_pose(rng, k)[:, :3]; x[has, 3:6] = 0.1 * rng.normal(size=(k, 3))
    x[has, 6:10] = rand_pose(rng, k)[:, 3:]
    if est_bias:
        x[has, 10:16] = 0.02 * rng.normal(size=(k, 6))
    A = 0.05 * rng.normal(size=(B0, n, n))
    P[has] = (A @ A.transpose(0, 2, 1) + 0.01 * np.eye(n))[has]
    d = dict(x=x, P=P, has=has)
    d["seed_z"] = rand_pose(rng, B0); d["seed_mask"] = (rng.uniform(size=B0) < 0.6).astype(np.uint8)
    d["u"] = rand_imu(rng, B0)
    d["z"] = d["seed_z"].copy(); d["z"][:, :3] += rng.normal(0.0, 0.01, (B0, 3))   # tag poses close to the ones the filters were seeded from
    d["mask"] = (rng.uniform(size=B0) < 0.7).astype(np.uint8)
    return d


def staged_calls(B_, dtype, est_bias, d, grow):
    """Every staged call once on a handle of B_ filters; `grow` makes the inputs of that handle from the 97 rows.  Returns what the
    calls gave back, by name."""
    ekf = qla.BatchedRelativePoseEKF(B_, dtype, est_bias=est_bias, limit_measurement_freq=0, **KW)
    out = {}
    pfp = np.tile(np.concatenate([list(ekf.derived.Q), KW["ab_static"], KW["wb_static"], list(ekf.derived.R)]), (B0, 1))
    pfp *= 1.0 + 0.1 * np.random.default_rng(7).uniform(size=pfp.shape)
    # initialize_state(mask=...) -> state_initialized, on a handle that holds no state yet
    ekf.initialize_state(grow(d["seed_z"]), mask=grow(d["seed_mask"]))
    out["seeded.state_initialized"] = ekf.state_initialized()
    out["seeded.x"], out["seeded.P"] = ekf.get_state()
    # set_state -> get_state
    ekf.set_state(grow(d["x"]), grow(d["P"]))
    out["x"], out["P"] = ekf.get_state()
    out["state_initialized"] = ekf.state_initialized()
    ekf.set_state(out["seeded.x"], out["seeded.P"])           # back to the seeded state, which the tag poses below belong to
    # set_filter_params -> get_filter_params
    ekf.set_filter_params(grow(pfp))
    out["pfp"] = ekf.get_filter_params()
    # upload_tick -> download_tick
    seq = ekf.make_inputs(2, [0, 1])
    seq.upload_tick(0, grow(d["u"]))
    seq.upload_tick(1, grow(d["u"]), grow(d["z"]), grow(d["mask"]))
    out["tick0.u"], _, out["tick0.mask"] = seq.download_tick(0)
    out["tick1.u"], out["tick1.z"], out["tick1.mask"] = seq.download_tick(1)
    for k, v in ekf.report().items():
        out[f"report.{k}"] = v
    out["innov.nu"], out["innov.S"], out["innov.nis"] = ekf.innovation(grow(d["z"]), grow(d["mask"]))
    acc, out["gated.nis"] = ekf.update_gated(grow(d["z"]), 16.81, grow(d["mask"]))
    out["gated.accepted"] = acc.astype(np.uint8)
    # one filter_update tick with tag poses, gating and side outputs on
    ekf.enable_gating(True); ekf.enable_aux(True)
    ekf.filter_update(grow(d["u"]), grow(d["z"]), grow(d["mask"]))
    out["flags.performed"], out["flags.consumed"], out["flags.upds_since"] = ekf.tick_flags()
    out["aux.accel"], out["aux.obs"] = ekf.get_aux()
    node = ekf.node_report()
    for name in node.dtype.names:
        out[f"node.{name}"] = np.ascontiguousarray(node[name])
    assert ekf.count_nonfinite() == 0
    seq.close(); ekf.close()
    return out


@pytest.mark.parametrize("est_bias", [1, 0], ids=["bias", "no-bias"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_a_tiled_batch_returns_the_tiled_result(dtype, est_bias, monkeypatch):
    monkeypatch.setenv("QLE_QUAD", "0")
    d = inputs(est_bias)
    small = staged_calls(B0, dtype, est_bias, d, lambda a: a)
    large = staged_calls(B, dtype, est_bias, d, tiled)
    # the small run exercised what the comparison is about
    live = (d["seed_mask"] != 0) & (d["mask"] != 0)
    assert np.array_equal(small["seeded.state_initialized"], d["seed_mask"]) and np.array_equal(small["state_initialized"] != 0, d["has"])
    assert np.array_equal(small["tick1.mask"] != 0, d["mask"] != 0) and np.array_equal(small["pfp"].shape, (B0, 24))
    assert np.isfinite(small["innov.nis"][live]).all() and np.isnan(small["innov.nis"][~live]).all()
    assert small["gated.accepted"].any()
    assert small["flags.performed"].any() and small["aux.obs"].any() and small["node.performed_correction"].any()
    assert sorted(small) == sorted(large)
    for name in small:
        assert large[name].shape[0] == B, name
        assert_same_bits(large[name], tiled(small[name]), f"{dtype} est_bias={est_bias} {name}")
