"""The error budget on the GPU (include/qle_budget.h, libqle_budget.so: k_budget, k_budget_reduce; DeviceRecords.budget,
DeviceIO.budget_run, BatchedRelativePoseEKF.error_budget).  Every row of tests/budget_variant_table.py runs.

B = 165: two full tiles and a ragged one of 37 -- both half-wave swaps, a group boundary and the ragged end.  Inputs:
budget_variant_table.Inputs (consistency_util.make_case, a mask with the first tile on and mixed bits elsewhere, one all-zero record,
one filter with a NaN covariance word), held to their conditions on the CPU.

The sums are compared EXACTLY.  The 256 words of every filter are formed in numpy from the call's own err (returned as float64), its
status, and state(dtype=float64) -- all three exact images of the device words -- and reduced by budget_variant_table.tile_sum (the
xor-butterfly of wave_sum, by definition a tile's field) and, per group, from left to right from +0.0.  No tolerance is involved.
err itself is held to consistency_util.err_ref under err_ratio <= 1, the bar k_nees's own err is held to; both worst ratios on the same
inputs are printed (tests/tolerances_budget.md).
"""
import numpy as np
import pytest

import budget_variant_table as bv
import consistency_util as cu
import quadrotor_landing_amd as qla
import side_variant_table as st
from quadrotor_landing_amd import budget
from test_gpu_side_variants import Handle, dev, host

pytestmark = pytest.mark.gpu

B = bv.B


@pytest.fixture(autouse=True)
def torch_first():
    """torch is imported before the first handle of a test exists: a torch that is first imported after the engine has initialised the
    HIP runtime reports no GPU."""
    import torch
    return torch


def row_of(dtype, record="full15", pfp=False):
    return next(r for r in bv.ROWS if r["dtype"] == dtype and r["record"] == record and r["pfp"] == pfp)


def call(rec, xt, mask, group_tiles=None):
    """One budget call with every output -> (sums, err as float64, status) on the host"""
    b = rec.budget(xt, mask=mask, group_tiles=group_tiles, return_err=True, return_status=True, dtype="float64")
    return host(b.sums, b.err, b.status)


def partials_of(rec, err, status):
    """The exact reference: the tile partials [tiles,256] from the call's err and status and the view's own state, as float64"""
    _, P = host(*rec.state(dtype="float64"))
    return bv.tile_partials(bv.words_ref(err, status, P))


def check_exact(rec, xt, mask, what):
    """Checks 3 and 4 on any view: group_tiles = 1 gives the tile sums, None and 2 their left-to-right sums.  -> (partials, err, status)"""
    sums, err, status = call(rec, xt, mask, 1)
    part = partials_of(rec, err, status)
    bv.same_bits(sums, part, f"{what}: sums per tile against tile_sum of the 256 words")
    for gt in (None, 2):
        s, e, stt = call(rec, xt, mask, gt)
        bv.same_bits(s, bv.group_sums(part, gt), f"{what}: group_tiles={gt}")
        bv.same_bits(e, err, "err"); bv.same_bits(stt, status, "status")
    return part, err, status


# ------------------------------------------------------------------------------------------------ every row
@pytest.mark.parametrize("row", bv.ROWS, ids=[r["id"] for r in bv.ROWS])
def test_every_row(row, monkeypatch):
    d = bv.conditions(row)
    T, n = row["dtype"], st.RECORDS[row["record"]][0]
    h = Handle(row, d, monkeypatch)
    xt, mask = dev(d.xt, T), dev(d.mask)
    before = h.words()
    with budget.BUDGET.launch_census() as mine, qla.side_launch_census() as closed, qla.launch_census() as tick:
        sums, err, status = call(h.io, xt, mask, 1)
    got = {(bv.LIBRARY, st.kernel_id(k)) for k in mine}
    assert got == set(row["kernels"]), f"{row['id']}: launched {sorted(got)}, expected {sorted(row['kernels'])}"      # 8
    assert tick == [] and not any(closed.values()), (tick, closed)
    bv.same_bits(h.words(), before, "the record array behind the call")                                              # 7
    np.testing.assert_array_equal(status, d.status)                                                                  # 2
    live = d.status != bv.OFF
    xh, _ = h.ekf.get_state()
    eref = cu.err_ref(xh[live], d.xt[live], d.ab[live], d.wb[live], n)
    ratio = cu.err_ratio(err[live], eref, T)
    _, err_nees, _ = h.io.nees(xt, mask=mask, return_err=True, dtype="float64")
    err_nees = host(err_nees)[0]
    ratio_nees = cu.err_ratio(err_nees[live], eref, T)
    same = np.array_equal(err.view(np.uint64), err_nees.view(np.uint64))
    print(f"{row['id']}: err / bar k_budget {ratio:.3g}, k_nees {ratio_nees:.3g}, same bits {same}")
    assert err.shape == (B, n) and not err[~live].any()
    assert ratio <= 1.0, (ratio, ratio_nees)                                                                         # 1
    part, err2, status2 = check_exact(h.io, xt, mask, row["id"])                                                     # 3, 4
    bv.same_bits(sums, part, "a second call")                                                                        # 6
    bv.same_bits(err2, err, "a second call: err"); bv.same_bits(status2, status, "a second call: status")
    assert np.isfinite(part).all() and part[bv.NAN_FILTER // 64, 0] == (d.status[128:] == bv.COUNTED).sum()          # 5
    assert part[0, 0] == 64 and (part[:, 0] == [(d.status[t:t + 64] == bv.COUNTED).sum() for t in (0, 64, 128)]).all()
    if n == 9:
        assert not part[:, 10:16].any()
    h.close()


# ------------------------------------------------------------------------------------------------ once per dtype
@pytest.mark.parametrize("dtype", st.DTYPES)
def test_a_shard_of_whole_groups_reproduces_them(dtype, monkeypatch):
    """Additivity over shards: a handle over filters 64..164 alone gives groups 1 and 2 of the whole batch, bit for bit."""
    row = row_of(dtype, pfp=True)
    d = bv.conditions(row)
    h = Handle(row, d, monkeypatch)
    whole, _, _ = call(h.io, dev(d.xt, dtype), dev(d.mask), 1)
    h.close()
    s = Handle(row, d, monkeypatch, batch=B - 64, x=d.x[64:], P=d.P[64:], pfp=d.pfp[64:])
    shard, _, status = call(s.io, dev(d.xt[64:], dtype), dev(d.mask[64:]), 1)
    np.testing.assert_array_equal(status, d.status[64:])
    bv.same_bits(shard, whole[1:], "the shard's groups against groups 1 and 2 of the whole batch")
    both = budget.Budget.combine([budget.Budget(whole[0:1]), budget.Budget(bv.group_sums(shard, None))])   # tile 0 and the shard as one group
    assert both.n[0] == (d.status == bv.COUNTED).sum()
    s.close()


def test_a_group_longer_than_the_reduce_looks_ahead(monkeypatch):
    """k_budget_reduce issues the loads of 32 tiles together and finishes with single tiles: 37 tiles (2 341 filters, the last tile of 37)
    take both paths, one group and groups of 33 + 4; the sums stay the left-to-right sums, bit for bit."""
    row = row_of("f32")
    d = bv.conditions(row)
    nB = 36 * 64 + 37
    rng = np.random.default_rng(37)
    ab, wb = (np.broadcast_to(st.held("f32", np.array(st.HW[k])), (nB, 3)) for k in ("ab_static", "wb_static"))
    x, P, xt = cu.make_case(rng, nB, 15, "f32", ab, wb)
    mask = (rng.uniform(size=nB) < 0.7).astype(np.uint8)
    h = Handle(row, d, monkeypatch, batch=nB, x=x, P=P, pfp=None)
    xt_d, mask_d = dev(xt, "f32"), dev(mask)
    sums, err, status = call(h.io, xt_d, mask_d, 1)
    np.testing.assert_array_equal(status, mask)
    part = partials_of(h.io, err, status)
    assert part.shape == (37, 256)
    bv.same_bits(sums, part, "sums per tile")
    for gt in (None, 33, 32):
        bv.same_bits(call(h.io, xt_d, mask_d, gt)[0], bv.group_sums(part, gt), f"group_tiles={gt}")
    h.close()


@pytest.mark.parametrize("dtype", st.DTYPES)
def test_one_reference_row_is_the_row_expanded(dtype, monkeypatch):
    row = row_of(dtype)
    d = bv.conditions(row)
    h = Handle(row, d, monkeypatch)
    one = d.xt[5]
    mask = dev(d.mask)
    ref = call(h.io, dev(np.broadcast_to(one, (B, 16)), dtype), mask, 1)
    for shape in ((16,), (1, 16)):
        got = call(h.io, dev(one.reshape(shape), dtype), mask, 1)
        for g, r, name in zip(got, ref, ("sums", "err", "status")):
            bv.same_bits(g, r, f"x_true {shape}: {name}")
    assert np.abs(ref[1]).max() > 0
    h.close()


@pytest.mark.parametrize("dtype", st.DTYPES)
def test_forecast_snapshot_and_fused_views(dtype, monkeypatch):
    row = row_of(dtype)
    d = bv.conditions(row)
    h = Handle(row, d, monkeypatch)
    xt, mask = dev(d.xt, dtype), dev(d.mask)
    fc = h.io.lookahead(dev(d.u, dtype), 2)
    part, _, status = check_exact(fc, xt, mask, "Forecast.budget")
    assert status[d.ZERO] == bv.OFF and (status == bv.COUNTED).sum() * 2 >= B
    snap = h.io.snapshot()
    part_s, _, status_s = check_exact(snap, xt, mask, "Snapshot.budget")
    np.testing.assert_array_equal(status_s, d.status)
    bv.same_bits(part_s, check_exact(h.io, xt, mask, "the handle")[0], "a snapshot's budget against the handle's")
    h.close()
    M, G = 4, 41
    f = Handle(row, d, monkeypatch, batch=M * G, x=d.x[:M * G], P=d.P[:M * G])
    logw = dev(np.random.default_rng(3).normal(size=M * G))
    fused = f.io.bank(M).fuse(logw)
    assert fused.batch == G
    gmask = np.ones(G, np.uint8); gmask[7] = 0
    part_f, _, status_f = check_exact(fused, dev(d.xt[:M * G:M], dtype), dev(gmask), "Fused.budget")
    assert part_f.shape == (1, 256) and status_f[7] == bv.OFF and (status_f == bv.COUNTED).sum() >= G // 2
    f.close()


@pytest.mark.parametrize("dtype", st.DTYPES)
def test_budget_run_is_the_tick_loop_with_a_budget_every_fourth_tick(dtype, monkeypatch):
    """12 ticks, every = 4: every sums[j] carries the bits of a direct budget call at that tick of a per-tick `tick` loop, and the final
    state the bits of one `run` over the 12 ticks."""
    row = row_of(dtype)
    d = bv.conditions(row)
    K, every, tags = 12, 4, [2, 9]
    rng = np.random.default_rng(12)
    U = st.held(dtype, np.stack([st.rand_imu(rng, B) for _ in range(K)]))
    Z = st.held(dtype, np.stack([d.z, d.z + 0.01 * rng.normal(size=d.z.shape)]))
    Mk = np.stack([d.mask, 1 - d.mask]).astype(np.uint8)
    XT = st.held(dtype, np.stack([d.xt + 0.01 * j for j in range(K // every)]))
    Ud, Zd, Md, XTd, mask = dev(U, dtype), dev(Z, dtype), dev(Mk), dev(XT, dtype), dev(d.mask)
    a, b_, c = (Handle(row, d, monkeypatch) for _ in range(3))
    res = a.io.budget_run(a.io.sequence(Ud, Zd, tags, Md), XTd, every, mask=mask, group_tiles=2)
    assert tuple(res.sums.shape) == (K // every, 2, 256)
    sums = host(res.sums)[0]
    for k in range(K):
        if k in tags:
            b_.io.tick(Ud[k].clone(), Zd[tags.index(k)].clone(), Md[tags.index(k)].clone())
        else:
            b_.io.tick(Ud[k].clone())
        if (k + 1) % every == 0:
            j = k // every
            direct = host(b_.io.budget(XTd[j], mask=mask, group_tiles=2).sums)[0]
            bv.same_bits(sums[j], direct, f"sums[{j}] against a direct call after tick {k}")
    assert np.isfinite(sums).all() and (sums[:, :, 0] >= 2).all() and not np.array_equal(sums[0], sums[2])
    c.io.run(c.io.sequence(Ud, Zd, tags, Md))
    for got, want, name in zip(a.ekf.get_state(), c.ekf.get_state(), "xP"):
        bv.same_bits(got, want, f"{name} after budget_run against one run over the {K} ticks")
    for hh in (a, b_, c):
        hh.close()


@pytest.mark.parametrize("dtype", st.DTYPES)
def test_host_arrays_give_the_bits_of_the_tensor_call(dtype, monkeypatch):
    row = row_of(dtype, pfp=True)
    d = bv.conditions(row)
    h = Handle(row, d, monkeypatch)
    for gt in (None, 1):
        sums, err, status = call(h.io, dev(d.xt, "f64"), dev(d.mask), gt)
        hb = h.ekf.error_budget(d.xt, mask=d.mask, group_tiles=gt)
        bv.same_bits(hb.sums, sums, "sums"); bv.same_bits(hb.err, err, "err"); bv.same_bits(hb.status, status, "status")
    one = h.ekf.error_budget(d.xt[5], group_tiles=1)
    bv.same_bits(one.sums, call(h.io, dev(d.xt[5], "f64"), None, 1)[0], "one reference row")
    assert np.isfinite(hb.mean).all() and hb.var_ratio.shape == (3, 15) and (hb.n == [(d.status[t:t + 64] == 1).sum() for t in (0, 64, 128)]).all()
    h.close()
