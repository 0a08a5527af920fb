"""CPU tests of the look-ahead (include/qle_lookahead.h, libqle_lookahead.so, quadrotor_landing_amd/lookahead.py, csrc/ekf_lookahead.hpp):
the library builds, exports and binds what its header declares, its kernels are its own (none shared with, none added to, the five
existing libraries), its generated code passes the stale-EXEC audit, uses no scratch memory and no LDS and keeps the register counts its
launch bounds promise, every refusal is made before any GPU call (without a GPU a HIP call would fail with another error class), and the
per-filter body of k_lookahead -- lookahead_filter, compiled for the host with g++, once more under AddressSanitizer and UBSan -- agrees
with h applications of the dense oracle's predict.

Reference and bars: lookahead_util.py.  What the host build does not cover are the kernel's loads and stores, its masks and the view it
returns: tests/test_gpu_lookahead.py.

Measured on the host build (worst over the grid below, deviation / bar, bar = h x the per-step tolerance of tests/tolerances.md):
printed per case by test_host_compiled_forecast_matches_h_oracle_predicts (`pytest -s`).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import host_harness
import lookahead_util as lu
import side_lib_util
from elf_util import _kernels, _needed
from quadrotor_landing_amd import _lib, consistency, devio, gate, health, lookahead
from side_lib_util import (FakeTensor, _params, _view, assert_audit_counts, assert_exports_and_binds, ensure_built, kernel_descriptors,
                           run_audit, scratch_free)
from util import forbid_native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qle_lookahead.h")
N_KERNELS = 8   # k_lookahead: T x PFP x COMPACT


@pytest.fixture(scope="module")
def look_so():
    return ensure_built("lookahead")


# ---------------------------------------------------------------- 1. header, exports, kernels
def test_library_exports_and_binds_every_declared_function(look_so):
    _, txt = assert_exports_and_binds(lookahead, HEADER, "qlk", look_so,
                                      ["qlk_last_error", "qlk_launch_census_begin", "qlk_launch_census_end", "qlk_launch_count", "qlk_lookahead", "qlk_lookahead_host", "qlk_workspace_bytes"])
    body = re.search(r"typedef struct qlk_coast \{(.*?)\} qlk_coast;", txt, flags=re.S).group(1)
    assert re.findall(r"(?:uint32_t|double)\s+([a-z_]+);", body) == [n for n, _ in lookahead.QlkCoast._fields_]
    assert int(re.search(r"#define QLK_MAX_HORIZON (\d+)", txt).group(1)) == lookahead.MAX_HORIZON == 4096
    assert re.search(r"#define QLK_F32 0\b", txt) and re.search(r"#define QLK_F64 1\b", txt)
    assert (lookahead.QLK_F32, lookahead.QLK_F64) == (devio.QDV_F32, devio.QDV_F64) == (0, 1)


def test_kernels_are_disjoint_from_the_five_existing_libraries(look_so):
    mine = _kernels(look_so)
    others = {p: _kernels(p) for p in (_lib.LIB_PATH, devio.DEVIO_LIB_PATH, gate.GATE_LIB_PATH, consistency.CONSISTENCY_LIB_PATH, health.HEALTH_LIB_PATH)}
    assert mine and all(others.values())
    for p, k in others.items():
        assert not mine & k, (p, sorted(mine & k))
        assert not any("k_lookahead" in _lib.demangle(m) for m in k), p
    ids = {_lib.demangle(m) for m in mine}
    assert all(i.startswith("void qle::k_lookahead<") for i in ids), sorted(ids)
    assert len(ids) == N_KERNELS
    assert {re.match(r"void qle::k_lookahead<(\w+), (\w+), (\w+)>", i).groups() for i in ids} == {
        (t, f, c) for t in ("float", "double") for f in ("true", "false") for c in ("true", "false")}


def test_library_links_the_hip_runtime_and_the_tick_library_only(look_so):
    needed = _needed(look_so)
    assert any(n.startswith("libamdhip64") for n in needed), needed
    assert [n for n in needed if "qle_" in n] == ["libqle_ekf.so"], needed   # qle_params_derive, as the gate library
    assert not any("oracle" in n for n in needed), needed


# ---------------------------------------------------------------- 2. audit and resources
@pytest.fixture(scope="module")
def audit(look_so):
    return run_audit("lookahead")


def test_generated_device_code_passes_the_stale_exec_audit(audit):
    assert_audit_counts(audit[0], "lookahead", N_KERNELS)


def test_no_kernel_uses_scratch_memory_or_lds_and_the_registers_fit(audit):
    """The kernel descriptors of the generated assembly: 0 bytes of private segment and no LDS for every kernel, and the register
    counts the launch bounds promise -- fp32 within the 256 registers that leave room for two waves per SIMD, fp64 within 512."""
    r, asm = audit
    assert r.returncode == 0
    found, meta = kernel_descriptors(asm)
    assert len(found) == N_KERNELS and all("k_lookahead<" in k for k in found), sorted(found)
    for name, (scratch, lds, vgpr) in found.items():
        print(f"{name.split('(')[0]}: scratch {scratch} B, LDS {lds} B, registers {vgpr}")
        assert scratch == 0, (name, scratch)
        assert lds == 0, (name, lds)
        assert vgpr <= (256 if "k_lookahead<float" in name else 512), (name, vgpr)
    assert scratch_free(meta), meta


# ---------------------------------------------------------------- 3. refusals, before any GPU call
def _coast(r=1.0, th=0.5):
    c = lookahead.QlkCoast()
    c.struct_size = C.sizeof(c); c.sigma_r_max = r; c.sigma_theta_max = th
    return c


def test_library_refuses_before_any_gpu_call(look_so):
    """No GPU here: a call that got as far as the HIP runtime would return QLE_ERR_HIP (or crash on the fake pointers), not these."""
    K = lookahead.lookahead_lib()
    B = C.byref
    INV = _lib.QLE_ERR_INVALID
    v, p, coast, ahead = _view(), _params(), _coast(), _lib.QleDeviceView()
    need = K.qlk_workspace_bytes(B(v))
    assert need == 128 * 144 * 4 and K.qlk_workspace_bytes(B(_view(dtype=_lib.QLE_F64, batch=64))) == 64 * 144 * 8
    U, WS, TK, MK = 0x7F1000000000, 0x7F2000000000, 0x7F3000000000, 0x7F4000000000

    def call(v_=B(v), p_=B(p), u=U, ud=lookahead.QLK_F32, h=8, mask=MK, ws=WS, nb=need, ahead_=B(ahead), coast_=B(coast), tk=TK):
        return K.qlk_lookahead(v_, p_, u, ud, h, mask, ws, nb, ahead_, coast_, tk)

    err = lambda: K.qlk_last_error()
    assert call(v_=None) == INV and b"view" in err()
    assert call(p_=None) == INV and b"params" in err()
    for size in (0, C.sizeof(v) - 8, C.sizeof(v) + 8):                      # a wrong struct_size: the view
        bad = _view(); bad.struct_size = size
        assert call(v_=B(bad)) == INV and b"struct_size" in err()
        assert K.qlk_workspace_bytes(B(bad)) == INV
    for size in (0, C.sizeof(coast) - 8, C.sizeof(coast) + 8):              # ... and the limits
        bad = _coast(); bad.struct_size = size
        assert call(coast_=B(bad)) == INV and b"struct_size" in err()
    odd = _view(); odd.state = 0x7F0000000008                                # misaligned pointers
    assert call(v_=B(odd)) == INV and b"aligned" in err()
    assert call(u=U + 8) == INV and b"aligned" in err()
    assert call(ws=WS + 8) == INV and b"aligned" in err()
    assert call(tk=TK + 2) == INV and b"aligned" in err()
    for h in (-1, lookahead.MAX_HORIZON + 1, 2 ** 31 - 1, -2 ** 31):         # h out of range
        assert call(h=h) == INV and b"horizon" in err()
    assert call(nb=need - 1) == INV and b"too small" in err()                # a workspace that is too small
    assert call(nb=0) == INV and call(ws=None) == INV
    for ws in (v.state, v.state + need - 16, v.state - need + 16, v.state + 16):   # ... or overlaps view->state
        assert call(ws=ws) == INV and b"overlaps" in err(), hex(ws)
    assert call(ws=v.state - 4 * need, nb=5 * need + 16) == INV and b"overlaps" in err()   # a larger workspace around the state
    assert call(u=None) == INV and b"u is null" in err()                     # u == NULL
    assert call(coast_=None) == INV and b"both" in err()                     # one of coast / ticks_to_limit without the other
    assert call(tk=None) == INV and b"both" in err()
    for field in ("sigma_r_max", "sigma_theta_max"):                          # a limit that is not > 0, NaN included
        for val in (0.0, -1.0, float("nan"), float("-inf")):
            bad = _coast(); setattr(bad, field, val)
            assert call(coast_=B(bad)) == INV and field.encode() in err(), (field, val)
    assert call(ud=7) == INV and b"u_dtype" in err()
    assert call(ahead_=None) == INV and b"ahead" in err()
    for wrong in (dict(dtype=7), dict(n=12), dict(batch=0), dict(n=15, compact=1)):
        assert call(v_=B(_view(**wrong))) == INV
    assert call(p_=B(_params(est_bias=0))) == INV and b"est_bias" in err()   # the view says 15 states
    # the host entry refuses the same, before it allocates anything
    u = np.zeros((100, 6)); tk = np.zeros(100, np.int32)
    pu, pt = u.ctypes.data_as(C.POINTER(C.c_double)), tk.ctypes.data_as(C.POINTER(C.c_int32))
    host = lambda h=8, ws=WS, nb=need, coast_=B(coast), tk_=pt, u_=pu: K.qlk_lookahead_host(B(v), B(p), u_, h, None, ws, nb, B(ahead), coast_, tk_)
    assert host(h=-1) == INV and host(h=4097) == INV and host(nb=need - 1) == INV and host(ws=v.state) == INV
    assert host(coast_=None) == INV and host(tk_=None) == INV and host(u_=None) == INV and host(ws=WS + 4) == INV
    assert K.qlk_launch_count() == 0


class FakeEkf(side_lib_util.FakeEkf):
    def __init__(self, **kw):
        self.params = _params(**kw)


def test_deviceio_refuses_bad_lookahead_arguments_before_any_gpu_call(monkeypatch):
    ekf = FakeEkf()   # its parameters come from the tick library: made first
    forbid_native(monkeypatch)
    B = 100
    io = devio.DeviceIO(ekf)
    u, m = FakeTensor((B, 6)), FakeTensor((B,), dtype="uint8")
    for bad_u in (np.zeros((B, 6)), FakeTensor((B, 7)), FakeTensor((B, 6), dtype="float16"), FakeTensor((B, 6), device="cuda:1"),
                  FakeTensor((B, 6), device="cpu"), FakeTensor((B, 6), contiguous=False), FakeTensor((B, 6), ptr=0x7F0000000008)):
        with pytest.raises(ValueError):
            io.lookahead(bad_u, 4)
    for bad_m in (np.zeros(B, np.uint8), FakeTensor((B,), dtype="float32"), FakeTensor((B, 1), dtype="uint8"), FakeTensor((B,), dtype="uint8", device="cuda:1")):
        with pytest.raises(ValueError):
            io.lookahead(u, 4, mask=bad_m)
    for bad_h in (-1, lookahead.MAX_HORIZON + 1, 2.5, True, 10 ** 12):
        with pytest.raises(ValueError):
            io.lookahead(u, bad_h)
    for kw in (dict(sigma_r_max=0.0), dict(sigma_r_max=-1.0), dict(sigma_theta_max=float("nan")), dict(sigma_theta_max=float("-inf"))):
        with pytest.raises(ValueError):
            io.lookahead(u, 4, **kw)
    for good in (lambda: io.lookahead(u, 0), lambda: io.lookahead(u, lookahead.MAX_HORIZON, mask=m, sigma_r_max=2.0)):
        with pytest.raises(AssertionError, match="native library"):
            good()   # a good call is what reaches the libraries
    assert lookahead.make_coast() is None and lookahead.make_coast(sigma_theta_max=0.5).sigma_r_max == float("inf")


# ---------------------------------------------------------------- 4. the arithmetic on the host, 5. once more under the sanitizers
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/cpp/lookahead_harness.cpp: ekf_lookahead.hpp's lookahead_filter compiled by g++ (the HIP headers define the device
    decorators away), once as it is and once as a stand-alone program under AddressSanitizer and UBSan."""
    return host_harness.build("lookahead_harness", tmp_path_factory)


def run_harness(exe, tmp, po, dtype, compact, h, x, P, u, pfp, asked=None, sigma_r_max=np.inf, sigma_theta_max=np.inf):
    B, n = x.shape[0], po.num_states
    hdr = [B, int(dtype == "f64"), int(compact), int(pfp is not None), h, sigma_r_max, sigma_theta_max, *host_harness.params_header(po)]
    on = np.ones((B, 1)) if asked is None else np.asarray(asked, np.float64).reshape(B, 1)
    per = np.concatenate([x, host_harness.full_P(P, compact), u, np.zeros((B, 24)) if pfp is None else pfp, on], axis=1)
    o = host_harness.run(exe, tmp, hdr, [per], (B, 242))
    P = o[:, 16:241].reshape(B, 15, 15)
    if compact:
        assert np.isnan(P[:, 9:, :]).all() and np.isnan(P[:, :, 9:]).all()
    else:
        assert not P[:, n:, :].any() and not P[:, :, n:].any()               # a filter without bias states keeps zero bias blocks
    return o[:, :16], P[:, :n, :n].copy(), o[:, 241].astype(np.int32)


GRID = [(d, r, f) for d in ("f64", "f32") for r in lu.RECORDS for f in (False, True)]
GRID_IDS = [f"{d}-{r}-{'pfp' if f else 'shared'}" for d, r, f in GRID]
B_CPU = 40


@pytest.fixture(scope="module")
def references():
    """per (dtype, record, pfp): the case and the oracle's trajectory over the longest horizon, computed once"""
    out = {}
    for dtype, record, use_pfp in GRID:
        n, _ = lu.RECORDS[record]
        po, x, P, u, pfp = lu.make_case(dtype, n, use_pfp, B_CPU, seed=100 + n + int(use_pfp))
        out[dtype, record, use_pfp] = (po, x, P, u, pfp) + lu.oracle_trajectory(po, x, P, u, max(lu.HORIZONS), pfp)
    return out


@pytest.mark.parametrize("dtype,record,use_pfp", GRID, ids=GRID_IDS)
def test_host_compiled_forecast_matches_h_oracle_predicts(harness, references, tmp_path, dtype, record, use_pfp):
    n, compact = lu.RECORDS[record]
    po, x, P, u, pfp, xs, Ps = references[dtype, record, use_pfp]
    wb = np.tile(lu.held(dtype, np.array(lu.HW["wb_static"])), (B_CPU, 1)) if pfp is None else pfp[:, 15:18]
    assert not (u[0, 3:6] - x[0, 13:16] - wb[0]).any()                           # exactly zero rate
    w1 = np.linalg.norm(u[1, 3:6] - x[1, 13:16] - wb[1]) * po.dT_nom
    assert 0 < w1 < po.small_ang_tol and np.linalg.norm(u[2, 3:6]) > 4.0
    for h in lu.HORIZONS:
        for exe in (harness if h in (0, 17) else harness[:1]):                # the plain build, and under ASan + UBSan at h = 0 and 17
            xg, Pg, ticks = run_harness(exe, tmp_path, po, dtype, compact, h, x, P, u, pfp)
            assert (ticks == -1).all()                                        # no limit given: nothing crosses +inf
            if h == 0:                                                        # h = 0 returns the input bits
                assert np.array_equal(xg, x) and np.array_equal(Pg, P)
                continue
            dev = lu.deviations(xg, Pg, xs[h], Ps[h])
            bar = {k: h * v for k, v in lu.STEP_TOL[dtype].items()}
            print(f"{dtype} {record} pfp={use_pfp} h={h}: " + ", ".join(f"{k} {dev[k]:.2e} (bar {bar[k]:.1e}, {dev[k] / bar[k]:.3f})" for k in dev))
            assert np.array_equal(Pg, Pg.transpose(0, 2, 1)) and np.isfinite(xg).all() and np.isfinite(Pg).all()
            assert all(dev[k] <= bar[k] for k in dev), (h, dev, bar)
    assert lu.deviations(xs[17], Ps[17], xs[0], Ps[0])["state"] > 1e-3           # the horizon moved the state


def test_skipped_filters_come_back_all_zero(harness, references, tmp_path):
    po, x, P, u, pfp, xs, Ps = references["f32", "full15", True]
    x = x.copy(); x[5] = 0.0; x[6, 6:10] = 0.0                                  # two filters without state (one with other words set)
    asked = np.ones(B_CPU); asked[7::3] = 0
    skipped = (asked == 0) | ~x[:, 6:10].any(axis=1)
    for exe in harness:
        xg, Pg, ticks = run_harness(exe, tmp_path, po, "f32", False, 17, x, P, u, pfp, asked, sigma_r_max=1e-3, sigma_theta_max=1e-3)
        assert not xg[skipped].any() and not Pg[skipped].any() and (ticks[skipped] == -1).all()
        assert (ticks[~skipped] == 0).all()                                   # every prior variance is above 1e-6
        x1, P1, _ = run_harness(exe, tmp_path, po, "f32", False, 17, x, P, u, pfp)
        assert np.array_equal(xg[~skipped], x1[~skipped]) and np.array_equal(Pg[~skipped], P1[~skipped])


COAST_H = 17
COAST_GRID = [(d, r, f) for d in ("f64", "f32") for r in ("full15", "compact9") for f in (False, True)]


@pytest.mark.parametrize("dtype,record,use_pfp", COAST_GRID, ids=[f"{d}-{r}-{'pfp' if f else 'shared'}" for d, r, f in COAST_GRID])
def test_ticks_to_limit_is_the_rule_on_the_oracle_covariances(harness, tmp_path, dtype, record, use_pfp):
    """The case of the GPU test (same builder, same batch, same seed): by the oracle alone the crossings spread over k = 0, inside the
    horizon and never, and at most 5 % of the filters come within 1e-3 of a limit; the host-compiled body gives every other filter
    the tick the rule gives on the oracle's covariances."""
    n, compact = lu.RECORDS[record]
    B = 200
    po, x, P, u, pfp, sr, st, Ps = lu.coast_case(dtype, n, use_pfp, B, COAST_H, seed=300 + n)
    ref = lu.ticks_rule(Ps, sr, st)
    clear = lu.limit_margin(Ps, sr, st) >= lu.MARGIN
    print(f"{dtype} {record} pfp={use_pfp}: sigma_r_max {sr:.4g} sigma_theta_max {st:.4g}; crossings {np.bincount(ref + 1, minlength=COAST_H + 2)}; "
          f"excluded {(~clear).sum()} of {B}")
    assert (~clear).mean() <= lu.MAX_EXCLUDED
    assert (ref == 0).sum() >= B // 10 and (ref == -1).sum() >= B // 10 and ((ref > 0) & (ref < COAST_H)).sum() >= B // 4
    assert len(set(ref[ref > 0])) >= 6                                        # spread over the horizon, not one tick
    only_r, only_t = lu.ticks_rule(Ps, sr, np.inf), lu.ticks_rule(Ps, np.inf, st)
    assert (only_r != ref).any() and (only_t != ref).any()                    # both limits decide somewhere
    for exe in harness:
        _, _, ticks = run_harness(exe, tmp_path, po, dtype, compact, COAST_H, x, P, u, pfp, sigma_r_max=sr, sigma_theta_max=st)
        assert np.array_equal(ticks[clear], ref[clear]), np.argwhere(ticks != ref).ravel()
    _, _, t_r = run_harness(harness[0], tmp_path, po, dtype, compact, COAST_H, x, P, u, pfp, sigma_r_max=sr)
    _, _, t_t = run_harness(harness[0], tmp_path, po, dtype, compact, COAST_H, x, P, u, pfp, sigma_theta_max=st)
    assert np.array_equal(t_r[clear], only_r[clear]) and np.array_equal(t_t[clear], only_t[clear])   # +inf disables a limit
    for h in (0, 5):                                                          # a shorter horizon sees the crossings up to it
        _, _, t_h = run_harness(harness[0], tmp_path, po, dtype, compact, h, x, P, u, pfp, sigma_r_max=sr, sigma_theta_max=st)
        assert np.array_equal(t_h[clear], np.where(ref <= h, ref, -1)[clear])
