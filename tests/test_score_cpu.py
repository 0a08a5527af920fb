"""CPU tests of innovation scoring (include/qle_score.h, libqle_score.so, quadrotor_landing_amd/score.py, csrc/ekf_score.hpp): the library
builds, exports and binds what its header declares, its kernels are its own, it needs the tick library and no other library of the
project, its generated code passes the stale-EXEC audit, every refusal is made before any GPU call (without a GPU a HIP call would fail
with another error class), and the arithmetic of k_score -- compiled for the host, once plain and once as a stand-alone program under
AddressSanitizer and UBSan -- accumulates 5 consecutive tag ticks as the reference of score_util does: the dense oracle's predict
followed by the numpy restatement of the innovation per tick, numpy's slogdet, plain fp64 sums.

What the host build covers: score_accumulate and pregate_eval_pivots.  What it does not: the kernel's own loads and stores (the
accumulator planes among them) and the batch summary; tests/test_gpu_score.py holds those.

Measured deviations of the host-compiled arithmetic from the reference (worst over both orientation methods, shared and per-filter
parameters, 64 filters, 5 ticks; each word relative to its sum of absolute terms) and the stated tolerances: tests/tolerances_score.md.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import host_harness
import oracle
from elf_util import _kernels
from gate_util import HW, predict_then_innovation
from oracle import ekf_np
from quadrotor_landing_amd import _lib, score
from score_util import COUNTS, PREV, TOL, ScoreRef, deviations, make_sequence
from side_lib_util import _params, _views, assert_audit_counts, assert_exports_and_binds, ensure_built, run_audit
from util import forbid_native, rand_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qle_score.h")


@pytest.fixture(scope="module")
def score_so():
    return ensure_built("score")


def test_library_exports_and_binds_every_declared_function(score_so):
    _, txt = assert_exports_and_binds(score, HEADER, "qsc", score_so,
                                      ["qsc_last_error", "qsc_launch_census_begin", "qsc_launch_census_end", "qsc_launch_count", "qsc_run", "qsc_run_host", "qsc_score_tick", "qsc_summary"])
    assert score.WORDS == int(re.search(r"#define QSC_WORDS (\d+)", txt).group(1)) == 40
    assert score.SUMS == int(re.search(r"#define QSC_SUMS (\d+)", txt).group(1)) == 30


def test_kernels_are_its_own_and_only_the_scoring_ones(score_so):
    mine, main = _kernels(score_so), _kernels(_lib.LIB_PATH)
    assert mine and main and not mine & main, sorted(mine & main)
    ids = {_lib.demangle(m) for m in mine}
    tick = {i for i in ids if i.startswith("void qle::k_score<")}
    assert len(tick) == 16   # T x DIRECT x PFP x COMPACT
    rest = {i.split("(")[0] for i in ids - tick}
    assert rest == {"qle::k_score_tiles", "qle::k_score_reduce"}, sorted(rest)
    assert not any("k_score" in _lib.demangle(m) for m in main)


def test_library_needs_the_tick_library_and_no_other(score_so):
    d = open(score_so, "rb").read()
    assert set(re.findall(rb"libqle_[a-z]+\.so", d)) == {b"libqle_ekf.so"}


def test_generated_device_code_passes_the_stale_exec_audit(score_so):
    assert_audit_counts(run_audit("score")[0], "score", 18)


# ---------------------------------------------------------------- refusals, before any GPU call
def test_library_refuses_before_any_gpu_call(score_so):
    """No GPU here: a call that got as far as the HIP runtime would return QLE_ERR_HIP (or crash on the fake pointers), not these."""
    Q = score.score_lib()
    v, iv = _views()
    p = _params()
    acc = 0x7F3000000000
    B = C.byref
    INV, STATE = _lib.QLE_ERR_INVALID, _lib.QLE_ERR_STATE
    tick = Q.qsc_score_tick
    assert tick(None, B(iv), B(p), acc) == INV and b"view" in Q.qsc_last_error()
    assert tick(B(v), None, B(p), acc) == INV
    assert tick(B(v), B(iv), None, acc) == INV
    assert tick(B(v), B(iv), B(p), None) == INV and b"acc" in Q.qsc_last_error()
    assert tick(B(v), B(iv), B(p), acc + 8) == INV and b"16-byte" in Q.qsc_last_error()
    short, _ = _views(); short.struct_size = C.sizeof(short) - 8
    assert tick(B(short), B(iv), B(p), acc) == INV and b"struct_size" in Q.qsc_last_error()
    _, ishort = _views(); ishort.struct_size = 8
    assert tick(B(v), B(ishort), B(p), acc) == INV and b"struct_size" in Q.qsc_last_error()
    mr = _params(multirate_ekf=1)
    assert tick(B(v), B(iv), B(mr), acc) == STATE and b"multirate" in Q.qsc_last_error()
    _, notag = _views(tag=False)
    assert tick(B(v), B(notag), B(p), acc) == INV and b"tag slot" in Q.qsc_last_error()
    assert tick(B(v), B(iv), B(_params(est_bias=0)), acc) == INV   # the view says 15 states
    # qsc_run / qsc_run_host: what can be refused without a handle is refused before the handle is looked at
    h = 0x7F4000000000
    for run, a in ((Q.qsc_run, acc), (Q.qsc_run_host, C.cast(acc, C.POINTER(C.c_double)))):
        assert run(h, h, 0, 1, None, a) == INV
        assert run(h, h, 0, 1, B(mr), a) == STATE and b"multirate" in Q.qsc_last_error()
        assert run(h, h, 0, 1, B(p), None) == INV and b"acc" in Q.qsc_last_error()
        assert run(None, h, 0, 1, B(p), a) == INV and b"handle" in Q.qsc_last_error()
    assert Q.qsc_run(h, h, 0, 1, B(p), acc + 8) == INV and b"16-byte" in Q.qsc_last_error()
    # qsc_summary
    out = 0x7F5000000000
    assert Q.qsc_summary(None, acc, None, out) == INV
    assert Q.qsc_summary(B(short), acc, None, out) == INV and b"struct_size" in Q.qsc_last_error()
    assert Q.qsc_summary(B(v), None, None, out) == INV
    assert Q.qsc_summary(B(v), acc + 8, None, out) == INV and b"16-byte" in Q.qsc_last_error()
    assert Q.qsc_summary(B(v), acc, None, None) == INV
    assert Q.qsc_launch_count() == 0


def test_python_refuses_multirate_before_any_native_call(monkeypatch):
    class FakeEkf:
        batch, dtype, device, num_states, _h = 100, _lib.QLE_F32, 0, 15, None
        params = _params(multirate_ekf=1)   # from the tick library: made first

    class FakeIO:
        ekf = FakeEkf()

    forbid_native(monkeypatch)
    with pytest.raises(_lib.QleError) as e:
        score.Scorer(FakeIO())
    assert e.value.code == _lib.QLE_ERR_STATE
    with pytest.raises(_lib.QleError) as e:
        score.run_host(FakeEkf(), None, 0, 1)
    assert e.value.code == _lib.QLE_ERR_STATE


def test_score_reads_the_accumulator_words():
    """Score over a hand-made record: the statistics are the ratios include/qle_score.h names."""
    acc = np.zeros((score.WORDS, 2))
    acc[0, 0], acc[1, 0], acc[3, 0] = 4, 26.0, -40.0
    acc[6:12, 0] = 2.0; acc[12:18, 0] = 8.0; acc[18:24, 0] = 4.0; acc[24:30, 0] = -2.0
    with np.errstate(divide="ignore", invalid="ignore"):
        s = score.Score(acc)
    assert s.n[0] == 4 and s.nis_mean[0] == 6.5
    assert s.loglik[0] == -0.5 * (26.0 - 40.0 + 24.0 * np.log(2 * np.pi))
    assert s.var_ratio.shape == (2, 6) and (s.var_ratio[0] == 2.0).all() and (s.rho1[0] == -0.25).all() and (s.nu_mean[0] == 0.5).all()
    assert s.loglik[1] == 0.0 and np.isnan(s.var_ratio[1]).all()


# ---------------------------------------------------------------- the arithmetic on the host
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/cpp/score_harness.cpp: score_accumulate and pregate_eval_pivots compiled by g++ (the HIP headers define the device decorators
    away), once as it is and once as a stand-alone program under AddressSanitizer and UBSan."""
    return host_harness.build("score_harness", tmp_path_factory)


TICKS, NF = 5, 64


def run_harness(exe, tmp, po, dtype, states, U, Z, ON, pfp):
    """states: [(x, P)] in front of every tick; -> acc [B, 40]"""
    B = NF
    hdr = [B, po.direct_orien_method, TICKS, int(pfp is not None), int(dtype == "f64"), *host_harness.params_header(po)]
    per = [np.concatenate([x, host_harness.full_P(P), U[t], Z[t], np.zeros((B, 24)) if pfp is None else pfp, ON[t][:, None].astype(np.float64)], axis=1)
           for t, (x, P) in enumerate(states)]
    return host_harness.run(exe, tmp, hdr, per, (B, 40))


GRID = [(d, o, f) for d in ("f64", "f32") for o in (1, 0) for f in (False, True)]
GRID_IDS = [f"{d}-direct{o}-{'pfp' if f else 'shared'}" for d, o, f in GRID]


@pytest.mark.parametrize("dtype,direct,use_pfp", GRID, ids=GRID_IDS)
def test_host_compiled_arithmetic_accumulates_five_ticks_as_the_reference(harness, tmp_path, dtype, direct, use_pfp):
    po = oracle.make_params(update_freq=400.0, direct_orien_method=direct, est_bias=1, **HW)
    p = ekf_np.Params.from_orc(po)
    rng = np.random.default_rng(11 + 7 * direct + int(use_pfp))
    r32 = (lambda a: a.astype(np.float32).astype(np.float64)) if dtype == "f32" else (lambda a: a)
    x, P = rand_states(rng, NF, po.num_states, cov_scale=0.05)
    pfp = None
    if use_pfp:
        pfp = np.zeros((NF, 24))
        pfp[:, 0:12] = np.array(list(po.Q)) * 10 ** rng.uniform(-0.5, 0.5, size=(NF, 12))
        pfp[:, 12:15] = HW["ab_static"]; pfp[:, 15:18] = HW["wb_static"]
        pfp[:, 18:24] = np.array(list(po.R)) * rng.uniform(0.3, 3.0, size=(NF, 6))
        pfp = r32(pfp)
    U, Z = make_sequence(rng, po, x, P, TICKS, range(TICKS), pfp, ang=0.1, pos=0.05)
    U, Z = r32(U), r32(Z)
    ON = np.ones((TICKS, NF), bool)
    ON[1, 5] = ON[3, 5] = False          # filter 5: two gaps, the lag pairs bridge them
    ON[:, 9] = False                     # filter 9: never on
    Z[2, 7, 0] = np.nan                  # filter 7: one tag pose that cannot be scored
    # every tick's state in front of it: the oracle's, free-running with every correction (rounded to what an fp32 handle holds)
    ref = ScoreRef(NF)
    states = []
    for t in range(TICKS):
        x, P = r32(x), r32(P)
        states.append((x, P))
        nu, S, nis, _, _ = predict_then_innovation(po, p, x, P, U[t], Z[t], pfp, mask=ON[t])
        ref.add(nu, S, nis, ON[t])
        m = (ON[t] & np.isfinite(Z[t]).all(axis=1)).astype(np.uint8)
        x, P = oracle.run_batch(po, x, P, U[t:t + 1], np.nan_to_num(Z[t])[None], m[None], per_filter_params=pfp)
    for exe in harness:
        acc = run_harness(exe, tmp_path, po, dtype, states, U, Z, ON, pfp)
        np.testing.assert_array_equal(acc[:, COUNTS], ref.acc[:, COUNTS])
        assert acc[5, 0] == 3 and acc[5, 5] == 2 and not acc[9].any() and acc[7, 4] == 1 and acc[7, 0] == 4 and acc[7, 5] == 3
        assert not acc[:, 36:].any()
        dev = deviations(acc, ref)
        print(f"{dtype} direct={direct} pfp={use_pfp}: " + " ".join(f"{g} {v:.2e}" for g, v in dev.items()))
        tol = TOL["cpu"][dtype]
        assert all(dev[g] < tol[g] for g in dev), (dev, tol)
        # nu^-: the last scored innovation, to the nu tolerance of its own size
        assert np.abs(acc[:, PREV] - ref.acc[:, PREV]).max() <= tol["nu"] * max(np.abs(ref.acc[:, PREV]).max(), 1e-300)
