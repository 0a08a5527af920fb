"""CPU tests of noise adaptation (include/qle_adapt.h, libqle_adapt.so, quadrotor_landing_amd/adapt.py, csrc/ekf_adapt.hpp): the library
builds, exports and binds what its header declares, its kernels are its own, it needs the tick library and no other library of the
project, its generated code passes the stale-EXEC audit and uses no scratch, every refusal is made before any GPU call (without a GPU a
HIP call would fail with another error class), noise_columns reproduces the R_k of quad::update_noise, and the arithmetic of the two
kernels -- compiled for the host, once plain and once as a stand-alone program under AddressSanitizer and UBSan -- accumulates 6
consecutive tag ticks with an apply after every third as the reference of adapt_util does: the dense oracle's predict followed by the
numpy restatement of the innovation per tick, numpy.linalg.solve, plain fp64 sums, the apply formula in numpy.

What the host build covers: noise_columns, adapt_sample, adapt_accumulate, adapt_apply_one and pregate_eval_pivots.  What it does not: the
kernels' own loads and stores (the accumulator planes and the R words of the parameter records among them); tests/test_gpu_adapt.py
holds those.

Measured deviations of the host-compiled arithmetic from the reference and the stated tolerances: tests/tolerances_adapt.md.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import host_harness
import oracle
from adapt_util import APPLY_TOL, COUNTS, TOL, apply_error, apply_ref, deviations, reference_run
from elf_util import _kernels
from gate_util import HW, TOL as GATE_TOL, predict_then_innovation
from innovation_util import CHI2_6_099
from oracle import ekf_np
from quadrotor_landing_amd import _lib, adapt
from score_util import make_sequence
from side_lib_util import (_params, _views, assert_audit_counts, assert_exports_and_binds, ensure_built, kernel_descriptors, run_audit,
                           scratch_free)
from util import forbid_native, rand_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qle_adapt.h")


@pytest.fixture(scope="module")
def adapt_so():
    return ensure_built("adapt")


def test_library_exports_and_binds_every_declared_function(adapt_so):
    _, txt = assert_exports_and_binds(adapt, HEADER, "qad", adapt_so,
                                      ["qad_apply", "qad_last_error", "qad_launch_census_begin", "qad_launch_census_end", "qad_launch_count", "qad_observe_tick", "qad_run", "qad_run_host"])
    assert adapt.WORDS == int(re.search(r"#define QAD_WORDS (\d+)", txt).group(1)) == 24
    assert C.sizeof(adapt.QadConfig) == 4 + 4 + 8 + 4 + 4 + 8 + 48 + 48


def test_kernels_are_its_own_and_only_the_adaptation_ones(adapt_so):
    mine, main = _kernels(adapt_so), _kernels(_lib.LIB_PATH)
    assert mine and main and not mine & main, sorted(mine & main)
    ids = {_lib.demangle(m) for m in mine}
    observe = {i for i in ids if i.startswith("void qle::k_adapt_observe<")}
    apply = {i for i in ids if i.startswith("void qle::k_adapt_apply<")}
    assert len(observe) == 8 and len(apply) == 2 and ids == observe | apply, sorted(ids)   # T x DIRECT x COMPACT; T
    assert not any("k_adapt" in _lib.demangle(m) for m in main)


def test_library_needs_the_tick_library_and_no_other(adapt_so):
    d = open(adapt_so, "rb").read()
    assert set(re.findall(rb"libqle_[a-z]+\.so", d)) == {b"libqle_ekf.so"}


def test_generated_device_code_passes_the_audit_and_uses_no_scratch(adapt_so):
    r, asm = run_audit("adapt")
    assert_audit_counts(r, "adapt", 10)
    desc, meta = kernel_descriptors(asm)
    assert len(desc) == 10 and all(d.scratch == 0 for d in desc.values()), {k: d.scratch for k, d in desc.items()}
    assert scratch_free(meta)


# ---------------------------------------------------------------- refusals, before any GPU call
def _cfg(**kw):
    c = adapt.QadConfig()
    c.struct_size = C.sizeof(c)
    c.window, c.gain, c.n_min, c.chi2_max = 4, 1.0, 2, float("inf")
    c.R_lo, c.R_hi = (C.c_double * 6)(*[1e-4] * 6), (C.c_double * 6)(*[1.0] * 6)
    for k, v in kw.items():
        setattr(c, k, (C.c_double * 6)(*v) if k in ("R_lo", "R_hi") else v)
    return c


def test_library_refuses_before_any_gpu_call(adapt_so):
    """No GPU here: a call that got as far as the HIP runtime would return QLE_ERR_HIP (or crash on the fake pointers), not these."""
    Q = adapt.adapt_lib()
    v, iv = _views()
    v.filter_params = 0x7F6000000000
    p = _params()
    acc = 0x7F3000000000
    B = C.byref
    INV, STATE = _lib.QLE_ERR_INVALID, _lib.QLE_ERR_STATE
    inf = float("inf")
    err = Q.qad_last_error
    obs = Q.qad_observe_tick
    assert obs(None, B(iv), B(p), acc, inf) == INV and b"view" in err()
    assert obs(B(v), None, B(p), acc, inf) == INV
    assert obs(B(v), B(iv), None, acc, inf) == INV
    assert obs(B(v), B(iv), B(p), None, inf) == INV and b"acc" in err()
    assert obs(B(v), B(iv), B(p), acc + 8, inf) == INV and b"16-byte" in err()
    for bad in (float("nan"), 0.0, -1.0):
        assert obs(B(v), B(iv), B(p), acc, bad) == INV and b"chi2_max" in err()
    short, _ = _views(); short.struct_size = C.sizeof(short) - 8; short.filter_params = v.filter_params
    assert obs(B(short), B(iv), B(p), acc, inf) == INV and b"struct_size" in err()
    _, ishort = _views(); ishort.struct_size = 8
    assert obs(B(v), B(ishort), B(p), acc, inf) == INV and b"struct_size" in err()
    mr = _params(multirate_ekf=1)
    assert obs(B(v), B(iv), B(mr), acc, inf) == STATE and b"multirate" in err()
    _, notag = _views(tag=False)
    assert obs(B(v), B(notag), B(p), acc, inf) == INV and b"tag slot" in err()
    assert obs(B(v), B(iv), B(_params(est_bias=0)), acc, inf) == INV   # the view says 15 states
    shared, _ = _views()   # filter_params NULL
    assert obs(B(shared), B(iv), B(p), acc, inf) == STATE and b"per-filter parameters are not in force" in err()
    # qad_apply
    ap = Q.qad_apply
    out, flags = 0x7F5000000000, 0x7F5100000000
    ok = _cfg()
    assert ap(None, acc, B(ok), flags, out) == INV
    assert ap(B(short), acc, B(ok), flags, out) == INV and b"struct_size" in err()
    assert ap(B(v), None, B(ok), flags, out) == INV and b"acc" in err()
    assert ap(B(v), acc + 8, B(ok), flags, out) == INV and b"16-byte" in err()
    assert ap(B(v), acc, None, flags, out) == INV and b"cfg" in err()
    assert ap(B(v), acc, B(ok), flags, out + 4) == INV and b"8-byte" in err()
    assert ap(B(shared), acc, B(ok), flags, out) == STATE and b"per-filter parameters are not in force" in err()
    bad_cfgs = [(_cfg(struct_size=C.sizeof(ok) - 8), b"struct_size"), (_cfg(window=0), b"window"), (_cfg(gain=0.0), b"gain"), (_cfg(gain=1.5), b"gain"),
                (_cfg(gain=float("nan")), b"gain"), (_cfg(n_min=0), b"n_min"), (_cfg(chi2_max=float("nan")), b"chi2_max"), (_cfg(chi2_max=0.0), b"chi2_max"),
                (_cfg(R_lo=[1e-4] * 5 + [0.0]), b"R_lo"), (_cfg(R_lo=[inf] + [1e-4] * 5), b"R_lo"), (_cfg(R_lo=[float("nan")] + [1e-4] * 5), b"R_lo"),
                (_cfg(R_hi=[1.0] * 3 + [1e-5] + [1.0] * 2), b"R_hi"), (_cfg(R_hi=[float("nan")] + [1.0] * 5), b"R_hi")]
    for c, word in bad_cfgs:
        assert ap(B(v), acc, B(c), flags, out) == INV and word in err(), word
    # qad_run / qad_run_host: what can be refused without a handle is refused before the handle is looked at
    h = 0x7F4000000000
    hacc = C.cast(acc, C.POINTER(C.c_double))
    run, run_host = Q.qad_run, Q.qad_run_host
    assert run(h, h, 0, 1, None, acc, B(ok)) == INV
    assert run(h, h, 0, 1, B(mr), acc, B(ok)) == STATE and b"multirate" in err()
    assert run(h, h, 0, 1, B(p), None, B(ok)) == INV and b"acc" in err()
    assert run(h, h, 0, 1, B(p), acc + 8, B(ok)) == INV and b"16-byte" in err()
    assert run(h, h, 0, 1, B(p), acc, None) == INV and b"cfg" in err()
    assert run(None, h, 0, 1, B(p), acc, B(ok)) == INV and b"handle" in err()
    assert run_host(h, h, 0, 1, None, B(ok), hacc, hacc) == INV
    assert run_host(h, h, 0, 1, B(mr), B(ok), hacc, hacc) == STATE and b"multirate" in err()
    assert run_host(h, h, 0, 1, B(p), B(ok), None, hacc) == INV and b"acc_host" in err()
    assert run_host(h, h, 0, 1, B(p), B(ok), hacc, None) == INV and b"R_host" in err()
    assert run_host(h, h, 0, 1, B(p), None, hacc, hacc) == INV and b"cfg" in err()
    assert run_host(None, h, 0, 1, B(p), B(ok), hacc, hacc) == INV and b"handle" in err()
    for c, word in bad_cfgs:
        assert run(h, h, 0, 1, B(p), acc, B(c)) == INV and word in err(), word
        assert run_host(h, h, 0, 1, B(p), B(c), hacc, hacc) == INV and word in err(), word
    assert Q.qad_launch_count() == 0


class FakeEkf:
    batch, dtype, device, num_states, _h = 100, _lib.QLE_F32, 0, 15, None

    def __init__(self, **kw):
        self.params = _params(**kw)   # from the tick library: made first


def test_python_refuses_multirate_and_bad_configurations_before_any_native_call(monkeypatch):
    class FakeIO:
        ekf = FakeEkf(multirate_ekf=1)

    plain = FakeEkf()
    plain.derived = _lib.QleDerived()
    _lib.check(_lib.lib().qle_params_derive(C.byref(plain.params), C.byref(plain.derived)))
    forbid_native(monkeypatch)
    with pytest.raises(_lib.QleError) as e:
        adapt.Adapter(FakeIO())
    assert e.value.code == _lib.QLE_ERR_STATE
    with pytest.raises(_lib.QleError) as e:
        adapt.run_host(FakeIO.ekf, None, 0, 1)
    assert e.value.code == _lib.QLE_ERR_STATE
    for kw in (dict(window=0), dict(gain=0.0), dict(gain=1.01), dict(n_min=0), dict(chi2_max=0.0), dict(chi2_max=float("nan")), dict(R_lo=[0.0] * 6),
               dict(R_lo=[1.0] * 6, R_hi=[0.5] * 6), dict(R_lo=[1.0] * 5)):
        with pytest.raises(ValueError):
            adapt.make_config(plain, **kw)
    c = adapt.make_config(plain)
    R = list(plain.derived.R)
    assert (c.window, c.gain, c.n_min, c.chi2_max) == (20, 1.0, 10, float("inf"))
    assert list(c.R_lo) == [r / 100.0 for r in R] and list(c.R_hi) == [r * 100.0 for r in R]
    assert adapt.make_config(plain, window=1).n_min == 1


def test_adaptation_reads_the_accumulator_words():
    acc = np.zeros((adapt.WORDS, 2))
    acc[0, 0], acc[1, 0], acc[20, 0], acc[21, 0], acc[22, 0] = 4, 1, 12, 2, 3
    acc[2:8, 0] = 0.08; acc[8:14, 0] = 6.0; acc[14:20, 0] = 3.0
    with np.errstate(divide="ignore", invalid="ignore"):
        a = adapt.Adaptation(acc)
    assert a.n[0] == 4 and a.n_bad[0] == 1 and a.n_total[0] == 12 and a.windows[0] == 2 and a.n_rejected[0] == 3
    assert a.r_hat.shape == (2, 6) and (a.r_hat[0] == 0.02).all() and (a.ratio[0] == 2.0).all()
    assert np.isnan(a.r_hat[1]).all() and np.isnan(a.ratio[1]).all()


# ---------------------------------------------------------------- the arithmetic on the host
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/cpp/adapt_harness.cpp: the arithmetic of ekf_adapt.hpp behind pregate_eval_pivots compiled by g++ (the HIP headers define the
    device decorators away), once as it is and once as a stand-alone program under AddressSanitizer and UBSan."""
    return host_harness.build("adapt_harness", tmp_path_factory)


TICKS, NF, WINDOW, N_MIN = 6, 64, 3, 2
CFG_WORDS = 20


def _header(po, dtype, ticks, window=WINDOW, gain=1.0, n_min=N_MIN, chi2_max=np.inf, lo=None, hi=None):
    R = np.array(list(po.R))
    lo, hi = (R / 100 if lo is None else lo), (R * 100 if hi is None else hi)
    return [NF, po.direct_orien_method, ticks, int(dtype == "f64"), window, gain, n_min, chi2_max, *lo, *hi, *host_harness.params_header(po)]


@pytest.mark.parametrize("direct", [1, 0])
def test_noise_columns_reproduce_the_noise_of_the_tick(harness, tmp_path, direct):
    """N diag(R) N^T of noise_columns against the R_k quad::update_noise multiplies out, fp64, random states and noises: relative to the
    largest element of R_k at the gate's own tolerance for S."""
    po = oracle.make_params(update_freq=400.0, direct_orien_method=direct, est_bias=1, **HW)
    p = ekf_np.Params.from_orc(po)
    rng = np.random.default_rng(21 + direct)
    x, _ = rand_states(rng, NF, 15)
    R = np.array(list(po.R)) * rng.uniform(0.3, 3.0, size=(NF, 6))
    from adapt_util import noise_jacobian
    for exe in harness:
        out = host_harness.run(exe, tmp_path, _header(po, "f64", 0), [np.concatenate([x, R], axis=1)], (NF, 72))
        Rk, N = out[:, :36].reshape(NF, 6, 6), out[:, 36:].reshape(NF, 6, 6)
        mine = np.einsum("bik,bk,bjk->bij", N, R, N)
        scale = np.abs(Rk).max(axis=(1, 2), keepdims=True)
        worst = float((np.abs(mine - Rk) / scale).max())
        print(f"direct={direct}: N diag(R) N^T against update_noise {worst:.2e}")
        assert worst < GATE_TOL["f64"]["S"]
        assert (np.abs(N - np.stack([noise_jacobian(p, x[i]) for i in range(NF)])).max() < 1e-14)
        assert (direct == 1) == bool(N[:, 0:3, 3:6].any()) and not N[:, 3:6, 0:3].any()


GRID = [(d, o) for d in ("f64", "f32") for o in (1, 0)]
GRID_IDS = [f"{d}-direct{o}" for d, o in GRID]


@pytest.mark.parametrize("dtype,direct", GRID, ids=GRID_IDS)
def test_host_compiled_arithmetic_adapts_over_six_ticks_as_the_reference(harness, tmp_path, dtype, direct):
    po = oracle.make_params(update_freq=400.0, direct_orien_method=direct, est_bias=1, **HW)
    p = ekf_np.Params.from_orc(po)
    rng = np.random.default_rng(31 + 7 * direct)
    r32 = (lambda a: a.astype(np.float32).astype(np.float64)) if dtype == "f32" else (lambda a: a)
    x, P = rand_states(rng, NF, po.num_states, cov_scale=0.05)
    pfp = np.zeros((NF, 24))
    pfp[:, 0:12] = np.array(list(po.Q)) * 10 ** rng.uniform(-0.5, 0.5, size=(NF, 12))
    pfp[:, 12:15] = HW["ab_static"]; pfp[:, 15:18] = HW["wb_static"]
    pfp[:, 18:24] = np.array(list(po.R)) * rng.uniform(0.3, 3.0, size=(NF, 6))
    pfp = r32(pfp)
    U, Z = make_sequence(rng, po, x, P, TICKS, range(TICKS), pfp, ang=0.05, pos=0.03)
    ON = np.ones((TICKS, NF), bool)
    ON[1, 5] = ON[2, 5] = False          # filter 5: one scored tick in the first window; it reaches n_min one window late
    ON[:, 9] = False                     # filter 9: never on
    Z[2, 7, 0] = np.nan                  # filter 7: one tag pose that cannot be scored
    Z[5, 11, 0:3] += np.array([0.6, -0.6, 0.53])   # filter 11: one tag pose displaced by 1 m (the last: the tick behind it takes it in)
    U, Z = r32(U), r32(Z)
    R0 = np.array(list(po.R))
    lo, hi = R0 / 100, R0 * 100
    trace = []
    ref, applies = reference_run(po, p, r32(x), r32(P), U, Z, ON.astype(np.uint8), range(TICKS), pfp, WINDOW, 1.0, N_MIN, lo, hi, dtype,
                                 chi2_max=CHI2_6_099, trace=trace)
    nis = np.stack([t[3] for t in trace])
    assert (np.abs(nis[np.isfinite(nis)] / CHI2_6_099 - 1) > 1e-3).all()   # every decision is clear of the threshold
    assert ref.min_sample > 0   # no sample of the reference is <= 0
    hdr = _header(po, dtype, TICKS, chi2_max=CHI2_6_099)
    per = [np.concatenate([xt, host_harness.full_P(Pt), U[t], Z[t], pfp, ON[t][:, None].astype(np.float64)], axis=1) for t, (xt, Pt, _, _) in enumerate(trace)]
    napply = TICKS // WINDOW
    for exe in harness:
        out = host_harness.run(exe, tmp_path, hdr, per, (NF, 30 + 37 * napply))
        acc, R_end = out[:, :24], out[:, 24:30]
        # counts are exact, at the end and in front of every apply
        np.testing.assert_array_equal(acc[:, COUNTS], ref.acc[:, COUNTS])
        assert not acc[:, 23].any()
        assert not acc[9].any() and (R_end[9] == pfp[9, 18:24]).all()                      # never on: 24 words and R untouched
        assert acc[7, 1] == 1 and acc[7, 20] == 5 and acc[11, 22] == 1 and acc[11, 20] == 5
        rest = np.setdiff1d(np.arange(NF), [5, 7, 9, 11])
        assert (acc[rest, 20] == 6).all() and (acc[rest, 21] == 2).all() and not acc[rest, 0].any() and not acc[rest][:, [1, 22]].any()
        assert acc[5, 20] == 4 and acc[5, 21] == 1 and acc[5, 0] == 0
        worst = {g: 0.0 for g in TOL["cpu"][dtype]}
        for j in range(napply):
            blk = out[:, 30 + 37 * j:30 + 37 * (j + 1)]
            before, Rb, Ra, applied = blk[:, :24], blk[:, 24:30], blk[:, 30:36], blk[:, 36] != 0
            ref_before, _, ref_applied, _ = applies[j]
            np.testing.assert_array_equal(before[:, COUNTS], ref_before.acc[:, COUNTS])
            np.testing.assert_array_equal(applied, ref_applied)
            np.testing.assert_array_equal(applied, before[:, 0] >= N_MIN)
            d = deviations(before, ref_before)
            worst = {g: max(worst[g], d[g]) for g in d}
            # the apply on its own: numpy on the harness's accumulators
            _, R_np, _, clamped = apply_ref(before, Rb, 1.0, N_MIN, lo, hi, dtype)
            rel, eq = apply_error(Ra, R_np, clamped)
            assert rel <= APPLY_TOL[dtype] and eq, (rel, eq)
            assert (Ra[~applied] == Rb[~applied]).all()
        # filter 5 carried its first window's sums into the second apply: n = 1 + 3
        assert out[5, 30 + 36] == 0 and out[5, 30] == 1 and out[5, 30 + 37 + 36] == 1 and out[5, 30 + 37] == 4
        assert (out[5, 30 + 37 + 2:30 + 37 + 8] > out[5, 30 + 2:30 + 8]).all()
        print(f"{dtype} direct={direct}: " + " ".join(f"{g} {v:.2e}" for g, v in worst.items()))
        tol = TOL["cpu"][dtype]
        assert all(worst[g] < tol[g] for g in worst), (worst, tol)


def test_a_tick_whose_S_is_not_positive_definite_counts_in_n_bad_and_changes_no_other_word(harness, tmp_path):
    """One tag tick, fp64: every fourth filter holds a negated covariance, so its S is finite with a negative eigenvalue.  Such a
    tick counts in n_bad and moves neither another word of the record nor R, whichever of the source's two factorisations of S
    (pregate_eval_pivots, adapt_sample) says so: both see the same S.  The other filters score the tick."""
    po = oracle.make_params(update_freq=400.0, direct_orien_method=1, est_bias=1, **HW)
    p = ekf_np.Params.from_orc(po)
    rng = np.random.default_rng(41)
    x, P = rand_states(rng, NF, po.num_states, cov_scale=0.05)
    pfp = np.tile(np.array([*po.Q, *HW["ab_static"], *HW["wb_static"], *po.R]), (NF, 1))
    U, Z = make_sequence(rng, po, x, P, 1, range(1), pfp, ang=0.05, pos=0.03)
    bad = np.arange(NF) % 4 == 1
    P[bad] = -P[bad]
    _, S, _, _, _ = predict_then_innovation(po, p, x, P, U[0], Z[0], pfp)
    low = np.linalg.eigvalsh(S).min(axis=1)
    assert np.isfinite(S).all() and (low[bad] < 0).all() and (low[~bad] > 0).all()
    per = [np.concatenate([x, host_harness.full_P(P), U[0], Z[0], pfp, np.ones((NF, 1))], axis=1)]
    for exe in harness:
        out = host_harness.run(exe, tmp_path, _header(po, "f64", 1, window=2), per, (NF, 30))   # one tick of a window of two: no apply
        acc, R_end = out[:, :24], out[:, 24:30]
        assert (acc[bad, 1] == 1).all() and not np.delete(acc[bad], 1, axis=1).any()
        assert (acc[~bad, 0] == 1).all() and (acc[~bad, 20] == 1).all() and not acc[~bad][:, [1, 22]].any()
        np.testing.assert_array_equal(R_end, pfp[:, 18:24])
