"""CPU tests of the IMM mixing step and mode-probability recursion (include/qle_imm.h, libqle_imm.so, quadrotor_landing_amd/imm.py,
csrc/ekf_imm.hpp): the library builds, exports and binds what its header declares, its five kernels are its own, it needs no other library
of the project, its generated code passes the stale-EXEC audit and uses no scratch memory and no LDS, every refusal is made before any GPU
call, the Python binding checks Pi on the host and refuses a multirate handle without a native call, and the arithmetic of k_imm_mix and
k_imm_update -- compiled for the host with g++, once plain and once as a stand-alone program under AddressSanitizer and UBSan, the
shuffle loops restated as the same ascending loops over an array -- agrees with the numpy restatements `imm_util.mix_ref` /
`imm_util.update_ref`.

Before it is used, `mix_ref` is pinned by forms that do not share its code: conservation of the first two moments (with rows of Pi
adding to 1, sum_j c_j x0_j = sum_i mu_i x_i and the law of total variance), a rank-one Pi against `bank_util.fuse_ref`, and an identity
Pi.

What the host build covers: the functions of ekf_imm.hpp and those it takes from ekf_bank.hpp.  What it does not: the kernel's loads and
stores, its shuffles, in-place writing and which records keep their bits; tests/test_gpu_imm.py holds those.

Measured deviations of the host-compiled arithmetic from the truth (printed per case, `pytest -s`) and the stated tolerances:
tests/tolerances_imm.md.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import bank_util as bu
import host_harness
import imm_util as iu
import side_lib_util
from elf_util import _kernels, _needed
from quadrotor_landing_amd import _lib, devio, imm
from side_lib_util import FakeTensor, assert_audit_counts, assert_exports_and_binds, ensure_built, kernel_descriptors, run_audit, scratch_free
from util import forbid_native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qle_imm.h")
N_KERNELS = 5   # k_imm_mix: T x COMPACT, and k_imm_update


@pytest.fixture(scope="module")
def imm_so():
    return ensure_built("imm")


# ---------------------------------------------------------------- 1. header, exports, kernels, audit, resources
def test_library_exports_and_binds_every_declared_function(imm_so):
    assert_exports_and_binds(imm, HEADER, "qim", imm_so, ["qim_last_error", "qim_launch_census_begin", "qim_launch_census_end", "qim_launch_count", "qim_mix", "qim_mix_host", "qim_update"])


def test_kernels_are_its_own_and_exactly_five(imm_so):
    mine, main = _kernels(imm_so), _kernels(_lib.LIB_PATH)
    assert mine and main and not mine & main, sorted(mine & main)
    ids = {_lib.demangle(m) for m in mine}
    assert len(ids) == N_KERNELS, sorted(ids)
    mixes = {i for i in ids if i.startswith("void qle::k_imm_mix<")}
    assert {re.match(r"void qle::k_imm_mix<(\w+), (\w+)>", i).groups() for i in mixes} == {(t, c) for t in ("float", "double") for c in ("true", "false")}
    assert len(mixes) == 4 and [i for i in ids - mixes if i.startswith("qle::k_imm_update(")] == sorted(ids - mixes)
    assert not any("k_imm" in _lib.demangle(m) for m in main)


def test_library_links_the_hip_runtime_only(imm_so):
    needed = _needed(imm_so)
    assert any(n.startswith("libamdhip64") for n in needed), needed
    assert not any("qle_" in n for n in needed), needed
    assert not re.findall(rb"libqle_[a-z]+\.so", open(imm_so, "rb").read())


@pytest.fixture(scope="module")
def audit(imm_so):
    return run_audit("imm")


def test_generated_device_code_passes_the_stale_exec_audit(audit):
    assert_audit_counts(audit[0], "imm", N_KERNELS)


def test_no_kernel_uses_scratch_memory_or_lds(audit):
    """The kernel descriptors of the generated assembly, read as tests/test_bank_cpu.py reads them: 0 bytes of private segment and no
    LDS for all five.  One wave per workgroup: the register file of a SIMD (512 per lane) is the limit, not 256."""
    r, asm = audit
    assert r.returncode == 0
    found, meta = kernel_descriptors(asm)
    assert len(found) == N_KERNELS and all("k_imm_" in k for k in found), sorted(found)
    for name, (scratch, lds, vgpr) in found.items():
        print(f"{name.split('(')[0]}: scratch {scratch} B, LDS {lds} B, registers {vgpr}")
        assert scratch == 0, (name, scratch)
        assert lds == 0, (name, lds)
        assert vgpr <= 512, (name, vgpr)
    assert scratch_free(meta), meta


# ---------------------------------------------------------------- 2. refusals, before any GPU call
_view = functools.partial(side_lib_util._view, batch=128)


def test_library_refuses_before_any_gpu_call(imm_so):
    """No GPU here: a call that got as far as the HIP runtime would return QLE_ERR_HIP (or crash on the fake pointers), not these."""
    K = imm.imm_lib()
    B = C.byref
    INV, STATE = _lib.QLE_ERR_INVALID, _lib.QLE_ERR_STATE
    v, par, mr = _view(), _lib.QleParams(), _lib.QleParams()
    mr.multirate_ekf = 1
    LM, PI, LC, MX, MK, LL = 0x7F1000000000, 0x7F2000000000, 0x7F3000000000, 0x7F4000000000, 0x7F5000000000, 0x7F6000000000

    def mix(v_=B(v), p=B(par), M=4, lm=LM, pi=PI, mask=MK, lc=LC, mx=MX):
        return K.qim_mix(v_, p, M, lm, pi, mask, lc, mx)

    def upd(v_=B(v), M=4, lc=LC, ll=LL, mask=MK, lo=-30.0, lm=LM):
        return K.qim_update(v_, M, lc, ll, mask, lo, lm)

    err = lambda: K.qim_last_error()
    for call in (mix, upd):
        assert call(v_=None) == INV and b"view" in err()
        for size in (0, C.sizeof(v) - 8, C.sizeof(v) + 8):                  # a wrong struct_size
            bad = _view(); bad.struct_size = size
            assert call(v_=B(bad)) == INV and b"struct_size" in err()
        for M in (0, 1, 3, 6, 12, 48, 128, -2, -64, 2 ** 31 - 1, -2 ** 31):  # members not a power of two in 2..64
            assert call(M=M) == INV and b"power of two" in err(), M
        for batch, M in ((100, 8), (140, 64), (130, 4), (2, 4)):              # batch % members != 0
            assert call(v_=B(_view(batch=batch)), M=M) == INV and b"multiple" in err(), (batch, M)
        odd = _view(); odd.state = 0x7F0000000008                            # misaligned records
        assert call(v_=B(odd)) == INV and b"aligned" in err()
        for wrong in (dict(dtype=7), dict(n=12), dict(batch=0), dict(n=15, compact=1)):
            assert call(v_=B(_view(**wrong))) == INV
    assert mix(lm=None) == INV and b"logmu is null" in err()                 # a NULL logmu, Pi or logc
    assert mix(pi=None) == INV and b"Pi is null" in err()
    assert mix(lc=None) == INV and b"logc is null" in err()
    assert mix(p=None) == INV and b"params" in err()
    for kw in (dict(lm=LM + 4), dict(pi=PI + 4), dict(lc=LC + 4)):           # misaligned pointers
        assert mix(**kw) == INV and b"aligned" in err(), kw
    assert mix(p=B(mr)) == STATE and b"multirate" in err()                   # multirate_ekf: the gate's and the scorer's rule
    assert mix(p=B(mr), M=3) == STATE                                        # ... ahead of everything refused about the view
    assert upd(lc=None) == INV and upd(ll=None) == INV and upd(lm=None) == INV
    for kw in (dict(lc=LC + 4), dict(ll=LL + 2), dict(lm=LM + 1)):
        assert upd(**kw) == INV and b"aligned" in err(), kw
    assert upd(lo=float("nan")) == INV and b"NaN" in err()                   # a NaN logmu_min
    # the host entry refuses the same, before it allocates anything
    lm, pi, lc, mx = np.zeros(128), np.eye(4), np.zeros(128), np.zeros(128, np.uint8)
    pd, pu = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    host = lambda M=4, v_=B(v), p=B(par), lm_=lm.ctypes.data_as(pd), pi_=pi.ctypes.data_as(pd), lc_=lc.ctypes.data_as(pd): K.qim_mix_host(   # noqa: E731
        v_, p, M, lm_, pi_, None, lc_, mx.ctypes.data_as(pu))
    assert host(M=3) == INV and host(M=128) == INV and host(v_=None) == INV and host(v_=B(_view(batch=100)), M=8) == INV
    assert host(lm_=None) == INV and host(pi_=None) == INV and host(lc_=None) == INV and host(p=None) == INV
    assert host(p=B(mr)) == STATE
    assert K.qim_launch_count() == 0


# ---------------------------------------------------------------- 3. the Python binding, without a native call
class Fake(FakeTensor):
    def fill_(self, v):
        return self

    def clone(self):
        return self


class FakeEkf:
    batch, dtype, device, num_states = 128, _lib.QLE_F32, 0, 15
    _h = None

    def __init__(self, multirate=0):
        self.params = _lib.QleParams()
        self.params.multirate_ekf = multirate


def good_Pi(M=4):
    return np.full((M, M), 0.1 / (M - 1)) + np.eye(M) * (0.9 - 0.1 / (M - 1))


def test_python_checks_Pi_and_refuses_multirate_before_any_native_call(monkeypatch):
    forbid_native(monkeypatch)
    monkeypatch.setattr(imm, "_upload", lambda device, a: Fake(a.shape, dtype="float64"))   # what a good call reaches: no GPU here
    monkeypatch.setattr(imm._t, "empty", lambda device, shape, dn, zero=False: Fake(tuple(shape), dtype=dn))
    io = devio.DeviceIO(FakeEkf())
    P4 = good_Pi()
    assert np.abs(P4.sum(axis=1) - 1).max() < 1e-15
    neg = P4.copy(); neg[1, 1] += neg[1, 2] + 0.05; neg[1, 2] = -0.05          # a negative entry in a row that still adds to 1
    short = P4.copy(); short[2] *= 0.9                                        # a row adding to 0.9
    nan = P4.copy(); nan[0, 3] = np.nan
    inf = P4.copy(); inf[3, 0] = np.inf
    off = P4.copy(); off[0, 0] += 1e-9                                        # beyond 1e-12
    for bad, what in ((neg, ">= 0"), (short, "add to 1"), (nan, "finite"), (inf, "finite"), (off, "add to 1"), (good_Pi(8), "shape"),
                      (P4[:3], "shape"), (P4.ravel(), "shape"), (np.zeros((4, 4, 1)), "shape"), ("no", "Pi"), (None, "Pi")):
        with pytest.raises(ValueError, match=what):
            io.imm(4, bad)
        with pytest.raises(ValueError, match=what):
            imm.mix_host(io.ekf, 4, np.zeros(128), bad, None)
    for M in (0, 1, 3, 6, 128, 2.5, True):                                    # the geometry is the bank's
        with pytest.raises(ValueError):
            io.imm(M, P4)
    with pytest.raises(ValueError, match="NaN"):
        io.imm(4, P4, logmu_min=float("nan"))
    with pytest.raises(ValueError, match="logmu0"):
        io.imm(4, P4, logmu0=np.zeros(64))
    with pytest.raises(ValueError):
        io.imm(4, P4, logmu0=FakeTensor((128,), dtype="float32"))
    mrio = devio.DeviceIO(FakeEkf(multirate=1))                               # a multirate handle is refused here
    with pytest.raises(_lib.QleError, match="multirate") as e:
        mrio.imm(4, P4)
    assert e.value.code == _lib.QLE_ERR_STATE
    with pytest.raises(_lib.QleError, match="multirate"):
        imm.mix_host(mrio.ekf, 4, np.zeros(128), P4, None)
    m = io.imm(4, P4.tolist(), logmu_min=-np.inf)                             # a nested list; -inf disables the floor
    assert (m.members, m.banks, m.logmu_min, m.logc) == (4, 32, -np.inf, None) and m.logmu.shape == (128,)
    assert io.imm(2, np.eye(2)).logmu_min == pytest.approx(np.log(1e-12))
    with pytest.raises(ValueError, match="mix first"):
        m.update(FakeTensor((128,), dtype="float64"))
    for bad_m in (np.zeros(128, np.uint8), FakeTensor((128,), dtype="float32"), FakeTensor((32,), dtype="uint8")):
        with pytest.raises(ValueError):
            m.mix(mask=bad_m)
    with pytest.raises(AssertionError, match="native library"):
        m.mix(mask=FakeTensor((128,), dtype="uint8"))   # a good call is what reaches the libraries


# ---------------------------------------------------------------- 4. the truth, pinned by forms that do not share its code
def shared_quaternion(rng, x, M):
    """one quaternion per bank (stateless members stay so)"""
    G = x.shape[0] // M
    qb = rng.normal(size=(G, 4)); qb /= np.linalg.norm(qb, axis=1, keepdims=True)
    has = x[:, 6:10].any(axis=1)
    x[has, 6:10] = qb.repeat(M, axis=0)[has]
    return x


def vec(x, n):
    """(r, v, 0, ab, wb): the vector states in the order of the covariance, the attitude left out"""
    y = np.zeros((x.shape[0], 15)); y[:, 0:6] = x[:, 0:6]; y[:, 9:15] = x[:, 10:16]
    return y[:, :n]


@pytest.mark.parametrize("M,n,shared", [(2, 15, False), (8, 9, False), (8, 15, True), (64, 15, True), (4, 15, False)])
def test_truth_conserves_the_first_two_moments(M, n, shared):
    """sum_j c_j x0_j = sum_i mu_i x_i and sum_j c_j (P0_j + (x0_j - xbar)(.)^T) = sum_i mu_i (P_i + (x_i - xbar)(.)^T) for a
    row-stochastic Pi without zeros and banks whose members are all valid (every member is mixed): exactly for the r, v, ab, wb words and the covariance blocks among
    them; with members that share one quaternion for everything (the attitude rows and columns are then those of P alone)."""
    rng = np.random.default_rng(300 + M + n)
    G = 5
    x, P, logmu, mask = bu.make_case(rng, M, G, n, "f64", empty_bank=False, specials=False)   # an invalid j would keep its share c_j
    if shared:
        x = shared_quaternion(rng, x, M)
    x[::3, 6:10] *= -1.0                                                      # stored as -q: the same attitude
    Pi = rng.uniform(0.05, 1.0, size=(M, M)); Pi /= Pi.sum(axis=1, keepdims=True)
    ref = iu.mix_ref(x, P, logmu, Pi, mask, M)
    keep = np.array([k for k in range(n) if shared or not 6 <= k < 9])        # without a shared attitude: the vector words only
    worst_x = worst_P = 0.0
    for g in range(G):
        s = slice(g * M, (g + 1) * M)
        valid = (mask[s] != 0) & x[s, 6:10].any(axis=1) & np.isfinite(logmu[s])
        if valid.sum() < 2:
            assert not ref.mixed[s].any()
            continue
        assert (ref.mixed[s] == valid).all()
        mu, c = iu.mode_probabilities(valid, logmu[s])[valid], ref.c[s][valid]
        assert abs(c.sum() - 1.0) < 8e-16
        y, y0 = vec(x[s][valid], n), vec(ref.x[s][valid], n)
        before, after = (mu[:, None] * y).sum(axis=0), (c[:, None] * y0).sum(axis=0)
        scale = (mu[:, None] * np.abs(y)).sum(axis=0) + (c[:, None] * np.abs(y0)).sum(axis=0)
        worst_x = max(worst_x, bu._rel(np.abs(before - after), scale))
        ybar = before
        e, e0 = y - ybar, y0 - ybar
        t = mu[:, None, None] * (P[s][valid] + e[:, :, None] * e[:, None, :])
        t0 = c[:, None, None] * (ref.P[s][valid] + e0[:, :, None] * e0[:, None, :])
        dev = np.abs(t.sum(axis=0) - t0.sum(axis=0))[np.ix_(keep, keep)]
        worst_P = max(worst_P, bu._rel(dev, (np.abs(t).sum(axis=0) + np.abs(t0).sum(axis=0))[np.ix_(keep, keep)]))
        if shared:
            q, q0 = x[s][valid][:, 6:10], ref.x[s][valid][:, 6:10]
            assert np.minimum(np.abs(q - q0).max(axis=1), np.abs(q + q0).max(axis=1)).max() < 4e-16   # d_theta = 0: the shared attitude
    print(f"IMM truth M={M} n={n} shared={shared}: conservation x {worst_x:.2e} P {worst_P:.2e} of the sum of absolute terms")
    assert worst_x < 16 * 2.0 ** -53 and worst_P < 16 * 2.0 ** -53, (worst_x, worst_P)   # a few fp64 roundings


@pytest.mark.parametrize("M,n", [(2, 15), (8, 9), (64, 15)])
def test_truth_with_a_rank_one_Pi_is_the_fused_estimate(M, n):
    """Every row of Pi the same distribution p: c_j = p_j and mu_{i|j} = mu_i for every j, so with members that share one quaternion every
    mixed member's record is the bank's fused estimate under the same log-weights -- `bank_util.fuse_ref`, which has its own reference
    member, its own sums, and is pinned against the mixture covariance by tests/test_bank_cpu.py."""
    rng = np.random.default_rng(400 + M + n)
    G = 5
    x, P, logmu, mask = bu.make_case(rng, M, G, n, "f64", empty_bank=False)
    x = shared_quaternion(rng, x, M)
    p = rng.uniform(0.05, 1.0, size=M); p /= p.sum()
    ref = iu.mix_ref(x, P, logmu, np.tile(p, (M, 1)), mask, M)
    fz = bu.fuse_ref(x, P, logmu, mask, M)
    worst = {"x": 0.0, "q": 0.0, "P": 0.0, "logc": 0.0}
    for g in range(G):
        for k in np.flatnonzero(ref.mixed[g * M:(g + 1) * M]) + g * M:
            keep = [w for w in range(16) if not 6 <= w < 10]
            sx = np.concatenate([fz.sx[g, 0:6] + ref.sx[k, 0:6], fz.sx[g, 9:15] + ref.sx[k, 9:15]])
            worst["x"] = max(worst["x"], bu._rel(np.abs(ref.x[k, keep] - fz.x[g, keep]), sx))
            worst["q"] = max(worst["q"], float(min(np.abs(ref.x[k, 6:10] - fz.x[g, 6:10]).max(), np.abs(ref.x[k, 6:10] + fz.x[g, 6:10]).max())))
            worst["P"] = max(worst["P"], bu._rel(np.abs(ref.P[k] - fz.P[g]), ref.sP[k] + fz.sP[g]))
            worst["logc"] = max(worst["logc"], abs(ref.c[k] - p[k - g * M]) / p[k - g * M])
    assert ref.mixed.sum() >= 4                                                # M = 2: two of five banks keep both members
    print(f"IMM truth M={M} n={n}: rank-one Pi against fuse_ref " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert all(v < 16 * 2.0 ** -53 for v in worst.values()), worst            # the rounding level of the conservation check


@pytest.mark.parametrize("M,n", [(2, 15), (8, 9), (64, 15)])
def test_truth_with_an_identity_Pi_mixes_nothing(M, n):
    rng = np.random.default_rng(500 + M + n)
    x, P, logmu, mask = bu.make_case(rng, M, 5, n, "f64")
    ref = iu.mix_ref(x, P, logmu, np.eye(M), mask, M)
    assert not ref.mixed.any() and np.array_equal(ref.x, x) and np.array_equal(ref.P, P)
    for g in range(5):
        s = slice(g * M, (g + 1) * M)
        valid = (mask[s] != 0) & x[s, 6:10].any(axis=1) & np.isfinite(logmu[s])
        mu = iu.mode_probabilities(valid, logmu[s])
        assert np.array_equal(ref.logc[s][valid], np.log(mu[valid])) and np.isneginf(ref.logc[s][~valid]).all()   # the normalised logmu


# ---------------------------------------------------------------- 5. the arithmetic on the host, once more under the sanitizers
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/cpp/imm_harness.cpp: the arithmetic of ekf_imm.hpp compiled by g++ (the HIP headers define the device decorators away),
    once as it is and once as a stand-alone program under AddressSanitizer and UBSan."""
    return host_harness.build("imm_harness", tmp_path_factory)


def run_mix(exe, tmp, dtype, compact, M, x, P, logmu, mask, Pi):
    B, n = x.shape[0], P.shape[1]
    per = np.concatenate([x, host_harness.full_P(P, compact), logmu[:, None], mask[:, None].astype(np.float64)], axis=1)
    o = host_harness.run(exe, tmp, [B, int(dtype == "f64"), int(compact), M], [Pi, per], (B, 243), argv=("mix",))
    Pm = o[:, 18:].reshape(B, 15, 15)
    assert not Pm[:, n:, :].any() and not Pm[:, :, n:].any()
    return o[:, 0], o[:, 1] != 0, o[:, 2:18], Pm[:, :n, :n].copy()


GRID = [(M, G, d, r) for M, G in iu.SHAPES for d in ("f64", "f32") for r in iu.RECORDS]


@pytest.mark.parametrize("M,G,dtype,record", GRID, ids=[f"M{M}-{d}-{r}" for M, G, d, r in GRID])
def test_host_compiled_mixing_matches_the_truth(harness, tmp_path, M, G, dtype, record):
    """At the shapes and record kinds of tests/test_gpu_imm.py: the worst deviation is taken over as many banks as the GPU test draws."""
    n, compact = iu.RECORDS[record]
    rng = np.random.default_rng(3000 + M + n)
    x, P, logmu, mask, Pi = iu.make_case(rng, M, G, n, dtype)
    ref = iu.mix_ref(x, P, logmu, Pi, mask, M)
    assert not ref.mixed[-M:].any() and np.isneginf(ref.logc[-M:]).all() and ref.mixed.sum() >= (G - 1) // 2
    for exe in harness:
        logc, mixed, xm, Pm = run_mix(exe, tmp_path, dtype, compact, M, x, P, logmu, mask, Pi)
        np.testing.assert_array_equal(mixed, ref.mixed)                      # exact: which members are mixed, where logc is -inf,
        np.testing.assert_array_equal(np.isneginf(logc), np.isneginf(ref.logc))
        np.testing.assert_array_equal(xm[~mixed], x[~mixed])                 # ... and every unmixed record
        np.testing.assert_array_equal(Pm[~mixed], P[~mixed])
        assert np.array_equal(Pm, Pm.transpose(0, 2, 1)) and np.isfinite(xm).all() and np.isfinite(Pm).all()
        dev = iu.deviations(logc, xm, Pm, ref)
        tol = iu.TOL[dtype]
        print(f"IMM host M={M} {dtype} {record}: " + " ".join(f"{k} {v:.2e} ({v / tol[k]:.3f} of {tol[k]:.0e})" for k, v in dev.items()))
        assert all(dev[k] <= tol[k] for k in dev), (dev, tol)


@pytest.mark.parametrize("M,G", iu.SHAPES, ids=[f"M{M}" for M, _ in iu.SHAPES])
def test_host_compiled_recursion_matches_the_truth(harness, tmp_path, M, G):
    rng = np.random.default_rng(3500 + M)
    logc, loglik, mask = iu.update_case(rng, M, G)
    for lo in (np.log(1e-12), -np.inf, -3.0):
        ref, scale = iu.update_ref(logc, loglik, mask, lo, M)
        if lo > -np.inf:
            assert (ref == lo).any() and (ref[mask != 0][np.isfinite(logc[mask != 0])] >= lo).all()   # the floor is applied
        else:
            assert np.isneginf(ref[np.isneginf(loglik) & (mask != 0) & np.isfinite(logc)]).all()       # -inf leaves -inf
        assert np.isneginf(ref[(mask == 0) | ~np.isfinite(logc)]).all()
        for exe in harness:
            got = host_harness.run(exe, tmp_path, [M * G, M, lo], [np.stack([logc, loglik, mask.astype(np.float64)], axis=1)], -1, argv=("update",))
            np.testing.assert_array_equal(np.isneginf(got), np.isneginf(ref))
            np.testing.assert_array_equal(got == lo, ref == lo)
            fin_ = np.isfinite(ref)
            dev = bu._rel(np.abs(got[fin_] - ref[fin_]), scale[fin_])
            print(f"IMM host update M={M} logmu_min={lo:.3g}: {dev:.2e} ({dev / iu.TOL_UPDATE:.3f} of {iu.TOL_UPDATE:.1e})")
            assert dev <= iu.TOL_UPDATE
