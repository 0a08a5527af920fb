"""CPU tests of the error budget (include/qle_budget.h, libqle_budget.so, quadrotor_landing_amd/budget.py, csrc/ekf_budget.hpp): the
library builds, exports and binds what its header declares; its generated code passes the stale-EXEC audit over exactly nine kernels,
uses no scratch memory, and LDS in the reduce alone; every kernel of the built code objects has a row in tests/budget_variant_table.py
and every row a kernel, with an exported host handle (the checks of tests/test_side_variant_table_cpu.py applied to this library, which
is outside that table's closed list: the Makefile's SIDE line still names exactly the eleven); every refusal is made before any GPU
call; `Budget`'s derived quantities are the numpy formulas; the inputs of the GPU test satisfy their conditions on the reference
alone; and the host-compilable parts of k_budget -- the 256 words of a lane, error_state, and the recursion of the halving butterfly
over 64-value arrays -- are exact (tests/cpp/budget_harness.cpp, plain and under AddressSanitizer and UBSan).

What the host build does not cover are the kernel's loads, its stores and the exchanges themselves (v_permlane32_swap,
v_permlane16_swap, DPP): tests/test_gpu_budget.py.
"""
import ctypes as C
import os

import numpy as np
import pytest

import budget_variant_table as bv
import consistency_util as cu
import host_harness
import side_variant_table as st
from elf_util import _gfx950_code_objects, _kernels, _symbols
from quadrotor_landing_amd import _lib, budget, devio
from side_lib_util import (FakeTensor, _params, _view, assert_audit_counts, assert_exports_and_binds, ensure_built, kernel_descriptors, run_audit,
                           scratch_free)
from test_side_variant_table_cpu import makefile_side
from util import forbid_native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qle_budget.h")
ELEVEN = ["devio", "gate", "consistency", "health", "lookahead", "sequence", "score", "bank", "imm", "adapt", "stateio"]


@pytest.fixture(scope="module")
def budget_so():
    return ensure_built("budget")


def test_library_exports_and_binds_every_declared_function(budget_so):
    assert_exports_and_binds(budget, HEADER, "qbg", budget_so, ["qbg_budget", "qbg_budget_host", "qbg_groups", "qbg_last_error", "qbg_launch_census_begin",
                                                                "qbg_launch_census_end", "qbg_launch_count"])
    assert "#define QBG_WORDS 256" in open(HEADER).read() and budget.WORDS == bv.WORDS == 256


@pytest.fixture(scope="module")
def audit(budget_so):
    return run_audit("budget")


def test_generated_device_code_passes_the_stale_exec_audit_over_nine_kernels(audit):
    assert_audit_counts(audit[0], "budget", 9)


def test_no_scratch_anywhere_and_no_lds_in_k_budget(audit):
    r, asm = audit
    assert r.returncode == 0
    found, meta = kernel_descriptors(asm)
    assert len(found) == 9 and len([k for k in found if "k_budget<" in k]) == 8, sorted(found)
    for name, (scratch, lds, vgpr) in found.items():
        print(f"{name.split('(')[0]}: scratch {scratch} B, LDS {lds} B, registers {vgpr}")
        assert scratch == 0, (name, scratch)
        assert lds == 0 or "k_budget_reduce" in name, (name, lds)                # the tile sum goes through registers, not the LDS
        assert vgpr <= (256 if "k_budget<float" in name else 512), (name, vgpr)   # fp32: room for two waves per SIMD
    assert scratch_free(meta), meta


def test_the_tile_sum_is_a_halving_butterfly(audit):
    """The exchanges the tile sum is made of are in the generated code, and no ds_bpermute (what 256 wave_sum calls would be)."""
    txt = open(audit[1]).read()
    assert txt.count("v_permlane32_swap") > 0 and txt.count("v_permlane16_swap") > 0 and "row_ror:8" in txt and "quad_perm" in txt
    assert "ds_bpermute" not in txt


# ---------------------------------------------------------------- the table against the built library
@pytest.fixture(scope="module")
def library(budget_so):
    d = open(budget_so, "rb").read()
    return dict(units=len(_gfx950_code_objects(d)), mangled=_kernels(budget_so), dynsym=set(_symbols(d, 11)))


def test_every_kernel_has_a_row_and_every_row_a_kernel(library):
    assert library["units"] > 0 and library["mangled"]
    ids = {st.kernel_id(_lib.demangle(m)) for m in library["mangled"]}
    assert len(ids) == len(library["mangled"]) == 9, sorted(ids)
    rows = bv.covered_kernels()
    assert ids == rows, (sorted(ids - rows), sorted(rows - ids))
    for r in bv.ROWS:
        assert r["kernels"] and r["reference"] and r["record"] in st.RECORDS and r["dtype"] in st.DTYPES and r["library"] == bv.LIBRARY, r["id"]
        assert all(lib == bv.LIBRARY and k.startswith("k_") for lib, k in r["kernels"]), r["id"]


def test_every_kernel_has_an_exported_host_handle(library):
    missing = sorted(library["mangled"] - library["dynsym"])
    assert not missing, [_lib.demangle(m) for m in missing]
    handles = {s for s in library["dynsym"] if s.startswith("_Z") and st.kernel_id(_lib.demangle(s)).split("<")[0] in ("k_budget", "k_budget_reduce")}
    assert handles <= library["mangled"], sorted(handles - library["mangled"])


def test_the_closed_list_stays_closed():
    assert makefile_side() == ELEVEN
    assert set(_lib.SIDE_LIBRARIES) == set(ELEVEN) and "budget" not in _lib.SIDE_LIBRARIES
    assert _lib.OPEN_LIBRARIES == {"budget": budget.BUDGET} and not budget.BUDGET.closed_census
    assert all(s.closed_census for s in _lib.SIDE_LIBRARIES.values())
    assert not st.rows_of("budget")


# ---------------------------------------------------------------- refusals, before any GPU call
def test_library_refuses_before_any_gpu_call(budget_so):
    """No GPU here: a call that got as far as the HIP runtime would return QLE_ERR_HIP (or crash on the fake pointers), not these."""
    K = budget.budget_lib()
    v, p = _view(), _params()
    xt, out = 0x7F1000000000, 0x7F3000000000
    B = C.byref
    INV = _lib.QLE_ERR_INVALID

    def call(v_=B(v), p_=B(p), xt_=xt, td=budget.QBG_F32, rows=100, gt=0, sums=out, err=None, dd=budget.QBG_F32, status=None):
        return K.qbg_budget(v_, p_, xt_, td, rows, None, gt, sums, err, dd, status)

    assert call(v_=None) == INV and b"view" in K.qbg_last_error()
    assert call(p_=None) == INV and call(xt_=None) == INV
    assert call(sums=None) == INV and b"sums" in K.qbg_last_error()
    short = _view(); short.struct_size = C.sizeof(short) - 8
    assert call(v_=B(short)) == INV and b"struct_size" in K.qbg_last_error()
    for rows in (0, 2, 99, 101, -1):
        assert call(rows=rows) == INV and b"true_rows" in K.qbg_last_error()
    assert call(gt=-1) == INV and b"group_tiles" in K.qbg_last_error()
    assert call(td=7) == INV and call(dd=7) == INV
    assert call(xt_=xt + 8) == INV and b"aligned" in K.qbg_last_error()
    assert call(sums=out + 4) == INV and call(err=out + 2) == INV and call(err=out + 4, dd=budget.QBG_F64) == INV
    assert call(p_=B(_params(est_bias=0))) == INV   # the view says 15 states
    hx = np.zeros((100, 16)); hs = np.zeros((1, 256))
    hp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    host = lambda v_, rows, gt, sums: K.qbg_budget_host(v_, B(p), hp(hx), rows, None, gt, sums, None, None)   # noqa: E731
    assert host(B(v), 7, 0, hp(hs)) == INV and host(B(v), 100, -2, hp(hs)) == INV and host(B(short), 100, 0, hp(hs)) == INV
    assert host(B(v), 100, 0, None) == INV and host(None, 100, 0, hp(hs)) == INV
    assert K.qbg_groups(100, -1) < 0 and K.qbg_groups(0, 0) < 0
    assert [K.qbg_groups(165, g) for g in (0, 1, 2, 3, 4)] == [1, 3, 2, 1, 1] == [budget.groups(165, g)[1] for g in (None, 1, 2, 3, 4)]
    assert K.qbg_launch_count() == 0


class FakeEkf:
    batch, dtype, device = 100, _lib.QLE_F32, 0
    _h = None

    def __init__(self, num_states=15, **kw):
        self.num_states = num_states
        self.params = _params(**kw)


class FakeSeq:
    n_ticks = 12


def test_deviceio_refuses_bad_budget_arguments_before_any_gpu_call(monkeypatch):
    ekf = FakeEkf()   # its parameters come from the tick library: made first
    forbid_native(monkeypatch)
    B = 100
    io = devio.DeviceIO(ekf)
    xt = FakeTensor((B, 16))
    bad = [
        dict(x_true=np.zeros((B, 16))),                               # a host array
        dict(x_true=FakeTensor((B, 15))),
        dict(x_true=FakeTensor((2, 16))),
        dict(x_true=FakeTensor((B, 16), dtype="float16")),
        dict(x_true=FakeTensor((B, 16), device="cuda:1")),
        dict(x_true=FakeTensor((B, 16), contiguous=False)),
        dict(x_true=FakeTensor((16,), ptr=0x7F0000000008)),           # not 16-byte aligned
        dict(x_true=xt, mask=FakeTensor((B,), dtype="float32")),
        dict(x_true=xt, group_tiles=-1),
        dict(x_true=xt, group_tiles=1.5),
        dict(x_true=xt, dtype="int32"),
        dict(x_true=xt, out=FakeTensor((1, 256), dtype="float32")),
        dict(x_true=xt, out=FakeTensor((2, 256), dtype="float64")),   # one group
        dict(x_true=xt, group_tiles=1, out=FakeTensor((1, 256), dtype="float64")),   # two groups
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            io.budget(**kw)
    for good in (dict(x_true=xt), dict(x_true=FakeTensor((16,))), dict(x_true=FakeTensor((1, 16), dtype="float64"), group_tiles=1)):
        with pytest.raises(AssertionError, match="native library"):
            io.budget(**good)                                         # a good call is what reaches the libraries
    xs = FakeTensor((3, B, 16))
    for kw in (dict(every=0), dict(every=2.5), dict(every=4, n=13), dict(every=4, t0=-1), dict(every=4, trace_every=4),
               dict(every=4, group_tiles=-1), dict(every=4, mask=FakeTensor((B, 1), dtype="uint8"))):
        with pytest.raises(ValueError):
            io.budget_run(FakeSeq(), xs, **kw)
    with pytest.raises(ValueError):
        io.budget_run(FakeSeq(), FakeTensor((2, B, 16)), every=4)     # J = 3
    with pytest.raises(AssertionError, match="native library"):
        io.budget_run(FakeSeq(), xs, every=4)


# ---------------------------------------------------------------- Budget: the derived quantities
def _numpy_budget(sums):
    n = sums[..., 0]
    E = np.zeros(sums.shape[:-1] + (15, 15)); P = np.zeros_like(E)
    for t, (i, j) in enumerate(bv.TRI):
        E[..., i, j] = E[..., j, i] = sums[..., 16 + t]
        P[..., i, j] = P[..., j, i] = sums[..., 136 + t]
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = sums[..., 1:16] / n[..., None]
        mse, Pm = E / n[..., None, None], P / n[..., None, None]
        dE, dP = np.einsum("...ii->...i", E), np.einsum("...ii->...i", P)
        return dict(n=n, mean=mean, mse=mse, cov=mse - mean[..., :, None] * mean[..., None, :], P_mean=Pm, var_ratio=dE / dP,
                    rms=np.sqrt(dE / n[..., None]), sigma=np.sqrt(dP / n[..., None]))


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_budget_derived_quantities_match_the_numpy_formulas(kind):
    rng = np.random.default_rng(20)
    J, G = 2, 3
    sums = np.zeros((J, G, 256))
    for j in range(J):
        for g in range(G):
            n = int(rng.integers(2, 200))
            e = rng.normal(size=(n, 15)) * rng.uniform(0.01, 2.0, size=15) + rng.normal(size=15) * 0.1
            A = rng.normal(size=(n, 15, 15)); Pm = np.einsum("bij,bkj->bik", A, A)
            sums[j, g] = bv.words_ref(e, np.ones(n, np.uint8), Pm).sum(axis=0)
    sums[1, 2] = 0.0                                                    # an empty group: NaN, not an exception
    ref = _numpy_budget(sums)
    if kind == "torch":
        import torch
        b = budget.Budget(torch.from_numpy(sums.copy()))
        get = lambda a: a.numpy()   # noqa: E731
    else:
        b = budget.Budget(sums.copy())
        get = lambda a: a           # noqa: E731
    empty = np.zeros((J, G), bool); empty[1, 2] = True
    for k, r in ref.items():
        got = get(getattr(b, k))
        assert got.shape == r.shape and got.dtype == np.float64, (k, got.shape, r.shape)
        if k != "n":
            assert np.isnan(got[empty]).all(), k
        full = ~empty
        dev = np.abs(got[full] - r[full]).max() / np.abs(r[full]).max()
        assert dev <= 1e-12, (k, dev)
    both = budget.Budget.combine([budget.Budget(b.sums[0]), budget.Budget(b.sums[1])])
    bv.same_bits(get(both.sums), sums[0] + sums[1], "combine")
    assert get(both.n)[2] == sums[0, 2, 0]
    with pytest.raises(ValueError):
        budget.Budget(sums[..., :255])


# ---------------------------------------------------------------- the inputs of the GPU test, on the reference alone
@pytest.mark.parametrize("row", bv.ROWS, ids=[r["id"] for r in bv.ROWS])
def test_the_reference_alone_satisfies_the_rows_conditions(row):
    d = bv.conditions(row)
    n = st.RECORDS[row["record"]][0]
    live = d.status != bv.OFF
    eref = np.zeros((d.B, n)); eref[live] = cu.err_ref(d.x[live], d.xt[live], d.ab[live], d.wb[live], n)
    w = bv.words_ref(eref, d.status, np.where(np.isfinite(d.P), d.P, 0.0))
    part = bv.tile_partials(w)
    assert part.shape == (3, 256) and np.isfinite(part).all() and (part[:, 0] >= 2).all() and part[:, 0].sum() == (d.status == bv.COUNTED).sum()
    assert not np.array_equal(bv.group_sums(part, 2)[0], bv.group_sums(part, None)[0])


# ---------------------------------------------------------------- the host-compilable parts
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/cpp/budget_harness.cpp compiled by g++ (the HIP headers define the device decorators away), once as it is and once as a
    stand-alone program under AddressSanitizer and UBSan."""
    return host_harness.build("budget_harness", tmp_path_factory)


LANE_CASES = [("f64", "full15"), ("f64", "full9"), ("f64", "compact9"), ("f32", "full15"), ("f32", "full9"), ("f32", "compact9")]


@pytest.fixture(scope="module")
def lane_results(harness, tmp_path_factory):
    """Every case through both builds, once: (inputs, out [B,287]) per (dtype, record); the two builds must agree to the bit."""
    res = {}
    for dtype, record in LANE_CASES:
        row = next(r for r in bv.ROWS if r["dtype"] == dtype and r["record"] == record and r["pfp"])
        d = bv.conditions(row)
        n, compact = st.RECORDS[record]
        per = np.concatenate([d.x, host_harness.full_P(d.P), d.xt, d.ab, d.wb, d.mask[:, None].astype(np.float64)], axis=1)
        outs = [host_harness.run(exe, tmp_path_factory.mktemp("lane"), [d.B, int(dtype == "f64"), int(compact), n, 0], [per], (d.B, 287)) for exe in harness]
        bv.same_bits(outs[0], outs[1], "plain and sanitised build")
        res[dtype, record] = (d, n, outs[0])
    return res


@pytest.mark.parametrize("dtype,record", LANE_CASES, ids=[f"{d}-{r}" for d, r in LANE_CASES])
def test_lane_words_and_error_state(lane_results, dtype, record):
    d, n, o = lane_results[dtype, record]
    words, counted, e, e_nees = o[:, :256], o[:, 256] != 0, o[:, 257:272], o[:, 272:287]
    bv.same_bits(e, e_nees, "error_state against the e of nees_eval")
    np.testing.assert_array_equal(counted, d.status == bv.COUNTED)
    live = d.status != bv.OFF
    ratio = cu.err_ratio(e[live][:, :n], cu.err_ref(d.x[live], d.xt[live], d.ab[live], d.wb[live], n), dtype)
    print(f"{dtype} {record}: err / bar {ratio:.3g}")
    assert ratio <= 1.0
    P = np.where(np.isfinite(d.P), d.P, 0.0)                              # the NaN filter is not counted: its words are zero
    bv.same_bits(words, bv.words_ref(e[:, :n], d.status, P), "the 256 words of every lane")
    assert words[d.status != bv.COUNTED].any() == 0 and (words[counted, 0] == 1.0).all()
    if n == 9:
        assert not words[:, 10:16].any()


def test_halving_butterfly_is_the_xor_butterfly_bit_for_bit(harness, lane_results, tmp_path):
    """tile_reduce over arrays against tile_sum: the words of the fp64 case (ragged last tile, off lanes and the NaN lane as zeros) and
    three tiles of random words over twenty orders of magnitude with mixed signs, where any other association of a sum shows."""
    d, n, o = lane_results["f64", "full15"]
    pad = np.zeros((192, 256)); pad[:d.B] = o[:, :256]
    rng = np.random.default_rng(5)
    rnd = rng.normal(size=(192, 256)) * 10.0 ** rng.uniform(-10, 10, size=(192, 256))
    rnd[150:] = 0.0                                                       # a ragged tile
    tiles = np.concatenate([pad, rnd]).reshape(6, 64, 256)
    ref = np.stack([bv.tile_sum(t) for t in tiles])
    naive = tiles.sum(axis=1)
    assert (naive != ref).mean() > 0.2                                    # the order matters on these inputs
    for exe in harness:
        got = host_harness.run(exe, tmp_path, [6, 1, 0, 15, 1], [tiles], (6, 256))
        bv.same_bits(got, ref, "tile_reduce against tile_sum")
    bv.same_bits(ref[:3], bv.tile_partials(o[:, :256]), "the padding of tile_partials")
