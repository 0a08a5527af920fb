"""Every kernel instantiation of the side libraries, launched and checked (tests/side_variant_table.py lists them; the CPU test holds
the list to the built libraries).

Every row creates its handle with the record kind forced (QLE_COMPACT, QLE_QUAD=0; the policy and the view are asserted, so that a
compact9 row cannot silently run on full records), sets the row's state, makes ONE call inside the side libraries' launch census
(quadrotor_landing_amd.side_launch_census) and the tick library's, asserts that the side census names exactly the row's kernels, and
compares every live filter with the row's reference under the tolerance that library states for the dtype (gate_util.TOL,
score_util.TOL["gpu"], adapt_util.TOL["gpu"], consistency_util's bars, lookahead_util.STEP_TOL per tick, bank_util.TOL, imm_util.TOL;
bits where the library only moves words; side_variant_table.ROW_TOL names the two rows held to a measured tolerance instead, and why).  A read-only call must leave every word of the record array as it was.  The inputs and what
keeps a row from hiding a failure are side_variant_table.Inputs / conditions, checked on the CPU; every comparison goes through
util.note, so tests/tolerances_side.md can be regenerated from a run (QLE_TOL_RECORD, tests/make_tolerances.py)."""
import ctypes as C

import numpy as np
import pytest

import adapt_util as au
import bank_util as bu
import consistency_util as cu
import gate_util as gu
import health_util as hu
import imm_util as iu
import lookahead_util as lu
import quadrotor_landing_amd as qla
import score_util as su_score
import side_variant_table as st
import stateio_util as su
from quadrotor_landing_amd import _lib, devio
from util import note

pytestmark = pytest.mark.gpu

NP_T = {"f32": np.float32, "f64": np.float64}
TORCH_T = {"f32": "float32", "f64": "float64"}


def _torch():
    import torch as t
    return t


@pytest.fixture(autouse=True)
def torch_first():
    """torch is imported before the first handle of a test exists: a torch that is first imported after the engine has initialised the
    HIP runtime reports no GPU."""
    return _torch()


def dev(a, dtype=None):
    """a numpy array as a device tensor (dtype: "f32" / "f64", the values are representable: the cast is exact)"""
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(NP_T[dtype]))
    return _torch().from_numpy(a).to("cuda:0")


def host(*ts):
    _torch().cuda.synchronize()
    return tuple(None if x is None else x.cpu().numpy() for x in ts)


def held_to(kind, value, tol):
    """util.note on a finite deviation (note itself lets a NaN pass)"""
    assert np.isfinite(value), (kind, value)
    return note(kind, value, tol)


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    u = {1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    same = a.view(u) == b.view(u)
    assert same.all(), f"{what}: {int((~same).sum())} of {same.size} words differ, first at {np.argwhere(~same)[0]}"


class Handle:
    """A handle of the row's record kind holding the row's state (and per-filter parameters), and its DeviceIO."""

    def __init__(self, row, d, monkeypatch, batch=None, x=None, P=None, pfp="row", state=True):
        n, compact = st.RECORDS[row["record"]]
        monkeypatch.setenv("QLE_COMPACT", "1" if compact else "0")   # read at handle creation, as tests/test_gpu_lookahead.make_handle sets them
        monkeypatch.setenv("QLE_QUAD", "0")
        self.ekf = qla.BatchedRelativePoseEKF(d.B if batch is None else batch, row["dtype"], params=qla.make_params(**d.kw))
        monkeypatch.delenv("QLE_COMPACT"); monkeypatch.delenv("QLE_QUAD")
        self.io = qla.DeviceIO(self.ekf)
        v = self.io._view()
        assert self.ekf.num_states == n and self.ekf.policy()["record_words"] == st.RECORD_WORDS[compact]
        assert bool(v.compact) == compact and v.num_states == n and v.record_words == st.RECORD_WORDS[compact]
        if state:
            self.ekf.set_state(d.x if x is None else x, d.P if P is None else P)
        pfp = d.pfp if isinstance(pfp, str) else pfp
        if pfp is not None:
            self.ekf.set_filter_params(pfp)
            same_bits(self.ekf.get_filter_params(), pfp, "the per-filter parameters as the device holds them")

    def words(self):
        """every word of the record array"""
        self.ekf.synchronize()
        return su.raw_read(self.io._view())

    def close(self):
        self.io.close()
        self.ekf.close()


def census(row, fn, tick_kernels=None):
    """fn() inside both censuses -> its result; the side census must name exactly the row's kernels.  tick_kernels: whether the tick
    library must have launched something (None: not asked)"""
    with qla.side_launch_census() as side, qla.launch_census() as tick:
        out = fn()
    got = {(lib, st.kernel_id(n)) for lib, names in side.items() for n in names}
    assert got == set(row["kernels"]), f"{row['id']}: launched {sorted(got)}, expected {sorted(row['kernels'])}"
    assert tick_kernels is None or bool(tick) == tick_kernels, (row["id"], tick)
    return out


def read_only(h, fn):
    """fn() must leave every word of the record array as it was"""
    before = h.words()
    out = fn()
    same_bits(h.words(), before, "the record array behind a read-only call")
    return out


def ids(rows):
    return [r["id"] for r in rows]


def rows(library, call=None):
    return [r for r in st.rows_of(library) if call is None or r["call"] == call]


# ------------------------------------------------------------------------------------------------ devio
@pytest.mark.parametrize("row", rows("devio", "DeviceIO.tick"), ids=ids(rows("devio", "DeviceIO.tick")))
def test_devio_pack(row, monkeypatch):
    """The records DeviceIO.tick packs read back (download_tick) with the bits of a twin slot filled by upload_tick with the same values."""
    d = st.conditions(row)
    S = row["src"]
    u, z = st.held(S, d.u), st.held(S, d.z)                                  # values of the source dtype
    h = Handle(row, d, monkeypatch)
    h.io.tick(dev(u, S))                                                     # makes the private two-tick sequence
    h.ekf.set_state(d.x, d.P)
    census(row, lambda: h.io.tick(dev(u, S), dev(z, S), dev(d.mask)), tick_kernels=True)
    got = h.io._seq.download_tick(1)
    twin = h.ekf.make_inputs(2, [0, 1])
    twin.upload_tick(1, u, z, d.mask)
    for g, r, name in zip(got, twin.download_tick(1), "uzm"):
        same_bits(g, r, f"tick record {name}")
    assert got[2][:64].all() and not got[2].all()
    twin.close(); h.close()


@pytest.mark.parametrize("row", rows("devio", "DeviceIO.state"), ids=ids(rows("devio", "DeviceIO.state")))
def test_devio_state(row, monkeypatch):
    d = st.conditions(row)
    h = Handle(row, d, monkeypatch)
    dst = TORCH_T[row["dst"]]
    x, P = host(*read_only(h, lambda: census(row, lambda: h.io.state(dtype=dst))))
    xh, Ph = h.ekf.get_state()
    same_bits(x, xh.astype(dst), "x"); same_bits(P, Ph.astype(dst), "P")
    assert not x[d.ZERO].any() and not P[d.ZERO].any() and x[d.on, 6:10].any(axis=1).all() and np.abs(P[d.on]).sum() > 0
    h.close()


@pytest.mark.parametrize("row", rows("devio", "DeviceIO.report"), ids=ids(rows("devio", "DeviceIO.report")))
def test_devio_report(row, monkeypatch):
    d = st.conditions(row)
    h = Handle(row, d, monkeypatch)
    dst = TORCH_T[row["dst"]]
    rep = read_only(h, lambda: census(row, lambda: h.io.report(dtype=dst)))
    ref = h.ekf.report()
    assert sorted(rep) == sorted(ref)
    for k in ref:
        same_bits(host(rep[k])[0], ref[k].astype(dst), k)
    assert np.abs(ref["bias"][d.on]).max() > 0.01                            # the static biases are in it
    h.close()


# ------------------------------------------------------------------------------------------------ gate
@pytest.mark.parametrize("row", rows("gate"), ids=ids(rows("gate")))
def test_gate(row, monkeypatch):
    d = st.conditions(row)
    T = row["dtype"]
    h = Handle(row, d, monkeypatch)
    nur, Sr, nisr, _ = d.innovation(row["predict"])
    z, m = dev(d.z, T), dev(d.mask)
    if row["predict"]:
        acc, nis, nu, S = host(*census(row, lambda: h.io.tick(dev(d.u, T), z, m, chi2_max=st.CHI2, return_nis=True), tick_kernels=True))
    else:
        nu, S, nis = host(*read_only(h, lambda: census(row, lambda: h.io.innovation(z, m), tick_kernels=False)))
    on = d.on
    nu, S, nis = nu.astype(np.float64), S.astype(np.float64), nis.astype(np.float64)
    assert np.isnan(nis[~on]).all() and np.isfinite(nis[on]).all() and not nu[~on].any() and not S[~on].any()
    tol = st.tolerances(row, gu.TOL[T])
    held_to("nu", gu.rel(nu[on], nur[on]), tol["nu"]); held_to("S", gu.rel(S[on], Sr[on]), tol["S"])
    held_to("nis", np.abs(nis[on] / nisr[on] - 1).max(), tol["nis"])
    if row["predict"]:
        far = np.abs(nisr / st.CHI2 - 1) > 1e-3                              # the existing rule: clear of the threshold
        assert far[on].sum() >= 0.98 * on.sum()
        want = on & (nisr <= st.CHI2)
        np.testing.assert_array_equal(acc[far | ~on] != 0, want[far | ~on])
        assert acc[on].any() and not acc[on].all() and not acc[d.BIG]
        xa, Pa = h.ekf.get_state()                                            # the tick behind the gate applied exactly the accepted corrections
        moved = np.abs(xa - d.x).max(axis=1) > 0
        assert moved[on].all() and not moved[d.ZERO]
    h.close()


# ------------------------------------------------------------------------------------------------ consistency
@pytest.mark.parametrize("row", rows("consistency"), ids=ids(rows("consistency")))
def test_consistency(row, monkeypatch):
    d = st.conditions(row)
    T, n = row["dtype"], st.RECORDS[row["record"]][0]
    h = Handle(row, d, monkeypatch)
    nees, err, summ = host(*read_only(h, lambda: census(row, lambda: h.io.nees(dev(d.xt, T), mask=dev(d.mask), blocks="all", return_err=True,
                                                                                 dtype="float64"), tick_kernels=False)))
    on = d.on
    eref = cu.err_ref(d.x[on], d.xt[on], d.ab[on], d.wb[on], n)
    ref = cu.nees_ref(d.P[on], eref, 31 if n == 15 else 7)
    assert np.isfinite(nees[on]).all() and np.isnan(nees[~on]).all() and not err[~on].any()
    held_to("nees / bar", cu.nees_ratio(nees[on], ref, d.P[on], T), 1.0)
    held_to("err / bar", cu.err_ratio(err[on], eref, T), 1.0)
    s = dict(zip(qla.consistency.SUMMARY_FIELDS, summ))
    assert s["count"] == on.sum() and s["n_not_pd"] == 0 and s["n_above"] == 0 and s["dof"] == n
    held_to("summary sum_nees", abs(s["sum_nees"] - nees[on].sum()) / nees[on].sum(), on.sum() * 2.0 ** -52)
    h.close()


# ------------------------------------------------------------------------------------------------ health
@pytest.mark.parametrize("row", rows("health", "DeviceIO.health"), ids=ids(rows("health", "DeviceIO.health")))
def test_health(row, monkeypatch):
    d = st.conditions(row)
    h = Handle(row, d, monkeypatch)
    x, P = h.ekf.get_state()
    ref, _ = hu.classify(x, P, mask=d.mask, **hu.LIMITS)
    status, flagged, summ = host(*read_only(h, lambda: census(row, lambda: h.io.health(mask=dev(d.mask), return_summary=True, **hu.LIMITS), tick_kernels=False)))
    assert np.array_equal(status, ref), (list(np.flatnonzero(status != ref)), list(status[status != ref]), list(ref[status != ref]))
    assert np.array_equal(flagged, (ref != 0).astype(np.uint8)) and np.array_equal(summ, hu.summary_of(ref, 63, x, d.mask))
    want = dict(zip(hu.CASE_NAMES, (0, 1, 1, 2, 4, 0, 8, 0)))
    assert [int(status[i]) for i in d.cases] == [want[k] for k in hu.CASE_NAMES]
    h.close()


@pytest.mark.parametrize("row", rows("health", "DeviceIO.retire"), ids=ids(rows("health", "DeviceIO.retire")))
def test_health_retire(row, monkeypatch):
    d = st.conditions(row)
    h = Handle(row, d, monkeypatch)
    compact = st.RECORDS[row["record"]][1]
    before = h.words()
    x0, P0 = h.ekf.get_state()
    gone = (d.mask != 0) & (np.arange(d.B) >= 64)                            # the mixed bits: tile 0 stays
    census(row, lambda: h.io.retire(dev(gone.astype(np.uint8))))
    after = h.words()
    rec = su.record_offsets(d.B, row["dtype"], su.RECORD_WORDS[compact])
    same_bits(after[rec[~gone]], before[rec[~gone]], "the records of the filters that stay")
    assert not after[rec[gone]].any() and gone.sum() > 30
    x, P = h.ekf.get_state()
    assert not x[gone].any() and not P[gone].any()
    same_bits(x[~gone], x0[~gone], "x of the filters that stay"); same_bits(P[~gone], P0[~gone], "P of the filters that stay")
    h.close()


@pytest.mark.parametrize("row", rows("health", "DeviceIO.reseed"), ids=ids(rows("health", "DeviceIO.reseed")))
def test_health_reseed_ands_the_masks(row, monkeypatch):
    d = st.conditions(row)
    h = Handle(row, d, monkeypatch)
    x, P = h.ekf.get_state()
    ref, _ = hu.classify(x, P, **hu.LIMITS)                                  # reseed classifies every filter; the mask says who has a detection
    status, reseeded = host(*census(row, lambda: h.io.reseed(dev(d.z, row["dtype"]), dev(d.mask), **hu.LIMITS), tick_kernels=True))
    assert np.array_equal(status, ref)
    want = (ref != 0) & (d.mask != 0)
    assert np.array_equal(reseeded != 0, want) and want.any() and ((ref != 0) & (d.mask == 0)).any()
    x1, P1 = h.ekf.get_state()
    assert np.isfinite(x1[want]).all() and np.isfinite(P1[want]).all()
    same_bits(x1[~want], x[~want], "x of the filters that were not reseeded"); same_bits(P1[~want], P[~want], "P of the filters that were not reseeded")
    h.close()


# ------------------------------------------------------------------------------------------------ lookahead
@pytest.mark.parametrize("row", rows("lookahead"), ids=ids(rows("lookahead")))
def test_lookahead(row, monkeypatch):
    d = st.conditions(row)
    T = row["dtype"]
    h = Handle(row, d, monkeypatch)
    f = read_only(h, lambda: census(row, lambda: h.io.lookahead(dev(d.u, T), st.HORIZON, mask=dev(d.mask)), tick_kernels=False))
    xf, Pf = host(*f.state(dtype="float64"))
    on = d.on
    xs, Ps = lu.oracle_trajectory(d.po, d.x[on], d.P[on], d.u[on], st.HORIZON, None if d.pfp is None else d.pfp[on])
    dv = lu.deviations(xf[on], Pf[on], xs[-1], Ps[-1])
    for k, v in dv.items():
        held_to(k, v, st.HORIZON * lu.STEP_TOL[T][k])                           # h predicts in a row: h times the per-step bar (lookahead_util)
    assert not xf[~on].any() and not Pf[~on].any() and np.abs(xf[on] - d.x[on]).max() > 1e-4
    h.close()


# ------------------------------------------------------------------------------------------------ sequence
@pytest.mark.parametrize("row", rows("sequence"), ids=ids(rows("sequence")))
def test_sequence_pack(row, monkeypatch):
    """K = 33 ticks packed by ONE call (two launches of k_sq_pack) read back with the bits of per-tick devio packs."""
    d = st.conditions(row)
    S = row["src"]
    t = _torch()
    K, tags = st.SEQ_K, list(st.SEQ_TAGS)
    U = st.held(S, np.stack([d.u + 0.01 * k for k in range(K)]))
    Z = st.held(S, np.stack([d.z + np.r_[0.001 * j, np.zeros(6)] for j in range(len(tags))]))
    M = np.stack([np.roll(d.mask, 7 * j) for j in range(len(tags))]); M[:, :64] = 1
    h = Handle(row, d, monkeypatch)
    Ud, Zd, Md = dev(U, S), dev(Z, S), dev(M)
    L = qla.sequence.sequence_lib()
    n0 = L.qsq_launch_count()
    seq = census(row, lambda: h.io.sequence(Ud, Zd, tags, Md))
    assert L.qsq_launch_count() - n0 == 2
    twin = h.ekf.make_inputs(K, [int(k in tags) for k in range(K)])
    D, view = devio.devio_lib(), h.io._view()
    for k in range(K):
        iv = _lib.QleInputsView(); iv.struct_size = C.sizeof(iv)
        _lib.check(qla.lib().qle_inputs_get_device_view(twin._h, k, C.byref(iv)))
        u = Ud[k].clone()
        z, m = (Zd[tags.index(k)].clone(), Md[tags.index(k)].clone()) if k in tags else (None, None)
        devio._dcheck(D.qdv_wait_stream(C.byref(view), int(t.cuda.current_stream().cuda_stream)))
        devio._dcheck(D.qdv_pack_inputs(C.byref(view), C.byref(iv), u.data_ptr(), None if z is None else z.data_ptr(), None if m is None else m.data_ptr(),
                                        devio._FLOATS[TORCH_T[S]]))
        t.cuda.synchronize()
    h.ekf.synchronize()
    for k in range(K):
        for g, r, name in zip(seq.inputs.download_tick(k), twin.download_tick(k), "uzm"):
            same_bits(g, r, f"tick {k} {name}")
    assert seq.inputs.download_tick(32)[2][:64].all() and not seq.inputs.download_tick(32)[2].all()
    seq.close(); twin.close(); h.close()


# ------------------------------------------------------------------------------------------------ score
def acc_of(obs, B):
    return np.ascontiguousarray(host(obs.acc)[0][:, :B].T)


@pytest.mark.parametrize("row", rows("score", "Scorer.observe"), ids=ids(rows("score", "Scorer.observe")))
def test_score(row, monkeypatch):
    d = st.conditions(row)
    T = row["dtype"]
    h = Handle(row, d, monkeypatch)
    sc = h.io.scorer()
    read_only(h, lambda: census(row, lambda: sc.observe(dev(d.u, T), dev(d.z, T), dev(d.mask))))
    acc = acc_of(sc, d.B)
    nu, S, nis, _ = d.innovation(True)
    ref = su_score.ScoreRef(d.B)
    scored = ref.add(nu, S, nis, d.on)
    assert np.array_equal(scored, d.on)
    np.testing.assert_array_equal(acc[:, su_score.COUNTS], ref.acc[:, su_score.COUNTS])
    assert (acc[d.on, 0] == 1).all() and not acc[~d.on].any() and not acc[:, 36:].any()
    tol = st.tolerances(row, su_score.TOL["gpu"][T])
    for g, v in su_score.deviations(acc, ref).items():
        if g != "lag":                                                        # one tick: no lag pair yet
            held_to(g, v, tol[g])
    held_to("prev nu", np.abs(acc[:, su_score.PREV] - ref.acc[:, su_score.PREV]).max() / np.abs(ref.acc[:, su_score.PREV]).max(), su_score.TOL["gpu"][T]["nu"])
    h.close()


@pytest.mark.parametrize("row", rows("score", "Scorer.summary"), ids=ids(rows("score", "Scorer.summary")))
def test_score_summary(row, monkeypatch):
    d = st.conditions(row)
    T = row["dtype"]
    h = Handle(row, d, monkeypatch)
    sc = h.io.scorer()
    sc.observe(dev(d.u, T), dev(d.z, T), dev(d.mask))
    pick = np.roll(d.mask, 31)
    s = host(read_only(h, lambda: census(row, lambda: sc.summary(dev(pick)))))[0]
    acc = acc_of(sc, d.B)[pick != 0]
    want, scale = acc[:, :30].sum(axis=0), np.abs(acc[:, :30]).sum(axis=0)
    live = scale > 0
    held_to("summary", (np.abs(s - want)[live] / scale[live]).max(), 1e-12)      # test_gpu_score's bar for the two-stage sum
    assert s[0] == acc[:, 0].sum() > 30 and s[4] == 0 and s[5] == 0 and not s[~live].any()
    h.close()


# ------------------------------------------------------------------------------------------------ bank, imm
@pytest.mark.parametrize("row", rows("bank"), ids=ids(rows("bank")))
def test_bank(row, monkeypatch):
    d = st.conditions(row)
    T, M, G = row["dtype"], row["M"], row["G"]
    h = Handle(row, d, monkeypatch)
    x, P = host(*h.io.state(dtype="float64"))
    ref = bu.fuse_ref(x, P, d.logw, d.mask, M)
    assert ref.best[-1] == -1 and (ref.best[:-1] >= 0).all()
    f = read_only(h, lambda: census(row, lambda: h.io.bank(M).fuse(dev(d.logw), dev(d.mask)), tick_kernels=False))
    xf, Pf = host(*f.state(dtype="float64"))
    w, best = host(f.w, f.best)
    np.testing.assert_array_equal(best, ref.best)
    np.testing.assert_array_equal(w == 0, ref.w == 0)
    assert not xf[-1].any() and not Pf[-1].any() and np.isfinite(xf).all() and np.isfinite(Pf).all() and xf.shape == (G, 16)
    for k, v in bu.deviations(w, xf, Pf, ref).items():
        held_to(k, v, bu.TOL[T][k])
    h.close()


@pytest.mark.parametrize("row", rows("imm", "Imm.mix"), ids=ids(rows("imm", "Imm.mix")))
def test_imm_mix(row, monkeypatch):
    d = st.conditions(row)
    T, M = row["dtype"], row["M"]
    h = Handle(row, d, monkeypatch)
    x, P = host(*h.io.state(dtype="float64"))
    x0, P0 = host(*h.io.state())
    ref = iu.mix_ref(x, P, d.logw, d.Pi, d.mask, M)
    assert not ref.mixed[-M:].any() and ref.mixed.sum() * 2 >= d.B - M
    im = h.io.imm(M, d.Pi, logmu0=d.logw)
    logc, mixed = host(*census(row, lambda: im.mix(dev(d.mask)), tick_kernels=False))
    xm, Pm = host(*h.io.state(dtype="float64"))
    x1, P1 = host(*h.io.state())
    np.testing.assert_array_equal(mixed != 0, ref.mixed)
    np.testing.assert_array_equal(np.isneginf(logc), np.isneginf(ref.logc))
    same_bits(x1[~ref.mixed], x0[~ref.mixed], "x of the unmixed records"); same_bits(P1[~ref.mixed], P0[~ref.mixed], "P of the unmixed records")
    assert np.isfinite(xm).all() and np.isfinite(Pm).all()
    for k, v in iu.deviations(logc, xm, Pm, ref).items():
        held_to(k, v, iu.TOL[T][k])
    h.close()


@pytest.mark.parametrize("row", rows("imm", "Imm.update"), ids=ids(rows("imm", "Imm.update")))
def test_imm_update(row, monkeypatch):
    d = st.conditions(row)
    M, G = row["M"], row["G"]
    h = Handle(row, d, monkeypatch)
    logc, loglik, mask = iu.update_case(d.rng, M, G)
    lo = np.log(1e-12)
    ref, scale = iu.update_ref(logc, loglik, mask, lo, M)
    im = h.io.imm(M, np.eye(M), logmu_min=lo)
    im.logc = dev(logc)
    got = host(read_only(h, lambda: census(row, lambda: im.update(dev(loglik), dev(mask)), tick_kernels=False)))[0]
    fin = np.isfinite(ref)
    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(ref))
    held_to("logmu", bu._rel(np.abs(got[fin] - ref[fin]), scale[fin]), iu.TOL_UPDATE)
    h.close()


# ------------------------------------------------------------------------------------------------ adapt
@pytest.mark.parametrize("row", rows("adapt", "Adapter.observe"), ids=ids(rows("adapt", "Adapter.observe")))
def test_adapt_observe(row, monkeypatch):
    d = st.conditions(row)
    T = row["dtype"]
    h = Handle(row, d, monkeypatch)
    ad = h.io.adapter(window=4)
    before = h.ekf.get_filter_params()
    read_only(h, lambda: census(row, lambda: ad.observe(dev(d.u, T), dev(d.z, T), dev(d.mask))))
    same_bits(h.ekf.get_filter_params(), before, "the parameter records behind observe")
    acc = acc_of(ad, d.B)
    nu, S, nis, xp = d.innovation(True)
    ref = au.AdaptRef(d.B)
    ref.add(d.p, nu, S, nis, xp, d.pfp[:, 18:24], d.on)
    np.testing.assert_array_equal(acc[:, au.COUNTS], ref.acc[:, au.COUNTS])
    assert (acc[d.on, 0] == 1).all() and not acc[~d.on].any()
    for g, v in au.deviations(acc, ref).items():
        held_to(g, v, au.TOL["gpu"][T][g])
    h.close()


@pytest.mark.parametrize("row", rows("adapt", "Adapter.apply"), ids=ids(rows("adapt", "Adapter.apply")))
def test_adapt_apply(row, monkeypatch):
    d = st.conditions(row)
    T = row["dtype"]
    h = Handle(row, d, monkeypatch)
    R0 = np.array(list(d.po.R))
    lo, hi = R0 / 2, R0 * 3                                                   # narrow bounds: some components clamp, some do not
    ad = h.io.adapter(window=1, n_min=1, R_lo=lo, R_hi=hi)
    ad.observe(dev(d.u, T), dev(d.z, T), dev(d.mask))
    acc0 = acc_of(ad, d.B)
    pfp0 = h.ekf.get_filter_params()
    R, applied = host(*read_only(h, lambda: census(row, lambda: ad.apply())))
    acc_want, R_want, ap_want, clamped = au.apply_ref(acc0, pfp0[:, 18:24], 1.0, 1, lo, hi, T)
    assert np.array_equal(applied != 0, ap_want) and np.array_equal(ap_want, d.on) and clamped.any() and not clamped[ap_want].all()
    pfp1 = h.ekf.get_filter_params()
    same_bits(R, pfp1[:, 18:24], "the R returned and the R in force")
    same_bits(pfp1[:, :18], pfp0[:, :18], "the other parameter words"); same_bits(pfp1[~ap_want], pfp0[~ap_want], "the records of the filters not applied")
    rel, eq = au.apply_error(R[ap_want], R_want[ap_want], clamped[ap_want])
    held_to("applied R", rel, au.APPLY_TOL[T])
    assert eq
    np.testing.assert_array_equal(acc_of(ad, d.B), acc_want)
    h.close()


# ------------------------------------------------------------------------------------------------ stateio
@pytest.mark.parametrize("row", rows("stateio", "DeviceIO.set_state"), ids=ids(rows("stateio", "DeviceIO.set_state")))
def test_stateio_pack(row, monkeypatch):
    d = st.conditions(row)
    T, S = row["dtype"], row["src"]
    n, compact = st.RECORDS[row["record"]]
    h = Handle(row, d, monkeypatch)
    prior = su.sentinel(d.B, T, seed=11)
    su.raw_write(h.io._view(), prior)
    x, P = su.random_state(d.B, n, seed=d.B + n, dtype=S)                    # values of the source dtype, P not symmetric
    x[d.ZERO], P[d.ZERO] = 0.0, 0.0
    census(row, lambda: h.io.set_state(dev(x, S), dev(P, S), dev(d.mask)))
    same_bits(h.words(), su.expected_pack(prior, d.B, T, compact, x, P, d.mask), "the whole record array after the masked pack")
    twin = Handle(row, d, monkeypatch, state=False)                          # and unmasked: the bits of the host set_state
    twin.ekf.set_state(x, P)
    h.io.set_state(dev(x, S), dev(P, S))
    for got, ref, name in zip(h.ekf.get_state(), twin.ekf.get_state(), "xP"):
        same_bits(got, ref, f"{name} against the host set_state")
    rec = su.record_offsets(d.B, T, su.RECORD_WORDS[compact])
    same_bits(h.words()[rec], twin.words()[rec], "the record words against the host set_state")
    twin.close(); h.close()


@pytest.mark.parametrize("row", rows("stateio", "DeviceIO.restore"), ids=ids(rows("stateio", "DeviceIO.restore")))
def test_stateio_copy(row, monkeypatch):
    """A 165-filter destination indexed into a snapshot of a 70-filter source: duplicates, one index out of range, masked filters."""
    d = st.conditions(row)
    T = row["dtype"]
    compact = st.RECORDS[row["record"]][1]
    wp = row["with_params"]
    sB = st.SRC_B
    src = Handle(row, d, monkeypatch, batch=sB, x=d.x[:sB], P=d.P[:sB], pfp=None if d.pfp is None else d.pfp[-sB:])
    dst = Handle(row, d, monkeypatch)
    first, second = su.sentinel(sB, T, seed=21), su.sentinel(d.B, T, seed=22, offset=0.25)
    su.raw_write(src.io._view(), first); su.raw_write(dst.io._view(), second)
    snap = src.io.snapshot(with_params=wp)
    index = d.rng.integers(0, sB, d.B).astype(np.int32)
    index[5], index[6], index[64] = sB, -1, index[0]                          # out of range twice, a duplicate across tiles
    written = host(census(row, lambda: dst.io.restore(snap, mask=dev(d.mask), index=dev(index), with_params=wp)))[0]
    want, ok = su.expected_copy(first, second, sB, d.B, T, compact, index, d.mask)
    same_bits(dst.words(), want, "the whole destination array")
    assert np.array_equal(written, ok) and not ok[5] and not ok[6] and 30 < ok.sum() < d.B
    if wp:
        pfp = d.pfp.copy(); pfp[ok != 0] = d.pfp[-sB:][index[ok != 0]]
        same_bits(dst.ekf.get_filter_params(), pfp, "the parameter records")
        same_bits(src.ekf.get_filter_params(), d.pfp[-sB:], "the source's parameter records")
    same_bits(src.words(), first, "the source array")
    dst.close(); src.close()
