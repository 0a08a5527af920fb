"""Every kernel instantiation of the eleven side libraries (csrc/Makefile, SIDE) as a test case: the side libraries' counterpart of
tests/variant_table.py.  tests/test_side_variant_table_cpu.py holds the table to the built libraries and every row's inputs to the
conditions below; tests/test_gpu_side_variants.py runs every row on the device inside the side libraries' launch census.

The rows are generated from the axis lists below, which restate the dispatch ladder of each <name>_capi.hip (and launch_flags of
side_run_host.hpp).  A ladder that gains a rung, or a kernel that gains an axis, has no row until the list here says so, and the CPU
test names the kernel.  The side kernels read no QLE_* override, so there are no policy axes: every row is held to its reference.

Each row: id, library, call (the Python entry whose launches the census covers), dtype (of the handle), record (full15 / full9 /
compact9: forced at handle creation with QLE_COMPACT and QLE_QUAD=0), direct (orientation method), pfp (per-filter parameters), the
extra axes src / dst (tensor dtype of devio, stateio and sequence), predict (PREDICT of k_pregate), with_params (k_si_copy), M and G
(banks), kernels (the exact set of (library, kernel id) the call launches in side libraries, reduce / tiles kernels and the pack of
the device-tensor boundary included) and reference (which comparison holds it).

Inputs (class Inputs, numpy only, the same on every machine): util.rand_states on B = 165 filters -- two full tiles and a ragged one
of 37 -- rounded to what a handle of the row's dtype holds; a mask with the first tile on and mixed bits elsewhere; one all-zero
("uninitialised") record; one lane whose tag pose is ~170 degrees from its attitude; per-filter parameters drawn as in
test_gpu_variants.Inputs where the row has them.  The bank and IMM rows take bank_util / imm_util's cases (M = 4 x G = 41, ragged, and
M = 64 x G = 3, a bank per tile), whose special members are their masked, stateless and -q records.

What keeps a row from hiding a failure (conditions(row), asserted for every row on the CPU): at least half of the filters are live
and every live filter's reference is finite and positive definite; gate rows see both outcomes at chi2 = 16.81 and at most 2 % of
the live filters lie within 1e-3 of the threshold; health rows see every status bit and no variance within 1e-3 of a limit.
"""
import itertools
import re
import zlib

import numpy as np

import consistency_util as cu
import health_util as hu
import imm_util as iu
import oracle
from gate_util import HW, predict_then_innovation
from innovation_util import CHI2_6_099
from oracle import ekf_np
from util import meas_near, rand_imu, rand_states

T_NAMES = {"f32": "float", "f64": "double"}
DTYPES = ("f32", "f64")
BOOLS = (False, True)
RECORDS = {"full15": (15, False), "full9": (9, False), "compact9": (9, True)}   # name -> (num_states, compact records)
RECORD_WORDS = {False: 136, True: 64}
B = 165                        # two full tiles and a ragged tile of 37
SRC_B = 70                     # stateio copy: the source of another batch size, one tile and 6
BANK_SHAPES = ((4, 41), (64, 3))   # (M, G): B = 164, ragged; a bank that fills a tile
SEQ_K, SEQ_TAGS = 33, (0, 31, 32)  # sequence pack: two chunks of 32, tag slots at both ends of the first and in the second
HORIZON = 2                    # lookahead rows
CHI2 = CHI2_6_099
EXCLUDED = {}                  # (library, kernel id) -> one-line reason it has no row (kept empty)
# Rows that exceed the tolerance their library states, and the one they are held to instead: 10 x the deviation measured on the MI355X
# against the fp64 reference (tests/tolerances_side.md), after the host-compiled arithmetic (tests/cpp/pregate_harness.cpp, the same
# pregate_eval) showed the same deviation on the same inputs.  Both are the fp32 innovation of a tag pose 0.02 .. 0.09 (m, rad) from the
# predicted state: nu_r = r_obs - r is the difference of two positions of 2 .. 4 m, its error of 1 .. 4 ulp of those (0.3e-6 .. 1.7e-6 m)
# is taken relative to the innovation's own largest component, a scale a hundred times below the operands.  gate_util.TOL's 3e-5 was
# measured on innovations of up to 170 degrees in every filter (scale ~3); the host build reaches 5.2e-5 on these rows' inputs.
ROW_TOL = {
    "DeviceIO.tick(chi2_max)-f32-compact9-direct1-predict1": {"nu": 3.4e-4},   # measured 3.31e-5 (host build: 2.3e-5 .. 5.2e-5 over the fp32 rows)
    "Scorer.observe-f32-full15-direct1": {"nu": 3.2e-4},                       # measured 3.14e-5, relative to the sum of |nu| (score_util)
}


def tolerances(row, stated):
    """the tolerances a row is held to: its library's stated ones for the dtype, ROW_TOL's entries over them"""
    return dict(stated, **ROW_TOL.get(row["id"], {}))


def b(v):
    return "true" if v else "false"


def kernel_id(demangled):
    """'void qsi::k_si_pack<float, double, 9, false>(double const*, ...)' -> 'k_si_pack<float, double, 9, false>'"""
    s = re.sub(r"^void\s+", "", demangled).split("(", 1)[0]
    return re.sub(r"\b\w+::", "", s)


def _n(record):
    return RECORDS[record][0]


def _c(record):
    return RECORDS[record][1]


# ---- kernel ids, as the ladders instantiate them
def k_dv_pack(T, S):
    return ("devio", f"k_dv_pack<{T_NAMES[T]}, {T_NAMES[S]}>")


def k_dv_state(T, D, record):                                   # devio_capi.hip state_t: num_states 15 / 9, compact at run time
    return ("devio", f"k_dv_state<{T_NAMES[T]}, {T_NAMES[D]}, {_n(record)}>")


def k_dv_report(T, D):
    return ("devio", f"k_dv_report<{T_NAMES[T]}, {T_NAMES[D]}>")


def k_pregate(T, direct, pfp, record, predict):                 # launch_flags: direct, pfp, compact; PREDICT by the entry
    return ("gate", f"k_pregate<{T_NAMES[T]}, {b(direct)}, {b(pfp)}, {b(_c(record))}, {b(predict)}>")


def k_nees(T, pfp, record):
    return ("consistency", f"k_nees<{T_NAMES[T]}, {b(pfp)}, {b(_c(record))}>")


def k_health(T, record):                                        # health_t: compact -> <true, 9>, else <false, n>
    return ("health", f"k_health<{T_NAMES[T]}, {b(_c(record))}, {_n(record)}>")


def k_lookahead(T, pfp, record):
    return ("lookahead", f"k_lookahead<{T_NAMES[T]}, {b(pfp)}, {b(_c(record))}>")


def k_sq_pack(T, S):
    return ("sequence", f"k_sq_pack<{T_NAMES[T]}, {T_NAMES[S]}>")


def k_score(T, direct, pfp, record):
    return ("score", f"k_score<{T_NAMES[T]}, {b(direct)}, {b(pfp)}, {b(_c(record))}>")


def k_bank_fuse(T, record):
    return ("bank", f"k_bank_fuse<{T_NAMES[T]}, {b(_c(record))}>")


def k_imm_mix(T, record):
    return ("imm", f"k_imm_mix<{T_NAMES[T]}, {b(_c(record))}>")


def k_adapt_observe(T, direct, record):                         # per-filter parameters are always in force: no pfp axis
    return ("adapt", f"k_adapt_observe<{T_NAMES[T]}, {b(direct)}, {b(_c(record))}>")


def k_si_pack(T, S, record):                                    # launch_pack: compact -> <9, true>, else <n, false>
    return ("stateio", f"k_si_pack<{T_NAMES[T]}, {T_NAMES[S]}, {_n(record)}, {b(_c(record))}>")


def k_si_copy(T, record):                                       # run_copy: quads of the record's words, of a record, of a parameter record
    w = 4 if T == "f32" else 8
    quads = lambda words: words * w // 16                       # noqa: E731
    return ("stateio", f"k_si_copy<{quads(RECORD_WORDS[_c(record)])}, {quads(144)}, {quads(24)}>")


def _row(rows, library, call, T, record, kernels, reference, direct=True, pfp=False, **extra):
    axes = [T, record] + ([f"direct{int(direct)}"] if "direct" in extra.pop("_show", ()) else []) + (["pfp"] if pfp else [])
    axes += [f"{k}{int(v) if isinstance(v, bool) else v}" for k, v in extra.items() if v is not None]
    rows.append(dict(id=f"{call}-" + "-".join(axes), library=library, call=call, dtype=T, record=record, direct=direct, pfp=pfp,
                     kernels=frozenset(kernels), reference=reference, **extra))


def build_rows():
    rows = []
    for T in DTYPES:
        # ---- devio: the pack of a tick's tensors (record-independent), state and report out (src / dst: the tensor dtype)
        for S in DTYPES:
            _row(rows, "devio", "DeviceIO.tick", T, "full15", {k_dv_pack(T, S)}, "bits of InputSequence.upload_tick", src=S)
        for D, record in itertools.product(DTYPES, RECORDS):
            _row(rows, "devio", "DeviceIO.state", T, record, {k_dv_state(T, D, record)}, "bits of get_state", dst=D)
            for F in BOOLS:
                _row(rows, "devio", "DeviceIO.report", T, record, {k_dv_report(T, D)}, "bits of report", pfp=F, dst=D)
        # ---- gate: qgt_gate_tick (PREDICT) behind the pack of DeviceIO.tick, qgt_innovation behind the pack of DeviceIO.innovation
        for record, D, F, PREDICT in itertools.product(RECORDS, BOOLS, BOOLS, BOOLS):
            _row(rows, "gate", "DeviceIO.tick(chi2_max)" if PREDICT else "DeviceIO.innovation", T, record,
                 {k_pregate(T, D, F, record, PREDICT), k_dv_pack(T, T)},
                 "gate_util.predict_then_innovation" if PREDICT else "innovation_util.innovation_ref_batch", direct=D, pfp=F, _show=("direct",),
                 predict=PREDICT)
        # ---- consistency: k_nees and, for the summary, k_nees_reduce
        for record, F in itertools.product(RECORDS, BOOLS):
            _row(rows, "consistency", "DeviceIO.nees", T, record, {k_nees(T, F, record), ("consistency", "k_nees_reduce")},
                 "consistency_util dense solve", pfp=F)
        # ---- health: k_health and k_health_reduce; k_retire; k_and_masks inside reseed
        for record in RECORDS:
            _row(rows, "health", "DeviceIO.health", T, record, {k_health(T, record), ("health", "k_health_reduce")}, "health_util.classify")
        for record in ("full15", "compact9"):
            _row(rows, "health", "DeviceIO.retire", T, record, {("health", f"k_retire<{T_NAMES[T]}>")}, "zeroed records, the others' bits")
        # ---- lookahead
        for record, F in itertools.product(RECORDS, BOOLS):
            _row(rows, "lookahead", "DeviceIO.lookahead", T, record, {k_lookahead(T, F, record)}, "oracle.run_batch with the held IMU sample", pfp=F)
        # ---- sequence: k_sq_pack, one launch per chunk of 32 ticks
        for S in DTYPES:
            _row(rows, "sequence", "DeviceIO.sequence", T, "full15", {k_sq_pack(T, S)}, "bits of per-tick devio packs", src=S)
        # ---- score: k_score behind the pack of Scorer.observe
        for record, D, F in itertools.product(RECORDS, BOOLS, BOOLS):
            _row(rows, "score", "Scorer.observe", T, record, {k_score(T, D, F, record), k_dv_pack(T, T)}, "score_util.ScoreRef", direct=D, pfp=F,
                 _show=("direct",))
        # ---- bank and imm: the ragged shape on every record kind, the bank that fills a tile once per dtype
        for (M, G), record in [(BANK_SHAPES[0], r) for r in RECORDS] + [(BANK_SHAPES[1], "full15")]:
            _row(rows, "bank", "Bank.fuse", T, record, {k_bank_fuse(T, record)}, "bank_util.fuse_ref", M=M, G=G)
            _row(rows, "imm", "Imm.mix", T, record, {k_imm_mix(T, record)}, "imm_util.mix_ref", M=M, G=G)
        # ---- adapt: k_adapt_observe behind the pack of Adapter.observe; k_adapt_apply
        for record, D in itertools.product(RECORDS, BOOLS):
            _row(rows, "adapt", "Adapter.observe", T, record, {k_adapt_observe(T, D, record), k_dv_pack(T, T)}, "adapt_util.AdaptRef", direct=D, pfp=True,
                 _show=("direct",))
        _row(rows, "adapt", "Adapter.apply", T, "full15", {("adapt", f"k_adapt_apply<{T_NAMES[T]}>")}, "adapt_util.apply_ref", pfp=True)
        # ---- stateio: k_si_pack (src: the tensors' dtype), k_si_copy (a 165-filter destination indexed into a 70-filter source)
        for S, record in itertools.product(DTYPES, RECORDS):
            _row(rows, "stateio", "DeviceIO.set_state", T, record, {k_si_pack(T, S, record)}, "stateio_util.expected_pack", src=S)
        for record, W in itertools.product(RECORDS, BOOLS):
            _row(rows, "stateio", "DeviceIO.restore", T, record, {k_si_copy(T, record)}, "stateio_util.expected_copy", pfp=W, with_params=W)
    # ---- the kernels without a dtype of their own
    _row(rows, "health", "DeviceIO.reseed", "f32", "full15", {k_health("f32", "full15"), ("health", "k_and_masks"), k_dv_pack("f32", "f32")},
         "health_util.classify AND the mask")
    _row(rows, "score", "Scorer.summary", "f64", "full15", {("score", "k_score_tiles"), ("score", "k_score_reduce")}, "numpy sum of the accumulators")
    _row(rows, "imm", "Imm.update", "f32", "full15", {("imm", "k_imm_update")}, "imm_util.update_ref", M=BANK_SHAPES[0][0], G=BANK_SHAPES[0][1])
    return rows


ROWS = build_rows()
assert len({r["id"] for r in ROWS}) == len(ROWS), "row ids must be unique"


def covered_kernels(library=None):
    """the (library, kernel id) pairs the rows name; library: that library's kernel ids"""
    pairs = set().union(*(r["kernels"] for r in ROWS))
    return pairs if library is None else {k for lib, k in pairs if lib == library}


def rows_of(library):
    return [r for r in ROWS if r["library"] == library]


# ------------------------------------------------------------------------------------------------ inputs
def held(dtype, a):
    """a as a handle (or a tensor) of `dtype` holds it, in double"""
    return None if a is None else (a.astype(np.float32).astype(np.float64) if dtype == "f32" else np.array(a, dtype=np.float64))


def params_kw(row):
    return dict(update_freq=400.0, direct_orien_method=int(row["direct"]), est_bias=int(_n(row["record"]) == 15), **HW)


class Inputs:
    """The inputs of a row, numpy only and a function of the row alone.  Every array is in double and holds values the row's dtype
    represents.  x, P: the state (one record all zero); u, z, mask; pfp (None without per-filter parameters); on: the filters the call
    works on (mask and a state); the bank and IMM rows: logw, Pi, and x, P, mask of bank_util.make_case."""
    ZERO = 70        # the all-zero record: a lane of the second tile
    BIG = 129        # ~170 degrees between tag pose and attitude: a lane of the ragged tile

    def __init__(self, row):
        T, n = row["dtype"], _n(row["record"])
        self.kw = params_kw(row)
        self.po = oracle.make_params(**self.kw)
        self.p = ekf_np.Params.from_orc(self.po)
        rng = self.rng = np.random.default_rng(zlib.crc32(row["id"].encode()))
        self.M, self.G = row.get("M"), row.get("G")
        self.B = B if self.M is None else self.M * self.G
        nB = self.B
        self.pfp = None
        if row["pfp"]:                                           # as test_gpu_variants.Inputs draws them
            pfp = np.zeros((nB, 24))
            pfp[:, 0:12] = np.array(list(self.po.Q)) * 10 ** rng.uniform(-0.5, 0.5, size=(nB, 12))
            pfp[:, 12:15] = np.array(HW["ab_static"]) + rng.normal(size=(nB, 3)) * 0.1
            pfp[:, 15:18] = np.array(HW["wb_static"]) + rng.normal(size=(nB, 3)) * 0.01
            pfp[:, 18:24] = np.array(list(self.po.R)) * rng.uniform(0.5, 2.0, size=(nB, 6))
            if n == 9:
                pfp[:, 6:12] = 0.0
            self.pfp = held(T, pfp)
        if self.M is not None:
            self.x, self.P, self.logw, self.mask, self.Pi = iu.make_case(rng, self.M, self.G, n, T)
            self.on = (self.mask != 0) & self.x[:, 6:10].any(axis=1)
            return
        if row["library"] == "consistency":                      # P = D C D with kappa(C) <= 100 and a truth drawn from it (attitude errors to 170 degrees)
            ab = np.broadcast_to(held(T, np.array(HW["ab_static"])), (nB, 3)) if self.pfp is None else self.pfp[:, 12:15]
            wb = np.broadcast_to(held(T, np.array(HW["wb_static"])), (nB, 3)) if self.pfp is None else self.pfp[:, 15:18]
            self.ab, self.wb = ab, wb
            x, P, self.xt = cu.make_case(rng, nB, n, T, ab, wb)
        else:
            x, P = rand_states(rng, nB, n, cov_scale=0.3)
            if n == 9:
                x[:, 10:16] = 0.0
        if row["call"] in ("DeviceIO.health", "DeviceIO.reseed"):   # the eight cases of health_util in three tiles, and variances around the limits
            P[4::5] *= 40.0
            xc, Pc = hu.case_list(T, n)
            self.cases = np.array([3, 17, 40, 63, 64, 100, 128, 164])
            x[self.cases], P[self.cases] = xc, Pc
        x[self.ZERO], P[self.ZERO] = 0.0, 0.0
        self.x, self.P = held(T, x), held(T, P)
        self.P = 0.5 * (self.P + self.P.transpose(0, 2, 1))
        self.u = held(T, rand_imu(rng, nB))
        finite = np.where(np.isfinite(self.x), self.x, 0.0)
        finite[~finite[:, 6:10].any(axis=1), 9] = 1.0
        z = meas_near(rng, self.po, finite, ang=0.3, pos=0.05)
        z[self.BIG:self.BIG + 1] = meas_near(rng, self.po, finite[self.BIG:self.BIG + 1], ang=0.0, pos=0.05)
        ax = np.array([0.6, -0.48, 0.64])                        # a unit axis: the tag pose turned by 170 degrees about it
        dq = np.concatenate([ax * np.sin(np.deg2rad(85.0)), [np.cos(np.deg2rad(85.0))]])
        z[self.BIG, 3:7] = ekf_np.qmul(z[self.BIG, 3:7], dq)
        far = rng.uniform(size=nB) < 0.3                         # displaced tag poses: the gate rejects them
        z[far, 0:2] += 1.5 * rng.normal(size=(int(far.sum()), 2))
        self.z = held(T, z)
        m = rng.uniform(size=nB) < 0.6
        m[0:64] = True                                           # one whole tile on, mixed bits elsewhere
        m[self.BIG] = True
        if row["call"] in ("DeviceIO.health", "DeviceIO.reseed"):
            m[self.cases] = True
        self.mask = m.astype(np.uint8)
        self.on = m & self.x[:, 6:10].any(axis=1)

    def ref_state(self):
        """(x, P) for a reference that steps every filter: the filters that are not on borrow filter 0's state (their results are not read)"""
        x, P = self.x.copy(), self.P.copy()
        x[~self.on], P[~self.on] = self.x[0], self.P[0]
        return x, P

    def innovation(self, predict):
        """(nu, S, nis, x_pred) of the filters that are on (NaN / 0 elsewhere): the reference of the gate, score and adapt rows"""
        x, P = self.ref_state()
        nu, S, nis, xp, _ = predict_then_innovation(self.po, self.p, x, P, self.u, self.z, self.pfp, mask=self.on, predict=predict)
        return nu, S, nis, xp


def pd(A):
    """[B] bool: finite and positive definite"""
    ok = np.isfinite(A).all(axis=(1, 2))
    out = np.zeros(len(A), bool)
    out[ok] = np.linalg.eigvalsh(A[ok]).min(axis=1) > 0
    return out


def conditions(row):
    """Asserts, on the reference alone, that the row cannot hide a failure (the module docstring); -> the Inputs."""
    d = Inputs(row)
    lib = row["library"]
    if row["call"] in ("DeviceIO.health", "DeviceIO.reseed"):    # a health row is there to see what is not finite and not definite
        on = d.mask != 0
        st, margin = hu.classify(d.x, d.P, mask=on, **hu.LIMITS)
        assert margin >= 1e-3, (row["id"], margin)               # |lambda_min| of every factored P: four orders above fp32 rounding of its entries (<= 4)
        assert all((st & bit).any() for bit in (hu.NONFINITE, hu.NOT_PD, hu.QNORM, hu.SIGMA_R)) and (st == 0)[on].any(), row["id"]
        fact = on & d.x[:, 6:10].any(axis=1) & (st & hu.NONFINITE == 0)
        dg = np.einsum("bii->bi", d.P)[fact]
        near = np.abs(dg[:, 0:3].max(axis=1) / hu.LIMIT ** 2 - 1) < 1e-3
        assert near.sum() <= 2, (row["id"], int(near.sum()))     # the two at_limit / above_limit cases of health_util, which are exact
        assert on.sum() * 2 >= d.B
        return d
    live = d.on
    assert live.sum() * 2 >= d.B, (row["id"], int(live.sum()))
    assert np.isfinite(d.x[live]).all() and pd(d.P[live]).all(), row["id"]
    if lib in ("gate", "score", "adapt"):
        nu, S, nis, _ = d.innovation(row.get("predict", True))
        assert np.isfinite(nu[live]).all() and pd(S[live]).all() and np.isfinite(nis[live]).all() and (nis[live] > 0).all(), row["id"]
        if lib == "gate" and row["predict"]:
            acc = nis[live] <= CHI2
            near = np.abs(nis[live] / CHI2 - 1) <= 1e-3
            assert acc.any() and not acc.all(), (row["id"], "the gate must accept some and reject some")
            assert near.sum() <= 0.02 * live.sum(), (row["id"], int(near.sum()))
            assert nis[d.BIG] > CHI2
    return d
