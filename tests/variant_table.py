"""Every tick-kernel instantiation of libqle_ekf.so as a test case (tests/test_variant_table_cpu.py checks the table against the built
library, tests/test_gpu_variants.py runs every row on the device).

The rows are generated from the axis lists below, which restate the launchers' with_bool / with_int lists (ekf_host.hpp, tu_*.hip).  A
launcher that gains a value, or a kernel that gains an axis, has no row until the list here says so, and the CPU test names the kernel.

Axes come in two kinds:
  semantic -- T, D (direct orientation method), F (per-filter parameters), G (device gating), COMPACT (record layout), M (multirate
      history), STEP and the kernel family: they change what is computed.  Rows with one semantic key run the same inputs.
  policy -- N (cache policy), L (loads first), W (filters per cooperative workgroup), the refresh tick, the split and the workgroup
      size: they must not change results.  The row of a semantic key with every policy axis at its canonical value is checked against
      the fp64 oracle; every other row of the key must equal it bit for bit.

Each row: id, entry (the call whose launches the census covers), dtype, params (engine parameter overrides), pfp (per-filter
parameters), gating, env (QLE_* overrides read at handle creation), B, kernels (the exact set of kernels that call launches, as
demangled template ids), key (the semantic key), canonical (True for the oracle-checked row of its key) and own_oracle.

own_oracle: a policy value that is not bit-invariant, so its rows are checked against the oracle and bit for bit against each other
only.  kw_tick with tag poses, W = 64 against W = 16: a whole-tile workgroup's two helper waves (innovation, gain inputs) load the
filter's record and predict its nominal state themselves; a quarter-tile workgroup's read the prediction of the main scalar wave from
the LDS.  The two predictions are the same expressions compiled into different code, and their last bits differ (fp32 state words
~1 ulp; the predict-only tick, which has no helper roles, is bit-identical across W).
"""
import itertools
import re

T_NAMES = {"f32": "float", "f64": "double"}
BOOLS = (False, True)
N_VALUES = (0, 1, 2, 3)            # predict_lanes / step_lanes: with_int<0, 1, 2, 3>(effective_nt)
KW_N_VALUES = (0, 1, 2)            # launch_quad: with_int<0, 1, 2>(nt), QLE_NT=3 runs as 0
KW_W_VALUES = (16, 64)             # launch_quad: with_int<16, 64>(fpw)
BLOCKS_LDS = (64, 128, 256)        # fp64 kernels with the split covariance (split_lds): one to four LDS windows per workgroup

# batch sizes: ragged (not a multiple of 64), a grid of at least 8 workgroups that is not a multiple of 8 at 64 / 128 / 256 threads
# (38 / 19 / 10 workgroups), so that batch_block() remaps the grid over the XCDs; more than 4 096 filters for whole-tile kw_tick workgroups
B_LANES = 2391
B_KW = {16: 2327, 64: 4439}    # kw_tick: 148 quarter-tile or 70 whole-tile workgroups
B_MAX = max(B_LANES, *B_KW.values())

# Helper kernels (staging, seeding, reports, the synthetic generator) are launched by the entry points of every row and checked by
# tests/test_gpu_variants.py::test_helper_kernels_census; none is left out of the census.
HELPER_FAMILIES = ("k_pack_off", "k_unpack_off", "k_pack_z_off", "k_unpack_z_off", "k_pack_P_off", "k_unpack_P_off", "k_relayout_P", "k_seed",
                   "k_report_off", "k_count_nonfinite", "k_upds_since", "k_synth", "k_rmse", "k_fill_i32", "k_rebase_ticks")
EXCLUDED = {}   # kernel id -> one-line reason it has no row (kept empty)


def b(v):
    return "true" if v else "false"


def k_predict(T, F, N, M, C, L):
    return f"k_predict<{T_NAMES[T]}, {b(F)}, {N}, {b(M)}, {b(C)}, {b(L)}>"


def k_step(T, D, F, G, N, C):
    return f"k_step<{T_NAMES[T]}, {b(D)}, {b(F)}, {b(G)}, {N}, {b(C)}>"


def k_update(T, D, F, C):
    return f"k_update<{T_NAMES[T]}, {b(D)}, {b(F)}, {b(C)}>"


def k_step_mr(T, D, F):
    return f"k_step_mr<{T_NAMES[T]}, {b(D)}, {b(F)}>"


def k_run_resident(T, D, F, C):
    return f"k_run_resident<{T_NAMES[T]}, {b(D)}, {b(F)}, {b(C)}>"


def k_innov(T, D, F, C, G):
    return f"k_innov<{T_NAMES[T]}, {b(D)}, {b(F)}, {b(C)}, {b(G)}>"


def kw_tick(T, D, F, G, STEP, N, W):
    return f"kw_tick<{T_NAMES[T]}, {b(D)}, {b(F)}, {b(G)}, {b(STEP)}, {N}, {W}>"


def kernel_id(demangled):
    """'void qle::k_step<float, true, ...>(float*, ...)' -> 'k_step<float, true, ...>'."""
    s = re.sub(r"^void\s+", "", demangled)
    s = s.split("(", 1)[0]
    return s.replace("qle::", "")


def loads_first_values(T, C):
    return BOOLS if T == "f32" and not C else (False,)   # with_bool_if<sizeof(T) == 4 && !COMPACT>


def nt_env(N):
    """QLE_* overrides that make effective_nt() return N on every tick."""
    return {"QLE_NT": str(N), "QLE_REFRESH": "0"}


def _row(rows, entry, T, key, canonical, kernels, env, B=B_LANES, params=None, pfp=False, gating=False, tag="", own_oracle=False):
    pol = ",".join(f"{k[4:]}={v}" for k, v in sorted(env.items()) if k not in ("QLE_QUAD", "QLE_COMPACT"))
    rows.append(dict(id=f"{entry}-{T}-" + "-".join(f"{k}{int(v) if isinstance(v, bool) else v}" for k, v in key[2:]) + (f"[{pol}]" if pol else "") + tag,
                     entry=entry, dtype=T, key=key, canonical=canonical, kernels=frozenset(kernels), env=dict(env), B=B,
                     params=dict(params or {}), pfp=pfp, gating=gating, own_oracle=own_oracle))


def build_rows():
    rows = []
    for T in ("f32", "f64"):
        lds_blocks = BLOCKS_LDS if T == "f64" else (64,)
        # ---- k_predict, M = 0: qle_predict on the one-lane kernels
        for F, C in itertools.product(BOOLS, BOOLS):
            key = ("predict", T, ("F", F), ("C", C))
            base = {"QLE_QUAD": "0", "QLE_COMPACT": "1" if C else "0"}
            for N, L in itertools.product(N_VALUES, loads_first_values(T, C)):
                env = dict(base, **nt_env(N))
                if T == "f32" and not C:
                    env["QLE_LOADS_FIRST"] = "1" if L else "0"
                _row(rows, "predict", T, key, N == 1 and (L or T == "f64" or C), {k_predict(T, F, N, False, C, L)}, env,
                     params=dict(est_bias=0 if C else 1), pfp=F)
        # ---- k_step, one fused tick: qle_step (G = 0) or qle_filter_update with device gating (G = 1)
        for D, F, G, C in itertools.product(BOOLS, BOOLS, BOOLS, BOOLS):
            key = ("step", T, ("D", D), ("F", F), ("G", G), ("C", C))
            for N in N_VALUES:
                env = dict({"QLE_QUAD": "0", "QLE_COMPACT": "1" if C else "0"}, **nt_env(N))
                _row(rows, "step", T, key, N == 1, {k_step(T, D, F, G, N, C)}, env,
                     params=dict(direct_orien_method=int(D), est_bias=0 if C else 1), pfp=F, gating=G)
            if T == "f64" and not G and not C:
                # the split policy with a given share of cached workgroup groups
                env = dict({"QLE_QUAD": "0", "QLE_COMPACT": "0", "QLE_SPLIT": "-20"}, **nt_env(3))
                _row(rows, "step", T, key, False, {k_step(T, D, F, G, 3, C)}, env,
                     params=dict(direct_orien_method=int(D), est_bias=1), pfp=F, gating=G)
        # ---- k_update: qle_update
        for D, F, C in itertools.product(BOOLS, BOOLS, BOOLS):
            key = ("update", T, ("D", D), ("F", F), ("C", C))
            for blk in lds_blocks:
                env = {"QLE_QUAD": "0", "QLE_COMPACT": "1" if C else "0", "QLE_BLOCK": str(blk)}
                _row(rows, "update", T, key, blk == 64, {k_update(T, D, F, C)}, env,
                     params=dict(direct_orien_method=int(D), est_bias=0 if C else 1), pfp=F)
        # ---- k_run_resident: qle_run_resident
        for D, F, C in itertools.product(BOOLS, BOOLS, BOOLS):
            key = ("run_resident", T, ("D", D), ("F", F), ("C", C))
            for blk in lds_blocks:
                env = {"QLE_QUAD": "0", "QLE_COMPACT": "1" if C else "0", "QLE_BLOCK": str(blk)}
                _row(rows, "run_resident", T, key, blk == 64, {k_run_resident(T, D, F, C)}, env,
                     params=dict(direct_orien_method=int(D), est_bias=0 if C else 1), pfp=F)
        # ---- multirate: qle_filter_update_stamped over a window whose predict-only ticks run k_predict<M = 1> and whose ticks with tag
        # poses run k_step_mr (full records only)
        for D, F in itertools.product(BOOLS, BOOLS):
            key = ("step_mr", T, ("D", D), ("F", F))
            params = dict(direct_orien_method=int(D), est_bias=1, multirate_ekf=1)
            for L in loads_first_values(T, False):
                lf = {"QLE_LOADS_FIRST": "1" if L else "0"} if T == "f32" else {}
                # default policy of a small state: the refresh tick (N = 1) on tick 0, then N = 2
                env = dict({"QLE_QUAD": "0"}, **lf)
                _row(rows, "step_mr", T, key, L or T == "f64",
                     {k_predict(T, F, 1, True, False, L), k_predict(T, F, 2, True, False, L), k_step_mr(T, D, F)}, env,
                     params=params, pfp=F, gating=True)
                for N in (0, 3):
                    env = dict({"QLE_QUAD": "0"}, **lf, **nt_env(N))
                    _row(rows, "step_mr", T, key, False, {k_predict(T, F, N, True, False, L), k_step_mr(T, D, F)}, env,
                         params=params, pfp=F, gating=True)
            for blk in lds_blocks[1:]:
                env = {"QLE_QUAD": "0", "QLE_BLOCK": str(blk)}
                _row(rows, "step_mr", T, key, False, {k_predict(T, F, 1, True, False, False), k_predict(T, F, 2, True, False, False),
                                                      k_step_mr(T, D, F)}, env, params=params, pfp=F, gating=True)
        # ---- k_innov: qle_innovation (G = 0) and qle_update_gated (G = 1: the gate, then k_update on the accepted records)
        for D, F, C, G in itertools.product(BOOLS, BOOLS, BOOLS, BOOLS):
            key = ("innovation" if not G else "update_gated", T, ("D", D), ("F", F), ("C", C))
            env = {"QLE_QUAD": "0", "QLE_COMPACT": "1" if C else "0"}
            ks = {k_innov(T, D, F, C, G)} | ({k_update(T, D, F, C)} if G else set())
            _row(rows, key[0], T, key, True, ks, env, params=dict(direct_orien_method=int(D), est_bias=0 if C else 1), pfp=F)
        # ---- kw_tick: the workgroup-cooperative tick (full records), predict-only (qle_predict) and with tag poses (qle_step /
        # qle_filter_update); W = 16 up to 4 096 filters, else 64
        for F in BOOLS:
            key = ("kw_predict", T, ("F", F))
            for N, W in itertools.product(KW_N_VALUES, KW_W_VALUES):
                env = dict({"QLE_QUAD": "2", "QLE_COMPACT": "0"}, **nt_env(N))
                _row(rows, "kw_predict", T, key, N == 1 and W == 16, {kw_tick(T, False, F, False, False, N, W)}, env, B=B_KW[W],
                     params=dict(est_bias=1), pfp=F, tag=f"-W{W}")
        for D, F, G in itertools.product(BOOLS, BOOLS, BOOLS):
            key = ("kw_step", T, ("D", D), ("F", F), ("G", G))
            for N, W in itertools.product(KW_N_VALUES, KW_W_VALUES):
                env = dict({"QLE_QUAD": "1", "QLE_COMPACT": "0"}, **nt_env(N))
                _row(rows, "kw_step", T, key, N == 1 and W == 16, {kw_tick(T, D, F, G, True, N, W)}, env, B=B_KW[W],
                     params=dict(direct_orien_method=int(D), est_bias=1), pfp=F, gating=G, tag=f"-W{W}", own_oracle=W == 64)
    return rows


ROWS = build_rows()


assert len({r["id"] for r in ROWS}) == len(ROWS), "row ids must be unique"


def groups():
    """semantic key -> its rows, the canonical row first"""
    out = {}
    for r in ROWS:
        out.setdefault(r["key"], []).append(r)
    for k, rs in out.items():
        rs.sort(key=lambda r: not r["canonical"])
        assert sum(r["canonical"] for r in rs) == 1, k
    return out


def covered_kernels():
    return set().union(*(r["kernels"] for r in ROWS))
