"""ctypes binding of include/qle_budget.h (libqle_budget.so): the per-component error budget of a batch against a truth, on the device.

Per group of filters (whole 64-filter tiles) the count, sum e, sum e e^T and sum P in fp64 -- 256 doubles, whatever the batch -- with e
the error of the consistency diagnostics (truth minus estimate in the filter's error-state convention) and P the stored covariance:
the ensemble bias of every state, the sample covariance of the error and the covariance the filters report beside it (k_budget,
k_budget_reduce: csrc/ekf_budget.hpp).  Both kernels only read the handle; the sums are deterministic to the bit and additive over
shards.  `DeviceRecords.budget` (records.py) is the caller for device tensors, on a handle's records and on every view of them;
`DeviceIO.budget_run` (devio.py) gives the budget at every e-th tick of a sequence; `BatchedRelativePoseEKF.error_budget` /
`synth_budget` (ekf.py) serve host arrays.  There is no fallback: a missing library is an error.

The library is outside the closed census of the eleven side libraries (csrc/Makefile, SIDE_OPEN; `_lib.OPEN_LIBRARIES`): its kernels
are the rows of tests/budget_variant_table.py, and `BUDGET.launch_census()` is its census.
"""
import ctypes as C

from ._lib import QleDeviceView, QleParams, SideLibrary

QBG_F32, QBG_F64 = 0, 1
WORDS = 256
N_ERR = 15
ERR0, OUTER0, COV0 = 1, 16, 136   # first word of sum e, of sum e e^T, of sum P
STATES = ("r_x", "r_y", "r_z", "v_x", "v_y", "v_z", "th_x", "th_y", "th_z", "ab_x", "ab_y", "ab_z", "wb_x", "wb_y", "wb_z")
STATUS_OFF, STATUS_COUNTED, STATUS_NONFINITE = 0, 1, 2


def tri(i, j):
    """word of (i, j), i <= j, in the row-major upper triangle of a 15 x 15 matrix"""
    return 15 * i - i * (i - 1) // 2 + (j - i)


_vp = C.c_void_p
_pview, _ppar = C.POINTER(QleDeviceView), C.POINTER(QleParams)
_pd, _pu8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
# every symbol include/qle_budget.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "qbg_last_error": (C.c_char_p, []),
    "qbg_launch_count": (C.c_int64, []),
    "qbg_launch_census_begin": (C.c_int, []),
    "qbg_launch_census_end": (C.c_int, [C.c_char_p, C.c_int64, C.POINTER(C.c_int64)]),
    "qbg_groups": (C.c_int64, [C.c_int64, C.c_int64]),
    "qbg_budget": (C.c_int, [_pview, _ppar, _vp, C.c_int32, C.c_int64, _vp, C.c_int64, _vp, _vp, C.c_int32, _vp]),
    "qbg_budget_host": (C.c_int, [_pview, _ppar, _pd, C.c_int64, _pu8, C.c_int64, _pd, _pd, _pu8]),
}

BUDGET = SideLibrary("budget", "QLE_BUDGET_LIB", SYMBOLS, "the error budget", "qbg_last_error", needs_tick_library=True, closed_census=False)
BUDGET_LIB_PATH, budget_lib, bcheck = BUDGET.path, BUDGET.load, BUDGET.check


def groups(batch, group_tiles):
    """(group_tiles as the library takes it, the number of groups): None / 0 = one group; refuses a negative or non-integer value.
    The arithmetic of qbg_groups, on the host: no library call."""
    gt = 0 if group_tiles is None else group_tiles
    if isinstance(gt, bool) or int(gt) != gt or gt < 0:
        raise ValueError(f"group_tiles must be a whole number of 64-filter tiles >= 0 (got {group_tiles!r})")
    gt = int(gt)
    tiles = -(-int(batch) // 64)
    return gt, (1 if gt == 0 else -(-tiles // gt))


_SYM = [[OUTER0 + tri(min(i, j), max(i, j)) for j in range(N_ERR)] for i in range(N_ERR)]
_DIAG = [tri(k, k) for k in range(N_ERR)]


class Budget:
    """The sums of one or more budgets, `sums` [..., G, 256] in float64 (a device tensor, or a numpy array from the host entries), and
    what an error budget reads off them, derived where the sums live with plain array operations -- a few hundred words, no kernel:
    n [..., G]; mean [..., G, 15] = sum e / n (the bias of every state); mse [..., G, 15, 15] = sum e e^T / n;
    cov = mse - mean mean^T (the sample covariance of the error); P_mean = sum P / n (the covariance the filters report);
    var_ratio [..., G, 15] = diag sum e e^T / diag sum P (above 1: the state is over-confident); rms = sqrt(diag mse) and
    sigma = sqrt(diag P_mean), the two curves of an "RMS error against sigma" plot.  A group with n = 0 gives NaN, not an exception.
    States in the order of `STATES`.  err [B, n] and status [B] are there when the call asked for them."""

    def __init__(self, sums, err=None, status=None):
        if tuple(sums.shape[-1:]) != (WORDS,):
            raise ValueError(f"sums: expected [..., G, {WORDS}], got {tuple(sums.shape)}")
        self.sums, self.err, self.status = sums, err, status

    @staticmethod
    def combine(budgets):
        """The budget of the union of shards or ranks: their sums added, in the order given."""
        budgets = list(budgets)
        if not budgets:
            raise ValueError("combine: no budgets")
        tot = budgets[0].sums
        for b in budgets[1:]:
            tot = tot + b.sums
        return Budget(tot)

    def _div(self, a, b):
        if type(a).__module__ == "numpy":
            import numpy as np
            with np.errstate(divide="ignore", invalid="ignore"):
                return a / b
        return a / b

    @property
    def n(self):
        return self.sums[..., 0]

    @property
    def sum_outer(self):
        """sum e e^T as full symmetric matrices [..., G, 15, 15]"""
        return self.sums[..., _SYM]

    @property
    def sum_P(self):
        return self.sums[..., [[w - OUTER0 + COV0 for w in row] for row in _SYM]]

    @property
    def mean(self):
        return self._div(self.sums[..., ERR0:ERR0 + N_ERR], self.sums[..., 0:1])

    @property
    def mse(self):
        return self._div(self.sum_outer, self.sums[..., 0:1, None])

    @property
    def cov(self):
        m = self.mean
        return self.mse - m[..., :, None] * m[..., None, :]

    @property
    def P_mean(self):
        return self._div(self.sum_P, self.sums[..., 0:1, None])

    @property
    def var_ratio(self):
        return self._div(self.sums[..., [OUTER0 + d for d in _DIAG]], self.sums[..., [COV0 + d for d in _DIAG]])

    @property
    def rms(self):
        return self._div(self.sums[..., [OUTER0 + d for d in _DIAG]], self.sums[..., 0:1]) ** 0.5

    @property
    def sigma(self):
        return self._div(self.sums[..., [COV0 + d for d in _DIAG]], self.sums[..., 0:1]) ** 0.5
