"""ctypes binding of include/qle_consistency.h (libqle_consistency.so): filter consistency against a truth, evaluated on the device.

Per filter NEES = e^T P^-1 e over all states or over the marginal of a selection of the blocks r, v, theta, ab, wb, with e = truth minus
estimate in the filter's error-state convention, and a deterministic batch summary (k_nees, k_nees_reduce: csrc/ekf_consistency.hpp).
Both kernels only read the handle.  `DeviceIO.nees` (devio.py) is the caller for device tensors, `BatchedRelativePoseEKF.nees` /
`synth_nees` (ekf.py) for host arrays.  There is no fallback: a missing library is an error.
"""
import ctypes as C

from ._lib import QleDeviceView, QleParams, SideLibrary

QCS_F32, QCS_F64 = 0, 1
BLOCKS = {"r": 1, "v": 2, "theta": 4, "ab": 8, "wb": 16}
_ALIASES = {"th": 4, "\u03b8": 4, "pose": 1 | 4, "bias": 8 | 16, "all": 31}
SUMMARY_FIELDS = ("count", "sum_nees", "sum_nees_sq", "n_above", "n_not_pd", "sum_r_err_sq", "sum_theta_err_sq", "dof")


class QcsSummary(C.Structure):
    """`struct qcs_summary`: eight doubles."""
    _fields_ = [(n, C.c_double) for n in SUMMARY_FIELDS]


_vp = C.c_void_p
_pview, _ppar = C.POINTER(QleDeviceView), C.POINTER(QleParams)
_pd, _pu8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
# every symbol include/qle_consistency.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "qcs_last_error": (C.c_char_p, []),
    "qcs_launch_count": (C.c_int64, []),
    "qcs_launch_census_begin": (C.c_int, []),
    "qcs_launch_census_end": (C.c_int, [C.c_char_p, C.c_int64, C.POINTER(C.c_int64)]),
    "qcs_nees": (C.c_int, [_pview, _ppar, _vp, C.c_int32, _vp, C.c_uint32, C.c_double, _vp, _vp, _vp, C.c_int32]),
    "qcs_nees_host": (C.c_int, [_pview, _ppar, _pd, _pu8, C.c_uint32, C.c_double, _pd, _pd, C.POINTER(QcsSummary)]),
}

CONSISTENCY = SideLibrary("consistency", "QLE_CONSISTENCY_LIB", SYMBOLS, "the consistency diagnostics", "qcs_last_error", needs_tick_library=True)
CONSISTENCY_LIB_PATH, consistency_lib, ccheck = CONSISTENCY.path, CONSISTENCY.load, CONSISTENCY.check


def block_mask(blocks, num_states=15):
    """The bit mask of a block selection: an int, "all" (every block the handle has), or names joined by + , or blanks out of
    r, v, theta (th), ab, wb, pose (= r + theta), bias (= ab + wb).  Refuses an empty selection, an unknown name, bits above 4 and
    bias blocks with num_states = 9."""
    have = 31 if num_states == 15 else 7
    if isinstance(blocks, str):
        if blocks.strip() == "all":
            return have
        m = 0
        for name in blocks.replace("+", " ").replace(",", " ").split():
            if name not in BLOCKS and name not in _ALIASES:
                raise ValueError(f"blocks: unknown block {name!r}, expected names out of {sorted(BLOCKS) + sorted(_ALIASES)}")
            m |= BLOCKS.get(name) or _ALIASES[name]
    elif isinstance(blocks, (list, tuple, set, frozenset)):
        m = 0
        for b in blocks:
            m |= block_mask(b, 15)
    else:
        m = int(blocks)
    if m <= 0 or m & ~31:
        raise ValueError(f"blocks: {blocks!r} selects nothing or bits above 4 (r, v, theta, ab, wb)")
    if m & ~have:
        raise ValueError(f"blocks: {blocks!r} selects a bias block, the handle has {num_states} states (est_bias = false)")
    return m


def check_chi2_hi(chi2_hi):
    chi2_hi = float(chi2_hi)
    if not chi2_hi > 0.0:
        raise ValueError(f"chi2_hi must be > 0 (got {chi2_hi})")
    return chi2_hi
