"""ctypes binding of include/qle_health.h (libqle_health.so): filter lifecycle from GPU memory.

`qhl_health` classifies every filter in one read-only launch (k_health: csrc/ekf_health.hpp) -- non-finite words, a covariance that is
not positive definite, a quaternion off the unit sphere, a standard deviation above a limit -- into a status byte per filter, a
`flagged` mask and a nine-count batch summary; `qhl_retire` turns flagged filters into "uninitialised" ones every tick skips;
`qhl_and_masks` forms flagged AND detections, the mask of a reseed.  `DeviceIO.seed / health / retire / reseed` (devio.py) are the
callers for device tensors, `BatchedRelativePoseEKF.health` (ekf.py) for host arrays.  There is no fallback: a missing library is an
error.
"""
import ctypes as C

from ._lib import QleDeviceView, SideLibrary

NONFINITE, NOT_PD, QNORM, SIGMA_R, SIGMA_V, SIGMA_THETA = 1, 2, 4, 8, 16, 32
ALL = 63
BITS = {"nonfinite": NONFINITE, "not_pd": NOT_PD, "qnorm": QNORM, "sigma_r": SIGMA_R, "sigma_v": SIGMA_V, "sigma_theta": SIGMA_THETA}
SUMMARY_FIELDS = ("evaluated", "flagged", "uninitialised", "n_nonfinite", "n_not_pd", "n_qnorm", "n_sigma_r", "n_sigma_v", "n_sigma_theta")


class QhlLimits(C.Structure):
    """`struct qhl_limits`."""
    _fields_ = [("struct_size", C.c_uint32), ("select", C.c_uint32), ("sigma_r_max", C.c_double), ("sigma_v_max", C.c_double),
                ("sigma_theta_max", C.c_double), ("qnorm_tol", C.c_double)]


class QhlSummary(C.Structure):
    """`struct qhl_summary`: nine doubles."""
    _fields_ = [(n, C.c_double) for n in SUMMARY_FIELDS]


_vp = C.c_void_p
_pview, _plim = C.POINTER(QleDeviceView), C.POINTER(QhlLimits)
_pu8 = C.POINTER(C.c_uint8)
# every symbol include/qle_health.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "qhl_last_error": (C.c_char_p, []),
    "qhl_launch_count": (C.c_int64, []),
    "qhl_launch_census_begin": (C.c_int, []),
    "qhl_launch_census_end": (C.c_int, [C.c_char_p, C.c_int64, C.POINTER(C.c_int64)]),
    "qhl_health": (C.c_int, [_pview, _plim, _vp, _vp, _vp, _vp]),
    "qhl_health_host": (C.c_int, [_pview, _plim, _pu8, _pu8, _pu8, C.POINTER(QhlSummary)]),
    "qhl_retire": (C.c_int, [_pview, _vp]),
    "qhl_and_masks": (C.c_int, [_pview, _vp, _vp, _vp]),
}

HEALTH = SideLibrary("health", "QLE_HEALTH_LIB", SYMBOLS, "the lifecycle kernels", "qhl_last_error")
HEALTH_LIB_PATH, health_lib, hcheck = HEALTH.path, HEALTH.load, HEALTH.check


def select_mask(select):
    """The bit mask of a selection of status bits: None (all), an int, or names joined by + , or blanks out of BITS.  Refuses an
    empty selection, an unknown name and bits above ALL."""
    if select is None:
        return ALL
    if isinstance(select, str):
        m = 0
        for name in select.replace("+", " ").replace(",", " ").split():
            if name == "all":
                m |= ALL
            elif name in BITS:
                m |= BITS[name]
            else:
                raise ValueError(f"select: unknown status bit {name!r}, expected names out of {sorted(BITS)}")
    elif isinstance(select, (list, tuple, set, frozenset)):
        m = 0
        for s in select:
            m |= select_mask(s)
    else:
        m = int(select)
    if m <= 0 or m & ~ALL:
        raise ValueError(f"select: {select!r} selects nothing or bits above {ALL}")
    return m


def make_limits(sigma_r_max=float("inf"), sigma_v_max=float("inf"), sigma_theta_max=float("inf"), qnorm_tol=1e-3, select=None):
    """A checked `QhlLimits`: every limit > 0 (inf = no limit; NaN refused), select as `select_mask` reads it."""
    lim = QhlLimits()
    lim.struct_size = C.sizeof(QhlLimits)
    lim.select = select_mask(select)
    for name, v in (("sigma_r_max", sigma_r_max), ("sigma_v_max", sigma_v_max), ("sigma_theta_max", sigma_theta_max), ("qnorm_tol", qnorm_tol)):
        v = float(v)
        if not v > 0.0:
            raise ValueError(f"{name} must be > 0 (got {v})")
        setattr(lim, name, v)
    return lim
