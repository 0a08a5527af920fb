"""ctypes binding of include/qle_lookahead.h (libqle_lookahead.so): state and covariance h ticks ahead, read-only.

`qlk_lookahead` loads every filter's record once, applies the predict h times in registers with the IMU sample held (k_lookahead:
csrc/ekf_lookahead.hpp) and stores the forecast records into a workspace of the caller's; the forecast is a `qle_device_view` of its
own, so every read-only consumer of a view works on it unchanged.  `Forecast` owns that workspace (a torch tensor) and the view and
offers the consumers: `state`, `report`, `health`, `nees` and `lookahead` again (forecasts chain).  `DeviceIO.lookahead` (devio.py) is
the caller for device tensors, `BatchedRelativePoseEKF.lookahead` (ekf.py) for host arrays.  There is no fallback: a missing library
is an error.
"""
import ctypes as C

from . import _tensors as _t
from ._lib import QleDeviceView, QleParams, SideLibrary
from .records import ViewRecords

QLK_F32, QLK_F64 = 0, 1
MAX_HORIZON = 4096


class QlkCoast(C.Structure):
    """`struct qlk_coast`."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("sigma_r_max", C.c_double), ("sigma_theta_max", C.c_double)]


_vp = C.c_void_p
_pview, _pparams, _pcoast = C.POINTER(QleDeviceView), C.POINTER(QleParams), C.POINTER(QlkCoast)
# every symbol include/qle_lookahead.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "qlk_last_error": (C.c_char_p, []),
    "qlk_launch_count": (C.c_int64, []),
    "qlk_launch_census_begin": (C.c_int, []),
    "qlk_launch_census_end": (C.c_int, [C.c_char_p, C.c_int64, C.POINTER(C.c_int64)]),
    "qlk_workspace_bytes": (C.c_int64, [_pview]),
    "qlk_lookahead": (C.c_int, [_pview, _pparams, _vp, C.c_int32, C.c_int32, _vp, _vp, C.c_int64, _pview, _pcoast, _vp]),
    "qlk_lookahead_host": (C.c_int, [_pview, _pparams, C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_uint8), _vp, C.c_int64, _pview, _pcoast,
                                     C.POINTER(C.c_int32)]),
}

LOOKAHEAD = SideLibrary("lookahead", "QLE_LOOKAHEAD_LIB", SYMBOLS, "the look-ahead kernel", "qlk_last_error", needs_tick_library=True)
LOOKAHEAD_LIB_PATH, lookahead_lib, kcheck = LOOKAHEAD.path, LOOKAHEAD.load, LOOKAHEAD.check


def check_horizon(h):
    """h as an int in 0..MAX_HORIZON; anything else is refused here, before any GPU call."""
    if isinstance(h, bool) or int(h) != h:
        raise ValueError(f"h must be an integer (got {h!r})")
    h = int(h)
    if not 0 <= h <= MAX_HORIZON:
        raise ValueError(f"h must be in 0..{MAX_HORIZON} (got {h})")
    return h


def make_coast(sigma_r_max=float("inf"), sigma_theta_max=float("inf")):
    """A checked `QlkCoast`, or None when both limits are infinite (no coast budget is asked for): every limit > 0, NaN refused."""
    vals = []
    for name, v in (("sigma_r_max", sigma_r_max), ("sigma_theta_max", sigma_theta_max)):
        v = float(v)
        if not v > 0.0:
            raise ValueError(f"{name} must be > 0 (got {v})")
        vals.append(v)
    if vals == [float("inf"), float("inf")]:
        return None
    c = QlkCoast()
    c.struct_size = C.sizeof(QlkCoast)
    c.sigma_r_max, c.sigma_theta_max = vals
    return c


class Forecast(ViewRecords):
    """The forecast of a `DeviceIO` (or of another `Forecast`) h ticks ahead: owns the workspace tensor the records live in and the
    `qle_device_view` of them.  `ticks_to_limit`: a device int32 tensor [B] (the coast budget), or None when no limit was given.
    Nothing here writes a handle; the consumers (`state`, `report`, `health`, `nees`) are the read-only bindings of `DeviceRecords`,
    run on the forecast view."""

    def __init__(self, io, view, workspace, h, ticks_to_limit):
        super().__init__(io.ekf, io.ekf.batch, view, workspace)   # the handle the forecast descends from (never written)
        self.h = h
        self.ticks_to_limit = ticks_to_limit

    def lookahead(self, u, h, mask=None, sigma_r_max=float("inf"), sigma_theta_max=float("inf")):
        """h more ticks from this forecast: the bits of one call over the sum of the horizons."""
        f = forecast(self, u, h, mask, sigma_r_max, sigma_theta_max)
        f.h += self.h
        return f


def forecast(rec, u, h, mask=None, sigma_r_max=float("inf"), sigma_theta_max=float("inf")):
    """`DeviceIO.lookahead` / `Forecast.lookahead`: the records of `rec` (a `DeviceRecords`) h ticks ahead, as a `Forecast`."""
    B = rec.batch
    src = rec._check(u, "u", (B, 6))
    h = check_horizon(h)
    rec._check_mask(mask)
    coast = make_coast(sigma_r_max, sigma_theta_max)
    K = lookahead_lib()
    view = rec._view()
    nbytes = kcheck(K.qlk_workspace_bytes(C.byref(view)))
    workspace = rec._alloc([(nbytes,)], "uint8")[0]
    ticks = rec._alloc([(B,)], "int32")[0] if coast is not None else None
    ahead = QleDeviceView()
    with rec._ordered(view, u, mask):
        kcheck(K.qlk_lookahead(C.byref(view), C.byref(rec.ekf.params), u.data_ptr(), _t.FLOATS[src], h,
                               None if mask is None else mask.data_ptr(), workspace.data_ptr(), nbytes, C.byref(ahead),
                               None if coast is None else C.byref(coast), None if ticks is None else ticks.data_ptr()))
    return Forecast(rec, ahead, workspace, h, ticks)
