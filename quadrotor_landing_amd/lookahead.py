"""ctypes binding of include/qle_lookahead.h (libqle_lookahead.so): state and covariance h ticks ahead, read-only.

`qlk_lookahead` loads every filter's record once, applies the predict h times in registers with the IMU sample held (k_lookahead:
csrc/ekf_lookahead.hpp) and stores the forecast records into a workspace of the caller's; the forecast is a `qle_device_view` of its
own, so every read-only consumer of a view works on it unchanged.  `Forecast` owns that workspace (a torch tensor) and the view and
offers the consumers: `state`, `report`, `health`, `nees` and `lookahead` again (forecasts chain).  `DeviceIO.lookahead` (devio.py) is
the caller for device tensors, `BatchedRelativePoseEKF.lookahead` (ekf.py) for host arrays.  There is no fallback: a missing library
is an error.
"""
import ctypes as C
import os

from ._lib import QleDeviceView, QleError, QleParams, load_side_library

_HERE = os.path.dirname(os.path.abspath(__file__))
LOOKAHEAD_LIB_PATH = os.environ.get("QLE_LOOKAHEAD_LIB") or os.path.join(_HERE, "libqle_lookahead.so")

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
    "qlk_workspace_bytes": (C.c_int64, [_pview]),
    "qlk_lookahead": (C.c_int, [_pview, _pparams, _vp, C.c_int32, C.c_int32, _vp, _vp, C.c_int64, _pview, _pcoast, _vp]),
    "qlk_lookahead_host": (C.c_int, [_pview, _pparams, C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_uint8), _vp, C.c_int64, _pview, _pcoast,
                                     C.POINTER(C.c_int32)]),
}

_klib = None


def lookahead_lib():
    """Load libqle_lookahead.so; raises (never falls back) when it is missing."""
    global _klib
    if _klib is None:
        _klib = load_side_library(LOOKAHEAD_LIB_PATH, SYMBOLS, "the look-ahead kernel", needs_tick_library=True)
    return _klib


def kcheck(rc):
    if rc < 0:
        raise QleError(rc, lookahead_lib().qlk_last_error().decode())
    return rc


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


class Forecast:
    """The forecast of a `DeviceIO` (or of another `Forecast`) h ticks ahead: owns the workspace tensor the records live in and the
    `qle_device_view` of them.  `ticks_to_limit`: a device int32 tensor [B] (the coast budget), or None when no limit was given.
    Nothing here writes a handle; the consumers are the existing read-only bindings, run on the forecast view."""

    def __init__(self, io, view, workspace, h, ticks_to_limit):
        self.ekf = io.ekf              # parameters, batch, device: the handle the forecast descends from (never written)
        self.view = view
        self.workspace = workspace
        self.h = h
        self.ticks_to_limit = ticks_to_limit
        # a DeviceIO whose view is the forecast view: state(), report(), health(), nees() and lookahead() run on it unchanged
        self._io = type(io)(io.ekf)
        self._io._view = lambda: self.view

    def state(self, dtype=None, out=None):
        """(x [B,16], P [B,n,n]) of the forecast as device tensors; a skipped filter's rows are zero."""
        return self._io.state(dtype=dtype, out=out)

    def report(self, dtype=None, out=None):
        """What the node would publish at the horizon (`DeviceIO.report`)."""
        return self._io.report(dtype=dtype, out=out)

    def health(self, **kw):
        """Which filters will be flagged at the horizon (`DeviceIO.health`); skipped filters are uninitialised there."""
        return self._io.health(**kw)

    def nees(self, x_true, **kw):
        """NEES of the forecast against a truth at the horizon (`DeviceIO.nees`)."""
        return self._io.nees(x_true, **kw)

    def lookahead(self, u, h, mask=None, sigma_r_max=float("inf"), sigma_theta_max=float("inf")):
        """h more ticks from this forecast: the bits of one call over the sum of the horizons."""
        f = self._io.lookahead(u, h, mask=mask, sigma_r_max=sigma_r_max, sigma_theta_max=sigma_theta_max)
        f.h += self.h
        return f
