"""ctypes binding of include/qle_gate.h (libqle_gate.so): the chi-square gate in front of the fused tick, fed from GPU memory.

One read-only kernel (k_pregate, csrc/ekf_pregate.hpp) between `qdv_pack_inputs` and the unchanged tick of `qle_run`: it clears the
mask word of the tick's tag record where NIS = delta_y^T S^-1 delta_y, evaluated against the predicted state, exceeds chi2_max.
`DeviceIO.tick(..., chi2_max=...)` and `DeviceIO.innovation` (devio.py) are the callers.  There is no fallback: a missing library is
an error.
"""
import ctypes as C
import os

from ._lib import QleDeviceView, QleError, QleInputsView, QleParams, load_side_library

_HERE = os.path.dirname(os.path.abspath(__file__))
GATE_LIB_PATH = os.environ.get("QLE_GATE_LIB") or os.path.join(_HERE, "libqle_gate.so")

QGT_F32, QGT_F64 = 0, 1
_vp = C.c_void_p
_pview, _pin, _ppar = C.POINTER(QleDeviceView), C.POINTER(QleInputsView), C.POINTER(QleParams)
# every symbol include/qle_gate.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "qgt_last_error": (C.c_char_p, []),
    "qgt_gate_tick": (C.c_int, [_pview, _pin, _ppar, C.c_double, _vp, _vp, _vp, _vp, C.c_int32]),
    "qgt_innovation": (C.c_int, [_pview, _pin, _ppar, _vp, _vp, _vp, C.c_int32]),
    "qgt_launch_count": (C.c_int64, []),
}

_glib = None


def gate_lib():
    """Load libqle_gate.so; raises (never falls back) when it is missing."""
    global _glib
    if _glib is None:
        _glib = load_side_library(GATE_LIB_PATH, SYMBOLS, "the gate in front of the fused tick", needs_tick_library=True)
    return _glib


def gcheck(rc):
    if rc != 0:
        raise QleError(rc, gate_lib().qgt_last_error().decode())
