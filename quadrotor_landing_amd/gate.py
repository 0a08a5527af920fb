"""ctypes binding of include/qle_gate.h (libqle_gate.so): the chi-square gate in front of the fused tick, fed from GPU memory.

One read-only kernel (k_pregate, csrc/ekf_pregate.hpp) between `qdv_pack_inputs` and the unchanged tick of `qle_run`: it clears the
mask word of the tick's tag record where NIS = delta_y^T S^-1 delta_y, evaluated against the predicted state, exceeds chi2_max.
`DeviceIO.tick(..., chi2_max=...)` and `DeviceIO.innovation` (devio.py) are the callers.  There is no fallback: a missing library is
an error.
"""
import ctypes as C

from ._lib import QLE_ERR_STATE, QleDeviceView, QleError, QleInputsView, QleParams, SideLibrary

QGT_F32, QGT_F64 = 0, 1
_vp = C.c_void_p
_pview, _pin, _ppar = C.POINTER(QleDeviceView), C.POINTER(QleInputsView), C.POINTER(QleParams)
# every symbol include/qle_gate.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "qgt_last_error": (C.c_char_p, []),
    "qgt_gate_tick": (C.c_int, [_pview, _pin, _ppar, C.c_double, _vp, _vp, _vp, _vp, C.c_int32]),
    "qgt_innovation": (C.c_int, [_pview, _pin, _ppar, _vp, _vp, _vp, C.c_int32]),
    "qgt_launch_count": (C.c_int64, []),
    "qgt_launch_census_begin": (C.c_int, []),
    "qgt_launch_census_end": (C.c_int, [C.c_char_p, C.c_int64, C.POINTER(C.c_int64)]),
}

GATE = SideLibrary("gate", "QLE_GATE_LIB", SYMBOLS, "the gate in front of the fused tick", "qgt_last_error", needs_tick_library=True)
GATE_LIB_PATH, gate_lib, gcheck = GATE.path, GATE.load, GATE.check


def check_chi2_max(chi2_max):
    """The gate's threshold as a float > 0 (inf accepts every finite NIS; NaN refused)."""
    chi2_max = float(chi2_max)
    if not chi2_max > 0.0:
        raise ValueError(f"chi2_max must be > 0 (got {chi2_max})")
    return chi2_max


def refuse_multirate(params, what="the gate"):
    """The gate and everything else that evaluates an innovation against the stored state is refused with multirate_ekf."""
    if params.multirate_ekf:
        raise QleError(QLE_ERR_STATE, f"{what} does not support multirate_ekf: a delayed measurement's innovation belongs to a history entry")
