"""ctypes binding of include/qle_sequence.h (libqle_sequence.so): a whole tensor sequence per call at the device-tensor boundary.

`qsq_pack` puts K ticks of device tensors (u [K,B,6], tag poses for the M ticks that have one, masks) into a device-resident
sequence with ceil(K / 32) launches of k_sq_pack (csrc/sequence_kernels.hpp); `qsq_run` runs the ticks from one C loop and
interleaves the existing read-only launches -- the chi-square gate, the report, the NEES -- as the per-tick path of devio.py does
from Python.  `DeviceIO.sequence` and `DeviceIO.run` (devio.py) are the callers; the records and results are, bit for bit, those of
the per-tick path.  There is no fallback: a missing library is an error.
"""
import ctypes as C
import os

from . import consistency as _cons
from . import gate as _gate
from ._lib import QleDeviceView, QleError, QleParams, load_side_library

_HERE = os.path.dirname(os.path.abspath(__file__))
SEQUENCE_LIB_PATH = os.environ.get("QLE_SEQUENCE_LIB") or os.path.join(_HERE, "libqle_sequence.so")

QSQ_F32, QSQ_F64 = 0, 1
CHUNK = 32   # ticks one launch of k_sq_pack fills (QSQ_CHUNK)
TRACE_KINDS = ("report", "nees")

_vp = C.c_void_p


class QsqRunOpts(C.Structure):
    """`struct qsq_run_opts`: what qsq_run does besides the ticks.  Every per-tick output slice has a pitch of padded_batch filters."""
    _fields_ = [("struct_size", C.c_uint32), ("dst_dtype", C.c_int32), ("chi2_max", C.c_double), ("params", C.POINTER(QleParams)),
                ("trace_every", C.c_int64), ("accepted", _vp), ("nis", _vp), ("pose", _vp), ("pose_cov", _vp), ("vel", _vp), ("bias", _vp),
                ("x_true_seq", _vp), ("true_dtype", C.c_int32), ("blocks", C.c_uint32), ("chi2_hi", C.c_double), ("nees", _vp),
                ("summary", _vp)]


# every symbol include/qle_sequence.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "qsq_last_error": (C.c_char_p, []),
    "qsq_launch_count": (C.c_int64, []),
    "qsq_pack": (C.c_int, [C.POINTER(QleDeviceView), _vp, C.c_int64, C.c_int64, _vp, _vp, _vp, C.c_int32]),
    "qsq_run": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.POINTER(QsqRunOpts)]),
}

_slib = None


def sequence_lib():
    """Load libqle_sequence.so; raises (never falls back) when it is missing.  The libraries it links are loaded first, so that it
    runs on the copies the per-tick path uses."""
    global _slib
    if _slib is None:
        from . import devio as _devio
        _devio.devio_lib(), _gate.gate_lib(), _cons.consistency_lib()
        _slib = load_side_library(SEQUENCE_LIB_PATH, SYMBOLS, "the sequence boundary", needs_tick_library=True)
    return _slib


def scheck(rc):
    if rc != 0:
        raise QleError(rc, sequence_lib().qsq_last_error().decode())


def check_meas_ticks(meas_ticks, n_ticks):
    """meas_ticks as a list of ints: strictly increasing tick indices in [0, n_ticks)."""
    if meas_ticks is None:
        return []
    try:
        ticks = [int(t) for t in meas_ticks]
    except (TypeError, ValueError):
        raise ValueError("meas_ticks: expected a host list of tick indices") from None
    if any(int(a) != a for a in meas_ticks):
        raise ValueError("meas_ticks: tick indices must be integers")
    if any(t < 0 or t >= n_ticks for t in ticks):
        raise ValueError(f"meas_ticks: tick indices must lie in [0, {n_ticks})")
    if any(b <= a for a, b in zip(ticks, ticks[1:])):
        raise ValueError("meas_ticks: tick indices must be strictly increasing")
    return ticks


class DeviceSequence:
    """K ticks of inputs in the records the tick kernels read, filled from device tensors (`DeviceIO.sequence`).  `pack` refills
    any window of it (streaming use), `close` frees it.  `inputs` is the `InputSequence` underneath: `ekf.run(seq.inputs, ...)` and
    `seq.inputs.download_tick(t)` work on it."""

    def __init__(self, io, n_ticks, meas_ticks):
        self.io, self.n_ticks, self.meas_ticks = io, int(n_ticks), list(meas_ticks)
        has = [0] * self.n_ticks
        for t in self.meas_ticks:
            has[t] = 1
        self.inputs = io.ekf.make_inputs(self.n_ticks, has)

    def slots(self, t0, n):
        """Tag slots among ticks [t0, t0 + n)."""
        return sum(1 for t in self.meas_ticks if t0 <= t < t0 + n)

    def pack(self, u_seq, z_seq=None, mask_seq=None, t0=0):
        """Fill ticks [t0, t0 + n), n = len(u_seq): u_seq [n,B,6], z_seq [m,B,7] and mask_seq [m,B] (uint8 / bool; None = all) for
        the m of those ticks that have a tag slot, in tick order.  ceil(n / 32) launches; asynchronous, the tensors may be reused as
        soon as the call returns."""
        io = self.io
        src, n = io._check_sequence(u_seq, z_seq, mask_seq, self.n_ticks, self.meas_ticks, t0)
        from . import devio as _devio
        D, S = _devio.devio_lib(), sequence_lib()
        view = io._view()
        with io._ordered(D, view, u_seq, z_seq, mask_seq):
            scheck(S.qsq_pack(C.byref(view), self.inputs._h, int(t0), n, u_seq.data_ptr(), None if z_seq is None else z_seq.data_ptr(),
                              None if mask_seq is None else mask_seq.data_ptr(), _devio._FLOATS[src]))
        return self

    def close(self):
        if self.inputs is not None:
            self.inputs.close()
            self.inputs = None


class SequenceResult:
    """What `DeviceIO.run` hands back, as device tensors (views of buffers with a pitch of padded_batch filters; None where not asked
    for): accepted [m,B] (uint8) and nis [m,B], one slice per tag tick of the range, of a gated run; report, a dict of pose [J,B,7],
    pose_cov [J,B,6,6], vel [J,B,3], bias [J,B,6]; nees [J,B] and summary [J,8] (consistency.SUMMARY_FIELDS).  Slice j of a trace is
    taken after tick t0 + (j + 1) * trace_every - 1."""

    def __init__(self, accepted=None, nis=None, report=None, nees=None, summary=None):
        self.accepted, self.nis, self.report, self.nees, self.summary = accepted, nis, report, nees, summary
