"""ctypes binding of include/qle_sequence.h (libqle_sequence.so): a whole tensor sequence per call at the device-tensor boundary.

`qsq_pack` puts K ticks of device tensors (u [K,B,6], tag poses for the M ticks that have one, masks) into a device-resident
sequence with ceil(K / 32) launches of k_sq_pack (csrc/sequence_kernels.hpp); `qsq_run` runs the ticks from one C loop and
interleaves the existing read-only launches -- the chi-square gate, the report, the NEES -- as the per-tick path of devio.py does
from Python.  `DeviceIO.sequence` and `DeviceIO.run` (devio.py) are the callers; the records and results are, bit for bit, those of
the per-tick path.  There is no fallback: a missing library is an error.
"""
import ctypes as C

from . import _tensors as _t
from . import consistency as _cons
from . import gate as _gate
from ._lib import QleDeviceView, QleParams, SideLibrary
from .records import REPORT

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
    "qsq_launch_census_begin": (C.c_int, []),
    "qsq_launch_census_end": (C.c_int, [C.c_char_p, C.c_int64, C.POINTER(C.c_int64)]),
    "qsq_pack": (C.c_int, [C.POINTER(QleDeviceView), _vp, C.c_int64, C.c_int64, _vp, _vp, _vp, C.c_int32]),
    "qsq_run": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.POINTER(QsqRunOpts)]),
}

# the libraries it links are loaded first, so that it runs on the copies the per-tick path uses
SEQUENCE = SideLibrary("sequence", "QLE_SEQUENCE_LIB", SYMBOLS, "the sequence boundary", "qsq_last_error", needs_tick_library=True,
                       after=(_t.DEVIO, _gate.GATE, _cons.CONSISTENCY))
SEQUENCE_LIB_PATH, sequence_lib, scheck = SEQUENCE.path, SEQUENCE.load, SEQUENCE.check


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


def check_sequence(io, u_seq, z_seq, mask_seq, n_ticks, meas_ticks, t0):
    """The argument checks of `DeviceIO.sequence` / `DeviceSequence.pack` (before any GPU call).  Returns (source dtype name, n).
    n_ticks None: the sequence is as long as u_seq."""
    B = io.batch
    shape = tuple(getattr(u_seq, "shape", ()))
    if len(shape) != 3 or shape[0] < 1:
        raise ValueError(f"u_seq: expected shape (K, {B}, 6) with K >= 1, got {shape}")
    n = int(shape[0])
    src = io._check(u_seq, "u_seq", (n, B, 6))
    if n_ticks is None:
        n_ticks = n
    t0, _ = check_window(t0, n, n_ticks)
    ticks = check_meas_ticks(meas_ticks, n_ticks)
    m = sum(1 for t in ticks if t0 <= t < t0 + n)
    if z_seq is None:
        if mask_seq is not None:
            raise ValueError("mask_seq given without z_seq")
        if m > 0:
            raise ValueError(f"{m} ticks of the range have a tag slot (meas_ticks) but z_seq is None")
    else:
        if m == 0:
            raise ValueError("z_seq given but no tick of the range has a tag slot (meas_ticks)")
        if io._check(z_seq, "z_seq", (m, B, 7)) != src:
            raise ValueError("u_seq and z_seq must have the same dtype")
        if mask_seq is not None:
            io._check(mask_seq, "mask_seq", (m, B), _t.MASKS)
    return src, n


def check_window(t0, n, n_ticks):
    """Ticks [t0, t0 + n) of a sequence of n_ticks (n None: to its end) as ints; a window that reaches beyond it is refused."""
    t0 = int(t0)
    n = n_ticks - t0 if n is None else int(n)
    if t0 < 0 or n < 0 or t0 + n > n_ticks:
        raise ValueError(f"ticks [{t0}, {t0 + n}) reach beyond the sequence of {n_ticks} ticks")
    return t0, n


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

    @staticmethod
    def window(io, seq, t0, n):
        """(t0, n) of ticks [t0, t0 + n) of `seq` (n None: to its end), which has to be an open sequence of `io`'s handle."""
        if not isinstance(seq, DeviceSequence) or seq.io.ekf is not io.ekf or seq.inputs is None:
            raise ValueError("seq: expected an open DeviceSequence made by this handle's DeviceIO.sequence")
        return check_window(t0, n, seq.n_ticks)

    def slots(self, t0, n):
        """Tag slots among ticks [t0, t0 + n)."""
        return sum(1 for t in self.meas_ticks if t0 <= t < t0 + n)

    def pack(self, u_seq, z_seq=None, mask_seq=None, t0=0):
        """Fill ticks [t0, t0 + n), n = len(u_seq): u_seq [n,B,6], z_seq [m,B,7] and mask_seq [m,B] (uint8 / bool; None = all) for
        the m of those ticks that have a tag slot, in tick order.  ceil(n / 32) launches; asynchronous, the tensors may be reused as
        soon as the call returns."""
        io = self.io
        src, n = check_sequence(io, u_seq, z_seq, mask_seq, self.n_ticks, self.meas_ticks, t0)
        S = sequence_lib()
        view = io._view()
        with io._ordered(view, u_seq, z_seq, mask_seq):
            scheck(S.qsq_pack(C.byref(view), self.inputs._h, int(t0), n, u_seq.data_ptr(), None if z_seq is None else z_seq.data_ptr(),
                              None if mask_seq is None else mask_seq.data_ptr(), _t.FLOATS[src]))
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


def make(io, u_seq, z_seq, meas_ticks, mask_seq):
    """`DeviceIO.sequence`: a K-tick `DeviceSequence` of `io`, created and packed with one call."""
    _, n = check_sequence(io, u_seq, z_seq, mask_seq, None, meas_ticks, 0)
    seq = DeviceSequence(io, n, check_meas_ticks(meas_ticks, n))
    try:
        return seq.pack(u_seq, z_seq, mask_seq)
    except Exception:
        seq.close()
        raise


def run(io, seq, t0, n, chi2_max, return_nis, trace_every, trace, x_true_seq, blocks, chi2_hi, dtype):
    """`DeviceIO.run`: the checks (before any GPU call), the `QsqRunOpts` and its output buffers, qsq_run, the `SequenceResult`."""
    B = io.batch
    t0, n = DeviceSequence.window(io, seq, t0, n)
    if chi2_max is None:
        if return_nis:
            raise ValueError("return_nis given without chi2_max")
    else:
        chi2_max = _gate.check_chi2_max(chi2_max)
        _gate.refuse_multirate(io.ekf.params)
    kinds = (trace,) if isinstance(trace, str) else tuple(trace)
    if set(kinds) - set(TRACE_KINDS) or not kinds:
        raise ValueError(f"trace: expected kinds out of {TRACE_KINDS}, got {kinds}")
    if trace_every is None:
        if kinds != ("report",) or x_true_seq is not None:
            raise ValueError("trace kinds or x_true_seq given without trace_every")
        kinds, J = (), 0
    else:
        if int(trace_every) != trace_every or int(trace_every) < 1:
            raise ValueError(f"trace_every must be an integer >= 1 (got {trace_every})")
        trace_every = int(trace_every)
        J = n // trace_every
    dn = io._out_dtype(dtype)
    opts = QsqRunOpts()
    opts.struct_size = C.sizeof(opts)
    opts.dst_dtype = _t.FLOATS[dn]
    opts.trace_every = trace_every or 0
    if "nees" in kinds:
        if x_true_seq is None:
            raise ValueError('trace "nees" needs x_true_seq')
        opts.true_dtype = _t.FLOATS[io._check(x_true_seq, "x_true_seq", (J, B, 16))]
        opts.blocks = _cons.block_mask(blocks, io.ekf.num_states)
        opts.chi2_hi = _cons.check_chi2_hi(chi2_hi)
    elif x_true_seq is not None:
        raise ValueError('x_true_seq given without "nees" in trace')
    S = sequence_lib()
    opts.params = C.pointer(io.ekf.params)
    view = io._view()
    Bp = int(view.padded_batch)
    res = SequenceResult()
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None   # noqa: E731
    if chi2_max is not None:
        opts.chi2_max = chi2_max
        m = seq.slots(t0, n)
        acc = io._alloc([(m, Bp)], "uint8")[0]
        nis = io._alloc([(m, Bp)], dn)[0] if return_nis else None
        opts.accepted, opts.nis = ptr(acc), ptr(nis)
        res.accepted, res.nis = acc[:, :B], None if nis is None else nis[:, :B]
    if "report" in kinds:
        bufs = io._alloc([(J, Bp) + s for _, s in REPORT], dn)
        opts.pose, opts.pose_cov, opts.vel, opts.bias = (ptr(b) for b in bufs)
        res.report = {k: b[:, :B] for (k, _), b in zip(REPORT, bufs)}
    if "nees" in kinds:
        nees, summary = io._alloc([(J, Bp)], dn)[0], io._alloc([(J, 8)], "float64")[0]
        opts.x_true_seq, opts.nees, opts.summary = ptr(x_true_seq), ptr(nees), ptr(summary)
        res.nees, res.summary = nees[:, :B], summary
        if J == 0:
            opts.true_dtype, opts.blocks, opts.chi2_hi = 0, 0, 0.0
    with io._ordered(view, x_true_seq):
        scheck(S.qsq_run(io.ekf._h, seq.inputs._h, t0, n, C.byref(opts)))
    return res
