"""ctypes binding of include/qle_bank.h (libqle_bank.so): posterior weights and one fused estimate per bank of filters, read-only.

A handle of B filters is G = B / M banks of M consecutive members (M a power of two in 2..64, B a multiple of M): filters with
different noise parameters (`set_filter_params`) fed the same IMU samples and tag poses.  `qbk_fuse` takes the members' unnormalised
log-weights -- the innovation log-likelihood a `score.Scorer` accumulates, or anything else -- and in ONE read-only launch (k_bank_fuse:
csrc/ekf_bank.hpp) writes every bank's moment-matched mixture, xbar = sum w_i x_i and Pbar = sum w_i (P_i + d_i d_i^T) in the filter's
error-state convention, into a workspace of the caller's; the result is a `qle_device_view` of its own, so every read-only consumer of a
view works on it unchanged.  `Fused` owns that workspace (a torch tensor) and the view and offers the consumers: `state`, `report`,
`health`, `nees`.  `DeviceIO.bank(M)` (devio.py) is the caller for device tensors, `BatchedRelativePoseEKF.fuse_banks` (ekf.py) for host
arrays.  There is no fallback: a missing library is an error.

Not provided: `lookahead` of a fused view (which Q a fused estimate coasts under is a modelling choice, and the fused view carries no
per-filter parameters), banks that cross a 64-filter tile, and a member count that is not a power of two.
"""
import ctypes as C
import os

from ._lib import QleDeviceView, QleError, load_side_library

_HERE = os.path.dirname(os.path.abspath(__file__))
BANK_LIB_PATH = os.environ.get("QLE_BANK_LIB") or os.path.join(_HERE, "libqle_bank.so")

MAX_MEMBERS = 64

_vp = C.c_void_p
_pview = C.POINTER(QleDeviceView)
# every symbol include/qle_bank.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "qbk_last_error": (C.c_char_p, []),
    "qbk_launch_count": (C.c_int64, []),
    "qbk_workspace_bytes": (C.c_int64, [_pview, C.c_int32]),
    "qbk_fuse": (C.c_int, [_pview, C.c_int32, _vp, _vp, _vp, C.c_int64, _pview, _vp, _vp]),
    "qbk_fuse_host": (C.c_int, [_pview, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_uint8), _vp, C.c_int64, _pview, C.POINTER(C.c_double),
                                C.POINTER(C.c_int32)]),
}

_blib = None


def bank_lib():
    """Load libqle_bank.so; raises (never falls back) when it is missing."""
    global _blib
    if _blib is None:
        _blib = load_side_library(BANK_LIB_PATH, SYMBOLS, "the filter-bank kernel", needs_tick_library=False)
    return _blib


def bcheck(rc):
    if rc < 0:
        raise QleError(rc, bank_lib().qbk_last_error().decode())
    return rc


def check_members(M, batch):
    """M as an int: a power of two in 2..MAX_MEMBERS that divides the batch; anything else is refused here, before any native call."""
    if isinstance(M, bool) or not isinstance(M, (int, float)) and not hasattr(M, "__index__") or int(M) != M:
        raise ValueError(f"members must be an integer (got {M!r})")
    M = int(M)
    if not 2 <= M <= MAX_MEMBERS or M & (M - 1):
        raise ValueError(f"members must be a power of two in 2..{MAX_MEMBERS} (got {M})")
    if batch % M:
        raise ValueError(f"the batch of {batch} filters is not a multiple of members = {M}")
    return M


class _FusedHandle:
    """What a `DeviceIO` reads of its handle, for the fused view: `batch` is the number of banks, everything else (parameters, dtype,
    device, num_states) is the handle's.  Never written through."""

    def __init__(self, ekf, banks):
        self._ekf = ekf
        self.batch = banks

    def __getattr__(self, name):
        return getattr(self._ekf, name)


class Fused:
    """The fused estimate of a `DeviceIO`'s banks: owns the workspace tensor the G records live in and the `qle_device_view` of them.
    `w` [B] (float64): the members' posterior weights, 0 for an invalid member; `best` [G] (int32): the filter index of each bank's
    reference member (the lowest-index valid member of the largest log-weight), -1 for an empty bank, whose record is all zero
    ("uninitialised" to every consumer).  Nothing here writes a handle; the consumers are the existing read-only bindings, run on the
    fused view.  `nees` takes its static biases from the handle's shared parameters: the fused view carries no per-filter parameters.
    There is no `lookahead`: which Q a fused estimate coasts under is a modelling choice."""

    def __init__(self, io, view, workspace, members, w, best):
        self.ekf = io.ekf              # the handle the estimate descends from (never written)
        self.members = check_members(members, io.ekf.batch)
        self.banks = io.ekf.batch // self.members
        self.view = view
        self.workspace = workspace
        self.w = w
        self.best = best
        # a DeviceIO over G filters whose view is the fused view: state(), report(), health() and nees() run on it unchanged
        self._io = type(io)(_FusedHandle(io.ekf, self.banks))
        self._io._view = lambda: self.view

    def state(self, dtype=None, out=None):
        """(x [G,16], P [G,n,n]) of the fused estimates as device tensors; an empty bank's rows are zero."""
        return self._io.state(dtype=dtype, out=out)

    def report(self, dtype=None, out=None):
        """What the node would publish for every bank (`DeviceIO.report`)."""
        return self._io.report(dtype=dtype, out=out)

    def health(self, **kw):
        """`DeviceIO.health` of the fused estimates; empty banks are uninitialised there."""
        return self._io.health(**kw)

    def nees(self, x_true, **kw):
        """NEES of the fused estimates against a truth x_true [G,16] (`DeviceIO.nees`)."""
        return self._io.nees(x_true, **kw)


class Bank:
    """The banks of a `DeviceIO`: `members` consecutive filters each.  `fuse` may be called any number of times; every call reads the
    handle's current state."""

    def __init__(self, io, members):
        self.io = io
        self.members = check_members(members, io.ekf.batch)
        self.banks = io.ekf.batch // self.members

    def fuse(self, logw, mask=None):
        """The posterior weights and the fused estimate of every bank from the members' unnormalised log-weights logw [B] (a float64
        device tensor; a `score.Scorer` is accepted in its place and contributes `result().loglik`) in ONE read-only launch.  A member
        counts when mask[i] != 0 (uint8 / bool [B]; None = all), it holds a state and its log-weight is finite.  Returns a `Fused`.
        Asynchronous, no synchronisation; the handle is not written."""
        io = self.io
        B = io.ekf.batch
        from . import score as _score
        if isinstance(logw, _score.Scorer):
            logw = logw.result().loglik
        io._check(logw, "logw", (B,), ("float64",))
        if mask is not None:
            io._check_mask(mask, B)
        from . import devio as _dv
        D, K = _dv.devio_lib(), bank_lib()
        view = io._view()
        nbytes = bcheck(K.qbk_workspace_bytes(C.byref(view), self.members))
        workspace = io._alloc([(nbytes,)], "uint8")[0]
        w = io._alloc([(B,)], "float64")[0]
        best = io._alloc([(self.banks,)], "int32")[0]
        fused = QleDeviceView()
        with io._ordered(D, view, logw, mask):
            bcheck(K.qbk_fuse(C.byref(view), self.members, logw.data_ptr(), None if mask is None else mask.data_ptr(), workspace.data_ptr(),
                              nbytes, C.byref(fused), w.data_ptr(), best.data_ptr()))
        return Fused(io, fused, workspace, self.members, w, best)
