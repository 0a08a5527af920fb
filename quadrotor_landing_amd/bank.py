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

from ._lib import QleDeviceView, SideLibrary
from .records import ViewRecords
from .score import Scorer

MAX_MEMBERS = 64

_vp = C.c_void_p
_pview = C.POINTER(QleDeviceView)
# every symbol include/qle_bank.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "qbk_last_error": (C.c_char_p, []),
    "qbk_launch_count": (C.c_int64, []),
    "qbk_launch_census_begin": (C.c_int, []),
    "qbk_launch_census_end": (C.c_int, [C.c_char_p, C.c_int64, C.POINTER(C.c_int64)]),
    "qbk_workspace_bytes": (C.c_int64, [_pview, C.c_int32]),
    "qbk_fuse": (C.c_int, [_pview, C.c_int32, _vp, _vp, _vp, C.c_int64, _pview, _vp, _vp]),
    "qbk_fuse_host": (C.c_int, [_pview, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_uint8), _vp, C.c_int64, _pview, C.POINTER(C.c_double),
                                C.POINTER(C.c_int32)]),
}

BANK = SideLibrary("bank", "QLE_BANK_LIB", SYMBOLS, "the filter-bank kernel", "qbk_last_error")
BANK_LIB_PATH, bank_lib, bcheck = BANK.path, BANK.load, BANK.check


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


class Fused(ViewRecords):
    """The fused estimate of a `DeviceIO`'s banks: owns the workspace tensor the G records live in and the `qle_device_view` of them.
    `w` [B] (float64): the members' posterior weights, 0 for an invalid member; `best` [G] (int32): the filter index of each bank's
    reference member (the lowest-index valid member of the largest log-weight), -1 for an empty bank, whose record is all zero
    ("uninitialised" to every consumer).  Nothing here writes a handle; the consumers (`state`, `report`, `health`, `nees`, over G
    filters) are the read-only bindings of `DeviceRecords`, run on the fused view.  `nees` takes its static biases from the handle's
    shared parameters: the fused view carries no per-filter parameters.  There is no `lookahead`: which Q a fused estimate coasts
    under is a modelling choice."""

    def __init__(self, io, view, workspace, members, w, best):
        self.members = check_members(members, io.ekf.batch)
        self.banks = io.ekf.batch // self.members
        super().__init__(io.ekf, self.banks, view, workspace)   # the handle the estimate descends from (never written)
        self.w = w
        self.best = best


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
        if isinstance(logw, Scorer):
            logw = logw.result().loglik
        io._check(logw, "logw", (B,), ("float64",))
        io._check_mask(mask)
        K = bank_lib()
        view = io._view()
        nbytes = bcheck(K.qbk_workspace_bytes(C.byref(view), self.members))
        workspace = io._alloc([(nbytes,)], "uint8")[0]
        w = io._alloc([(B,)], "float64")[0]
        best = io._alloc([(self.banks,)], "int32")[0]
        fused = QleDeviceView()
        with io._ordered(view, logw, mask):
            bcheck(K.qbk_fuse(C.byref(view), self.members, logw.data_ptr(), None if mask is None else mask.data_ptr(), workspace.data_ptr(),
                              nbytes, C.byref(fused), w.data_ptr(), best.data_ptr()))
        return Fused(io, fused, workspace, self.members, w, best)
