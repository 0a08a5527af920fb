"""ctypes binding of include/qle_stateio.h (libqle_stateio.so): write, copy and permute filter states in GPU memory.

`qsi_pack_state` is the inverse of `qdv_unpack_state` (k_si_pack: x and P tensors -> state records, the bits of `qle_set_state`) and
`qsi_copy` makes filter i of one view a bitwise copy of filter index[i] of another (k_si_copy).  Over them, for a `DeviceIO` (devio.py):
`set_state` from device tensors, `snapshot` -> a `Snapshot` that owns its records and is read through the same calls as the handle
(`state`, `report`, `health`, `nees`, `lookahead`), `restore`, `gather` and `fork`; and `gather_host` for the host arrays of
`BatchedRelativePoseEKF.gather_state`.  After every write of a handle's records the handle is told with `qle_mark_state_written`
(include/qle_ekf.h): the tick library owns its host flags.  There is no fallback: a missing library is an error.

What a snapshot holds is the state: the record words a tick moves, and the per-filter parameter records when asked.  It holds neither
the multirate history nor the counters (upds_since_correction, the rate limiter of `enable_gating`): after a write a multirate
history restarts at the next tick for every filter, as after `set_state` on the host path, and the counters go on as they were.
"""
import ctypes as C

from . import _tensors as _t
from . import lookahead as _look
from ._lib import QLE_ERR_STATE, QLE_F32, QleDeviceView, QleError, SideLibrary, check, lib
from .records import ViewRecords

QSI_F32, QSI_F64 = 0, 1
PARAM_WORDS = 24

_vp = C.c_void_p
_pview = C.POINTER(QleDeviceView)
# every symbol include/qle_stateio.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "qsi_last_error": (C.c_char_p, []),
    "qsi_launch_count": (C.c_int64, []),
    "qsi_launch_census_begin": (C.c_int, []),
    "qsi_launch_census_end": (C.c_int, [C.c_char_p, C.c_int64, C.POINTER(C.c_int64)]),
    "qsi_workspace_bytes": (C.c_int64, [_pview]),
    "qsi_pack_state": (C.c_int, [_pview, _vp, _vp, C.c_int32, _vp]),
    "qsi_copy": (C.c_int, [_pview, _pview, _vp, _vp, C.c_int32, _vp]),
    "qsi_copy_host": (C.c_int, [_pview, _pview, C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.c_int32, C.POINTER(C.c_uint8)]),
}

STATEIO = SideLibrary("stateio", "QLE_STATEIO_LIB", SYMBOLS, "device state I/O", "qsi_last_error")
STATEIO_LIB_PATH, stateio_lib, scheck = STATEIO.path, STATEIO.load, STATEIO.check


def refuse_masked_multirate(params, mask, what):
    """A write of some filters is refused with multirate_ekf: the handle restarts the history of every filter after a write."""
    if mask is not None and params.multirate_ekf:
        raise QleError(QLE_ERR_STATE, f"{what} with a mask does not support multirate_ekf: a written state restarts the history of every filter, "
                                      "the ones the mask leaves alone included (write the whole batch)")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _copy_view(view):
    v = QleDeviceView()
    C.memmove(C.byref(v), C.byref(view), C.sizeof(QleDeviceView))
    return v


class Snapshot(ViewRecords):
    """The records of a `DeviceIO` at one moment: owns the workspace tensor they live in, a copy of the per-filter parameter records
    when it was taken `with_params` (`params`, else None: its view then names the handle's live parameter records, which `report`
    reads for the static biases), and the `qle_device_view` of them.  Nothing writes it afterwards; `state`, `report`, `health` and
    `nees` are the read-only bindings of `DeviceRecords` run on the snapshot, `lookahead` a forecast from it."""

    def __init__(self, io, view, workspace, params):
        super().__init__(io.ekf, io.batch, view, workspace)
        self.params = params

    def lookahead(self, u, h, mask=None, sigma_r_max=float("inf"), sigma_theta_max=float("inf")):
        """`DeviceIO.lookahead` from the snapshot's records."""
        return _look.forecast(self, u, h, mask, sigma_r_max, sigma_theta_max)


def _mark_written(io):
    check(lib().qle_mark_state_written(io.ekf._h))


def set_state(io, x, P=None, mask=None):
    """`DeviceIO.set_state`."""
    B, n = io.batch, io.ekf.num_states
    if x is None and P is None:
        raise ValueError("x and P are both None: nothing to write")
    src = None
    if x is not None:
        src = io._check(x, "x", (B, 16))
    if P is not None:
        dn = io._check(P, "P", (B, n, n))
        if src is not None and dn != src:
            raise ValueError("x and P must have the same dtype")
        src = dn
    io._check_mask(mask)
    refuse_masked_multirate(io.ekf.params, mask, "set_state")
    S = stateio_lib()
    view = io._view()
    with io._ordered(view, x, P, mask):
        scheck(S.qsi_pack_state(C.byref(view), _ptr(x), _ptr(P), _t.FLOATS[src], _ptr(mask)))
    _mark_written(io)


def snapshot(io, with_params=False, into=None):
    """`DeviceIO.snapshot`.  into: a `Snapshot` of this handle whose workspace is written again (`gather` keeps one)."""
    S = stateio_lib()
    view = io._view()
    if with_params and not view.filter_params:
        raise QleError(QLE_ERR_STATE, "snapshot(with_params=True): no per-filter parameters are in force (set_filter_params)")
    if into is None:
        nbytes = scheck(S.qsi_workspace_bytes(C.byref(view)))
        workspace = io._alloc([(nbytes,)], "uint8")[0]
        wsz = 4 if view.dtype == QLE_F32 else 8
        params = io._alloc([(view.padded_batch * PARAM_WORDS * wsz,)], "uint8")[0] if with_params else None
    else:
        workspace, params = into.workspace, into.params
    snap = _copy_view(view)
    snap.state = workspace.data_ptr()
    if with_params:
        snap.filter_params = params.data_ptr()
    with io._ordered(view):
        scheck(S.qsi_copy(C.byref(view), C.byref(snap), None, None, int(bool(with_params)), None))
    if into is not None:
        into.view = snap
        return into
    return Snapshot(io, snap, workspace, params)


def restore(io, snap, mask=None, index=None, with_params=False):
    """`DeviceIO.restore`."""
    if not isinstance(snap, Snapshot):
        raise ValueError(f"snap: expected a Snapshot, got {type(snap).__name__}")
    B = io.batch
    for what in ("dtype", "num_states", "device"):
        if getattr(snap.ekf, what) != getattr(io.ekf, what):
            raise ValueError(f"snap: the snapshot's handle has {what} {getattr(snap.ekf, what)}, this handle {getattr(io.ekf, what)}")
    if index is None and snap.batch != B:
        raise ValueError(f"snap: a snapshot of {snap.batch} filters into a handle of {B} needs an index")
    if with_params and snap.params is None:
        raise ValueError("with_params: the snapshot was taken without its parameter records (snapshot(with_params=True))")
    if index is not None:
        io._check(index, "index", (B,), ("int32",), align=4)
    io._check_mask(mask)
    refuse_masked_multirate(io.ekf.params, mask, "restore")
    S = stateio_lib()
    view = io._view()
    written = io._alloc([(B,)], "uint8")[0] if index is not None else None
    with io._ordered(view, index, mask):
        if snap.view.stream != view.stream:   # a snapshot of another handle: this handle's stream behind the one that wrote it
            _t.dcheck(_t.devio_lib().qdv_wait_stream(C.byref(view), snap.view.stream))
        scheck(S.qsi_copy(C.byref(snap.view), C.byref(view), _ptr(index), _ptr(mask), int(bool(with_params)), _ptr(written)))
    _mark_written(io)
    return written


def gather(io, index, mask=None):
    """`DeviceIO.gather`."""
    io._check(index, "index", (io.batch,), ("int32",), align=4)
    io._check_mask(mask)
    refuse_masked_multirate(io.ekf.params, mask, "gather")
    io._gather_snap = snapshot(io, into=io._gather_snap)
    return restore(io, io._gather_snap, mask, index)


def fork_index(io, members, source=0):
    """index[i] = (i // members) * members + source as an int32 device tensor [B]."""
    B = io.batch
    for name, v in (("members", members), ("source", source)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"{name} must be an integer (got {v!r})")
    members, source = int(members), int(source)
    if members < 1 or B % members:
        raise ValueError(f"members must divide the batch of {B} (got {members})")
    if not 0 <= source < members:
        raise ValueError(f"source must be in 0..{members - 1} (got {source})")
    import torch
    i = torch.arange(B, dtype=torch.int32, device=torch.device("cuda", io.ekf.device))
    return (i // members) * members + source


def gather_host(ekf, index, mask=None):
    """`BatchedRelativePoseEKF.gather_state`: host arrays in, `written` as a numpy array out; two launches and one synchronisation."""
    import numpy as np
    B = ekf.batch
    idx = np.ascontiguousarray(index, np.int32)
    if idx.shape != (B,):
        raise ValueError(f"index: expected shape {(B,)}, got {idx.shape}")
    m = None
    if mask is not None:
        m = np.ascontiguousarray(mask, np.uint8)
        if m.shape != (B,):
            raise ValueError(f"mask: expected shape {(B,)}, got {m.shape}")
    refuse_masked_multirate(ekf.params, m, "gather_state")
    S = stateio_lib()
    view = _t.device_view(ekf)
    nbytes = scheck(S.qsi_workspace_bytes(C.byref(view)))
    workspace = _t.empty(ekf.device, (nbytes,), "uint8")
    snap = _copy_view(view)
    snap.state = workspace.data_ptr()
    written = np.empty(B, np.uint8)
    pu8 = C.POINTER(C.c_uint8)
    with _t.ordered(view, ekf.device):
        scheck(S.qsi_copy(C.byref(view), C.byref(snap), None, None, 0, None))
        scheck(S.qsi_copy_host(C.byref(snap), C.byref(view), idx.ctypes.data_as(C.POINTER(C.c_int32)), None if m is None else m.ctypes.data_as(pu8), 0,
                               written.ctypes.data_as(pu8)))
    check(lib().qle_mark_state_written(ekf._h))
    return written
