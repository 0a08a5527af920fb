"""What every binding at the device-tensor boundary shares, below all of them: the binding of include/qle_devio.h (libqle_devio.so),
the one check of a tensor argument, the ordering bracket between the handle's stream and the caller's, the one place device memory is
allocated, and `device_view`.  Imports nothing of the package but `_lib`.

A tensor is a torch tensor or anything with `data_ptr()`, `dtype`, `shape`, `device` (and optionally `is_contiguous()`).  torch is
imported lazily: only to find the caller's current stream for torch tensors and to allocate outputs.
"""
import ctypes as C
import sys

from ._lib import QleDeviceView, QleInputsView, SideLibrary, check, lib

QDV_F32, QDV_F64 = 0, 1
_vp = C.c_void_p
_pview, _pin = C.POINTER(QleDeviceView), C.POINTER(QleInputsView)
# every symbol include/qle_devio.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "qdv_last_error": (C.c_char_p, []),
    "qdv_pack_inputs": (C.c_int, [_pview, _pin, _vp, _vp, _vp, C.c_int32]),
    "qdv_unpack_state": (C.c_int, [_pview, _vp, _vp, C.c_int32]),
    "qdv_unpack_report": (C.c_int, [_pview, _vp, _vp, _vp, _vp, C.c_int32]),
    "qdv_wait_stream": (C.c_int, [_pview, _vp]),
    "qdv_signal_stream": (C.c_int, [_pview, _vp]),
    "qdv_launch_census_begin": (C.c_int, []),
    "qdv_launch_census_end": (C.c_int, [C.c_char_p, C.c_int64, C.POINTER(C.c_int64)]),
}
DEVIO = SideLibrary("devio", "QLE_DEVIO_LIB", SYMBOLS, "the device-tensor boundary", "qdv_last_error")
devio_lib, dcheck = DEVIO.load, DEVIO.check

FLOATS = {"float32": QDV_F32, "float64": QDV_F64}
MASKS = ("uint8", "bool")


def dtype_name(t):
    return str(t.dtype).rsplit(".", 1)[-1]


def device_index(t):
    """(type, index) of a tensor's device: torch.device, or a string such as 'cuda:1'."""
    d = t.device
    kind = getattr(d, "type", None)
    if kind is not None:
        idx = getattr(d, "index", None)
    else:
        kind, _, idx = str(d).partition(":")
        idx = int(idx) if idx else None
    return kind, (0 if idx is None else int(idx))


def is_torch(t):
    return type(t).__module__.split(".")[0] == "torch"


def check_tensor(t, name, shape, dtypes, device, align=16):
    """The one argument check (before any GPU call): t is a device tensor on GPU `device` of one of `dtypes` and of `shape`,
    contiguous, its storage aligned to `align` bytes (None: no rule, as for masks).  Returns the dtype's name."""
    for attr in ("data_ptr", "dtype", "shape", "device"):
        if not hasattr(t, attr):
            raise ValueError(f"{name}: expected a device tensor (data_ptr(), dtype, shape, device), got {type(t).__name__}")
    kind, idx = device_index(t)
    if kind not in ("cuda", "hip") or idx != device:
        raise ValueError(f"{name}: tensor is on {t.device}, the filter handle is on GPU {device}")
    dn = dtype_name(t)
    if dn not in dtypes:
        raise ValueError(f"{name}: dtype {t.dtype} not supported, expected one of {tuple(dtypes)}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    if hasattr(t, "is_contiguous") and not t.is_contiguous():
        raise ValueError(f"{name}: tensor must be contiguous")
    if align and t.data_ptr() % align != 0:
        raise ValueError(f"{name}: tensor storage must be {align}-byte aligned")
    return dn


def out_dtype(dtype, default):
    """The name of an output dtype: `default` for None, else float32 or float64 by name or torch dtype."""
    if dtype is None:
        return default
    dn = str(dtype).rsplit(".", 1)[-1]
    if dn not in FLOATS:
        raise ValueError(f"dtype {dtype} not supported, expected float32 or float64")
    return dn


def current_stream(device, *tensors):
    """hipStream_t of the caller's current stream on GPU `device` (torch's, when torch is in use), else the default stream."""
    if any(is_torch(t) for t in tensors if t is not None) or "torch" in sys.modules:
        import torch
        return int(torch.cuda.current_stream(device).cuda_stream)
    return 0


class ordered:
    """What the block queues on the view's stream runs behind the caller's current stream, and that stream goes on behind it
    (qdv_wait_stream ... qdv_signal_stream).  A call that raises in the block ends the bracket there: nothing is signalled."""

    def __init__(self, view, device, *tensors):
        self.view, self.stream = view, current_stream(device, *tensors)

    def __enter__(self):
        dcheck(devio_lib().qdv_wait_stream(C.byref(self.view), self.stream))

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            dcheck(devio_lib().qdv_signal_stream(C.byref(self.view), self.stream))


def empty(device, shape, dn, zero=False):
    """A fresh tensor of dtype `dn` (a name such as "float64") on GPU `device`, zeroed where asked: the one place the package's
    device-tensor boundary allocates device memory."""
    import torch
    make = torch.zeros if zero else torch.empty
    return make(shape, dtype=getattr(torch, dn), device=torch.device("cuda", device))


def device_view(ekf):
    """The `qle_device_view` of a handle: where its records live in GPU memory."""
    v = QleDeviceView()
    v.struct_size = C.sizeof(QleDeviceView)
    check(lib().qle_get_device_view(ekf._h, C.byref(v)))
    return v
