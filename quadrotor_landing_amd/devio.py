"""Device-tensor boundary: tick a `BatchedRelativePoseEKF` from tensors that already live in GPU memory.

`DeviceIO(ekf)` packs AoS tensors on the handle's GPU (float32 or float64) straight into the wave-tile records the tick
kernels read, runs the existing tick (`qle_run` over a private two-tick sequence, so every mode it serves is covered:
explicit masks, the device decision logic of `enable_gating`, multirate with a fixed or uniform-age delay), and returns
state and report as device tensors.  No host copy and no synchronisation on the way: the work is ordered by HIP events
between the handle's stream and the caller's current stream (include/qle_devio.h, libqle_devio.so).

A tensor is a torch tensor or anything with `data_ptr()`, `dtype`, `shape`, `device` (and optionally `is_contiguous()`).
torch is imported lazily: only to find the caller's current stream for torch tensors and to allocate outputs.

The chi-square gate runs from device tensors too: `tick(u, z, mask, chi2_max=...)` puts one read-only kernel (gate.py,
libqle_gate.so) in front of the unchanged tick, and `innovation(z)` returns nu, S and NIS as device tensors.  The host-array
`step_gated` / `update_gated` of `BatchedRelativePoseEKF` stay as they are (three launches per gated tick).

Filter consistency against a truth that lives on the GPU: `nees(x_true, ...)` returns every filter's normalised estimation error
squared e^T P^-1 e and an eight-double batch summary as device tensors (consistency.py, libqle_consistency.so: two read-only kernels,
no synchronisation).

Filter lifecycle from device tensors (health.py, libqle_health.so, and qle_initialize_state_slot of the tick library):
`seed(z, mask)` seeds filters from tag poses on the GPU, `health(...)` classifies every filter in one read-only launch (non-finite,
not positive definite, quaternion norm, sigma limits), `retire(mask)` makes filters "uninitialised" so that ticks skip them, and
`reseed(z, mask)` seeds the flagged filters that have a detection.  No host copy, no synchronisation; multirate handles included.

Look-ahead (lookahead.py, libqle_lookahead.so): `lookahead(u, h)` returns a `Forecast` -- state and covariance h ticks ahead with the
IMU sample held, computed in one read-only launch into a workspace of its own and readable through the same calls (`state`, `report`,
`health`, `nees`, `lookahead` again), with the coast budget `ticks_to_limit` when a sigma limit is given.

A whole tensor sequence per call (sequence.py, libqle_sequence.so): `sequence(u_seq, z_seq, meas_ticks, mask_seq)` packs K ticks of
tensors into a `DeviceSequence` with ceil(K / 32) launches, and `run(seq, ...)` runs them from one C loop -- with the gate, a report
trace and a NEES trace every so many ticks where asked -- instead of K Python calls of `tick`; the bits are those of the `tick` loop.

Innovation scoring for noise sweeps (score.py, libqle_score.so): `scorer()` returns a `Scorer` whose `observe(u, z, mask)` in front of a
`tick`, or `run(seq)` in place of `run`, accumulates every filter's innovation log-likelihood and per-component consistency statistics
on the GPU -- one read-only launch per tag tick, the ticks themselves unchanged.

Filter banks (bank.py, libqle_bank.so): `bank(M)` reads the handle as B / M banks of M consecutive filters, and `Bank.fuse(logw)` returns
a `Fused` -- the members' posterior weights and every bank's moment-matched estimate, computed in one read-only launch into a workspace
of its own and readable through the same calls (`state`, `report`, `health`, `nees`).

Still host-fed through `BatchedRelativePoseEKF`: `set_state` and the per-filter stamps of `dynamic_meas_delay`
(`filter_update(t_curr=..., apriltag_time=...)`).
"""
import contextlib
import ctypes as C
import os
import sys

from . import bank as _bank
from . import consistency as _cons
from . import gate as _gate
from . import health as _health
from . import lookahead as _look
from . import score as _score
from . import sequence as _seqm
from ._lib import QLE_ERR_STATE, QLE_F32, QleDeviceView, QleInputsView, QleError, check, lib, load_side_library

_HERE = os.path.dirname(os.path.abspath(__file__))
DEVIO_LIB_PATH = os.environ.get("QLE_DEVIO_LIB") or os.path.join(_HERE, "libqle_devio.so")

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
}

_dlib = None


def devio_lib():
    """Load libqle_devio.so; raises (never falls back) when it is missing."""
    global _dlib
    if _dlib is None:
        _dlib = load_side_library(DEVIO_LIB_PATH, SYMBOLS, "the device-tensor boundary", needs_tick_library=False)
    return _dlib


def _dcheck(rc):
    if rc != 0:
        raise QleError(rc, devio_lib().qdv_last_error().decode())


_FLOATS = {"float32": QDV_F32, "float64": QDV_F64}
_MASKS = ("uint8", "bool")


def _dtype_name(t):
    return str(t.dtype).rsplit(".", 1)[-1]


def _device_index(t):
    """(type, index) of a tensor's device: torch.device, or a string such as 'cuda:1'."""
    d = t.device
    kind = getattr(d, "type", None)
    if kind is not None:
        idx = getattr(d, "index", None)
    else:
        kind, _, idx = str(d).partition(":")
        idx = int(idx) if idx else None
    return kind, (0 if idx is None else int(idx))


def _is_torch(t):
    return type(t).__module__.split(".")[0] == "torch"


class DeviceIO:
    def __init__(self, ekf):
        self.ekf = ekf
        self._float = QDV_F32 if ekf.dtype == QLE_F32 else QDV_F64
        self._seq = None   # two ticks: 0 without a tag slot, 1 with one (made on the first tick)
        self._zero_u = {}  # innovation(): an all-zero IMU tensor per source dtype for the pack

    # ---- argument checks (before any GPU call)
    def _check(self, t, name, shape, dtypes):
        for attr in ("data_ptr", "dtype", "shape", "device"):
            if not hasattr(t, attr):
                raise ValueError(f"{name}: expected a device tensor (data_ptr(), dtype, shape, device), got {type(t).__name__}")
        kind, idx = _device_index(t)
        if kind not in ("cuda", "hip") or idx != self.ekf.device:
            raise ValueError(f"{name}: tensor is on {t.device}, the filter handle is on GPU {self.ekf.device}")
        dn = _dtype_name(t)
        if dn not in dtypes:
            raise ValueError(f"{name}: dtype {t.dtype} not supported, expected one of {tuple(dtypes)}")
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
        if hasattr(t, "is_contiguous") and not t.is_contiguous():
            raise ValueError(f"{name}: tensor must be contiguous")
        if t.data_ptr() % 16 != 0:
            raise ValueError(f"{name}: tensor storage must be 16-byte aligned")
        return dn

    def _current_stream(self, *tensors):
        """hipStream_t of the caller's current stream on the handle's device (torch's, when torch is in use), else the default stream."""
        if any(_is_torch(t) for t in tensors if t is not None) or "torch" in sys.modules:
            import torch
            return int(torch.cuda.current_stream(self.ekf.device).cuda_stream)
        return 0

    @contextlib.contextmanager
    def _ordered(self, D, view, *tensors):
        """What the block queues on the handle's stream runs behind the caller's current stream, and that stream goes on behind it
        (qdv_wait_stream ... qdv_signal_stream).  A call that raises in the block ends the bracket there: nothing is signalled."""
        stream = self._current_stream(*tensors)
        _dcheck(D.qdv_wait_stream(C.byref(view), stream))
        yield
        _dcheck(D.qdv_signal_stream(C.byref(view), stream))

    def _view(self):
        v = QleDeviceView()
        v.struct_size = C.sizeof(QleDeviceView)
        check(lib().qle_get_device_view(self.ekf._h, C.byref(v)))
        return v

    def _inputs_view(self, t):
        if self._seq is None:
            self._seq = self.ekf.make_inputs(2, [0, 1])
        iv = QleInputsView()
        iv.struct_size = C.sizeof(QleInputsView)
        check(lib().qle_inputs_get_device_view(self._seq._h, t, C.byref(iv)))
        return iv

    # ---- one tick from device tensors
    def tick(self, u, z=None, mask=None, chi2_max=None, return_nis=False):
        """One filter tick: u [B,6] and, on a tick with tag poses, z [B,7] and mask [B] (uint8 / bool; None = all), what
        `step(u, z, mask)` means on the host path (with `enable_gating`: what `filter_update` means).  Asynchronous; the
        tensors may be reused as soon as the call returns (the caller's current stream is ordered behind the pack).

        chi2_max (> 0; inf accepts every finite NIS): a chi-square gate in front of the tick.  One more launch (k_pregate) between
        the pack and the tick evaluates NIS = delta_y^T S^-1 delta_y of every tag pose against the predicted state and clears the
        mask where it exceeds chi2_max; the unchanged tick then applies exactly the accepted corrections (with `enable_gating`:
        a rejected tag pose is no detection -- not consumed, no reset of the rate limiter).  Returns `accepted` [B] (uint8) as a
        device tensor; with return_nis=True returns (accepted, nis [B], nu [B,6], S [B,6,6]) in the handle's compute dtype.  A
        masked or uninitialised filter, or one whose S is not positive definite: not accepted, NIS = NaN.  Refused with
        multirate_ekf."""
        B = self.ekf.batch
        src = self._check(u, "u", (B, 6), _FLOATS)
        if z is not None and self._check(z, "z", (B, 7), _FLOATS) != src:
            raise ValueError("u and z must have the same dtype")
        if mask is not None:
            if z is None:
                raise ValueError("mask given without z")
            self._check_mask(mask, B)
        if chi2_max is None:
            if return_nis:
                raise ValueError("return_nis given without chi2_max")
        else:
            chi2_max = self._check_gate(z, chi2_max)
        D = devio_lib()
        view = self._view()
        t = 0 if z is None else 1
        iv = self._inputs_view(t)
        out = None
        if chi2_max is not None:
            G = _gate.gate_lib()
            dn = self._out_dtype(None)
            accepted = self._alloc([(B,)], "uint8")[0]
            out = [accepted] + (self._alloc([(B,), (B, 6), (B, 6, 6)], dn) if return_nis else [None, None, None])
        with self._ordered(D, view, u, z, mask):
            _dcheck(D.qdv_pack_inputs(C.byref(view), C.byref(iv), u.data_ptr(), None if z is None else z.data_ptr(),
                                      None if mask is None else mask.data_ptr(), _FLOATS[src]))
            if out is not None:
                ptr = [None if o is None else o.data_ptr() for o in out]
                _gate.gcheck(G.qgt_gate_tick(C.byref(view), C.byref(iv), C.byref(self.ekf.params), chi2_max, ptr[1], ptr[0], ptr[2], ptr[3],
                                             _FLOATS[dn]))
        check(lib().qle_run(self.ekf._h, self._seq._h, t, 1))
        if out is not None:
            return tuple(out) if return_nis else out[0]

    def _check_gate(self, z, chi2_max):
        """The gate's own refusals (before any GPU call): a tick without tag poses, a threshold that is not > 0, multirate_ekf."""
        if z is None:
            raise ValueError("chi2_max given on a tick without tag poses (z is None)")
        chi2_max = float(chi2_max)
        if not chi2_max > 0.0:
            raise ValueError(f"chi2_max must be > 0 (got {chi2_max})")
        self._refuse_multirate()
        return chi2_max

    def _refuse_multirate(self):
        if self.ekf.params.multirate_ekf:
            raise QleError(QLE_ERR_STATE, "the gate does not support multirate_ekf: a delayed measurement's innovation belongs to a history entry")

    def innovation(self, z, mask=None, dtype=None):
        """(nu [B,6], S [B,6,6], nis [B]) of tag poses z [B,7] against the stored state as device tensors: `innovation(z, mask)` of the
        host path without the host.  Changes nothing.  Filters with mask 0 or without state: nu = 0, S = 0, nis = NaN.
        (The pack always moves an IMU record, so an all-zero one is kept per source dtype; a pack entry that takes u = NULL is a
        follow-up for include/qle_devio.h.)"""
        B = self.ekf.batch
        src = self._check(z, "z", (B, 7), _FLOATS)
        if mask is not None:
            self._check_mask(mask, B)
        dn = self._out_dtype(dtype)
        self._refuse_multirate()
        D, G = devio_lib(), _gate.gate_lib()
        view = self._view()
        iv = self._inputs_view(1)
        zero_u = self._zeros_u(src)
        nu, S, nis = self._alloc([(B, 6), (B, 6, 6), (B,)], dn)
        with self._ordered(D, view, z, mask):
            _dcheck(D.qdv_pack_inputs(C.byref(view), C.byref(iv), zero_u.data_ptr(), z.data_ptr(),
                                      None if mask is None else mask.data_ptr(), _FLOATS[src]))
            _gate.gcheck(G.qgt_innovation(C.byref(view), C.byref(iv), C.byref(self.ekf.params), nis.data_ptr(), nu.data_ptr(), S.data_ptr(),
                                          _FLOATS[dn]))
        return nu, S, nis

    # ---- filter consistency against a truth
    def nees(self, x_true, mask=None, blocks="all", chi2_hi=float("inf"), return_err=False, dtype=None):
        """NEES = e^T P^-1 e of every filter against x_true [B,16] (r, v, q xyzw, ab, wb: the layout of the state, with the total true
        biases; float32 or float64), e = truth minus estimate in the filter's error-state convention (include/qle_consistency.h).
        blocks: the marginal NEES is taken over -- "all", names such as "pose" (= r + theta), "r", "r+theta+ab+wb", or the bit mask
        (bit 0 r, 1 v, 2 theta, 3 ab, 4 wb); dof = 3 x the number of blocks.  mask [B] (uint8 / bool; None = all).
        Returns (nees [B], summary) or, with return_err=True, (nees, err [B,n], summary) as device tensors; summary is 8 float64
        values in the order of consistency.SUMMARY_FIELDS (count, sum_nees, sum_nees_sq, n_above = count with nees > chi2_hi,
        n_not_pd, sum_r_err_sq, sum_theta_err_sq, dof).  Asynchronous, no synchronisation, deterministic; changes nothing.  A filter
        with mask 0 or without state: nees = NaN, err = 0, not counted; a covariance that is not positive definite: nees = NaN,
        counted in n_not_pd."""
        B, n = self.ekf.batch, self.ekf.num_states
        src = self._check(x_true, "x_true", (B, 16), _FLOATS)
        if mask is not None:
            self._check_mask(mask, B)
        bits = _cons.block_mask(blocks, n)
        chi2_hi = _cons.check_chi2_hi(chi2_hi)
        dn = self._out_dtype(dtype)
        D, K = devio_lib(), _cons.consistency_lib()
        view = self._view()
        nees = self._alloc([(B,)], dn)[0]
        err = self._alloc([(B, n)], dn)[0] if return_err else None
        summary = self._alloc([(8,)], "float64")[0]
        with self._ordered(D, view, x_true, mask):
            _cons.ccheck(K.qcs_nees(C.byref(view), C.byref(self.ekf.params), x_true.data_ptr(), _FLOATS[src],
                                    None if mask is None else mask.data_ptr(), bits, chi2_hi, nees.data_ptr(),
                                    None if err is None else err.data_ptr(), summary.data_ptr(), _FLOATS[dn]))
        return (nees, err, summary) if return_err else (nees, summary)

    def _zeros_u(self, src):
        """The pack always moves an IMU record too: an all-zero one per source dtype (the slot is private and every tick packs its own)."""
        if self._zero_u.get(src) is None:
            import torch
            self._zero_u[src] = torch.zeros((self.ekf.batch, 6), dtype=getattr(torch, src), device=torch.device("cuda", self.ekf.device))
        return self._zero_u[src]

    # ---- filter lifecycle: seed, health check, retire, reseed
    def seed(self, z, mask=None, reinit_bias=False):
        """`initialize_state(z, reinit_bias, mask)` of the host path from device tensors: seeds the filters with mask != 0 (None = all)
        from their tag poses z [B,7] (float32 or float64), bit for bit what `qle_initialize_state_masked` writes for the same values.
        Works on a handle that was never seeded from the host.  Asynchronous; the tensors may be reused as soon as the call returns."""
        B = self.ekf.batch
        src = self._check(z, "z", (B, 7), _FLOATS)
        if mask is not None:
            self._check_mask(mask, B)
        D = devio_lib()
        view = self._view()
        iv = self._inputs_view(1)
        zero_u = self._zeros_u(src)
        with self._ordered(D, view, z, mask):
            self._seed_from_slot(D, view, iv, zero_u, z, mask, src, reinit_bias)

    def _seed_from_slot(self, D, view, iv, zero_u, z, mask, src, reinit_bias):
        _dcheck(D.qdv_pack_inputs(C.byref(view), C.byref(iv), zero_u.data_ptr(), z.data_ptr(), None if mask is None else mask.data_ptr(),
                                  _FLOATS[src]))
        check(lib().qle_initialize_state_slot(self.ekf._h, self._seq._h, 1, int(bool(reinit_bias))))

    def health(self, mask=None, sigma_r_max=float("inf"), sigma_v_max=float("inf"), sigma_theta_max=float("inf"), qnorm_tol=1e-3,
               select=None, return_summary=False):
        """Classify every filter in one read-only launch.  Returns (status, flagged), uint8 device tensors [B], or with
        return_summary=True (status, flagged, summary) with the nine float64 counts of health.SUMMARY_FIELDS (evaluated, flagged,
        uninitialised, then one count per status bit) as a device tensor.  status holds the bits of health.BITS for an initialised
        filter with mask != 0 (None = all) and 0 otherwise: NONFINITE (any record word NaN or Inf; nothing else is evaluated then),
        NOT_PD (a pivot of the L D L^T of P is <= 0), QNORM (|q.q - 1| > qnorm_tol), SIGMA_R / SIGMA_V / SIGMA_THETA (the largest
        variance of the block is above the limit squared; inf = no limit).  flagged = (status & select) != 0, select: None (every
        bit), names such as "nonfinite+not_pd", or the bit mask.  `flagged` is a mask for `retire`.  Asynchronous, no
        synchronisation, deterministic; changes nothing."""
        B = self.ekf.batch
        if mask is not None:
            self._check_mask(mask, B)
        lim = _health.make_limits(sigma_r_max, sigma_v_max, sigma_theta_max, qnorm_tol, select)
        D, H = devio_lib(), _health.health_lib()
        view = self._view()
        status, flagged = self._alloc([(B,), (B,)], "uint8")
        summary = self._alloc([(len(_health.SUMMARY_FIELDS),)], "float64")[0] if return_summary else None
        with self._ordered(D, view, mask):
            _health.hcheck(H.qhl_health(C.byref(view), C.byref(lim), None if mask is None else mask.data_ptr(), status.data_ptr(),
                                        flagged.data_ptr(), None if summary is None else summary.data_ptr()))
        return (status, flagged, summary) if return_summary else (status, flagged)

    def retire(self, mask):
        """The filters with mask != 0 lose their state: they become "uninitialised" (their record is zeroed), every tick leaves them
        untouched and a later `seed` treats them as fresh (upds_since_correction = 0, a one-entry multirate history).  One launch,
        asynchronous."""
        self._check_mask(mask, self.ekf.batch)
        D, H = devio_lib(), _health.health_lib()
        view = self._view()
        with self._ordered(D, view, mask):
            _health.hcheck(H.qhl_retire(C.byref(view), mask.data_ptr()))

    def reseed(self, z, mask=None, reinit_bias=True, **limits):
        """Health check, then seed the flagged filters that have a detection: `health(**limits)` over every filter, reseeded =
        flagged AND mask (mask: the filters z holds a tag pose for; None = all), `seed(z, reseeded, reinit_bias)`.  Returns
        (status, reseeded), uint8 device tensors.  A flagged filter without a detection stays as it is (and stays flagged):
        `retire` it to keep it out of the ticks.

        reinit_bias defaults to True here, unlike `seed`: seeding keeps the bias words of x unless asked to zero them
        (relative_pose_EKF.cpp:317-321), so a NaN bias -- the usual company of a diverged filter -- would survive the reseed and
        break the filter again on its next tick."""
        B = self.ekf.batch
        src = self._check(z, "z", (B, 7), _FLOATS)
        if mask is not None:
            self._check_mask(mask, B)
        unknown = set(limits) - {"sigma_r_max", "sigma_v_max", "sigma_theta_max", "qnorm_tol", "select"}
        if unknown:
            raise ValueError(f"reseed: unknown limits {sorted(unknown)}")
        lim = _health.make_limits(**limits)
        D, H = devio_lib(), _health.health_lib()
        view = self._view()
        iv = self._inputs_view(1)
        zero_u = self._zeros_u(src)
        status, reseeded = self._alloc([(B,), (B,)], "uint8")
        with self._ordered(D, view, z, mask):
            _health.hcheck(H.qhl_health(C.byref(view), C.byref(lim), None, status.data_ptr(), reseeded.data_ptr(), None))
            if mask is not None:
                _health.hcheck(H.qhl_and_masks(C.byref(view), reseeded.data_ptr(), mask.data_ptr(), reseeded.data_ptr()))
            self._seed_from_slot(D, view, iv, zero_u, z, reseeded, src, reinit_bias)
        return status, reseeded

    # ---- a whole tensor sequence per call
    def _check_sequence(self, u_seq, z_seq, mask_seq, n_ticks, meas_ticks, t0):
        """The argument checks of `sequence` / `DeviceSequence.pack` (before any GPU call).  Returns (source dtype name, n).
        n_ticks None: the sequence is as long as u_seq."""
        B = self.ekf.batch
        shape = tuple(getattr(u_seq, "shape", ()))
        if len(shape) != 3 or shape[0] < 1:
            raise ValueError(f"u_seq: expected shape (K, {B}, 6) with K >= 1, got {shape}")
        n = int(shape[0])
        src = self._check(u_seq, "u_seq", (n, B, 6), _FLOATS)
        if n_ticks is None:
            n_ticks = n
        t0 = int(t0)
        if t0 < 0 or t0 + n > n_ticks:
            raise ValueError(f"ticks [{t0}, {t0 + n}) reach beyond the sequence of {n_ticks} ticks")
        ticks = _seqm.check_meas_ticks(meas_ticks, n_ticks)
        m = sum(1 for t in ticks if t0 <= t < t0 + n)
        if z_seq is None:
            if mask_seq is not None:
                raise ValueError("mask_seq given without z_seq")
            if m > 0:
                raise ValueError(f"{m} ticks of the range have a tag slot (meas_ticks) but z_seq is None")
        else:
            if m == 0:
                raise ValueError("z_seq given but no tick of the range has a tag slot (meas_ticks)")
            if self._check(z_seq, "z_seq", (m, B, 7), _FLOATS) != src:
                raise ValueError("u_seq and z_seq must have the same dtype")
            if mask_seq is not None:
                self._check_mask(mask_seq, B, "mask_seq", (m, B))
                if mask_seq.data_ptr() % 16 != 0:
                    raise ValueError("mask_seq: tensor storage must be 16-byte aligned")
        return src, n

    def sequence(self, u_seq, z_seq=None, meas_ticks=None, mask_seq=None):
        """K ticks of tensors -> a `sequence.DeviceSequence`: u_seq [K,B,6]; meas_ticks, a host list of the M strictly increasing tick
        indices in [0, K) that carry a tag pose; z_seq [M,B,7] and mask_seq [M,B] (uint8 / bool; None = all) for those ticks, in tick
        order (float32 or float64, u_seq and z_seq alike).  Creates the K-tick sequence and packs it with ONE call (ceil(K / 32)
        launches of k_sq_pack instead of K packs).  Asynchronous; the tensors may be reused as soon as the call returns."""
        src, n = self._check_sequence(u_seq, z_seq, mask_seq, None, meas_ticks, 0)
        seq = _seqm.DeviceSequence(self, n, _seqm.check_meas_ticks(meas_ticks, n))
        try:
            return seq.pack(u_seq, z_seq, mask_seq)
        except Exception:
            seq.close()
            raise

    def run(self, seq, t0=0, n=None, chi2_max=None, return_nis=False, trace_every=None, trace=("report",), x_true_seq=None, blocks="all",
            chi2_hi=float("inf"), dtype=None):
        """Ticks [t0, t0 + n) of a `DeviceSequence` (n None: to its end) in ONE native call: what n calls of `tick` do, in the same
        order, from a C loop (include/qle_sequence.h), and bit for bit their results.  Works on whatever `tick` works on.

        chi2_max: the chi-square gate of `tick` in front of every tick that has a tag slot; the result then has `accepted` [m,B]
        (uint8), one slice per tag tick of the range in tick order, and with return_nis=True `nis` [m,B].  Refused with multirate_ekf.
        A gated run leaves the accepted masks in the sequence: running it again without a gate replays the accepted corrections.
        trace_every = e: after every e-th tick of the range the kinds named in `trace` are taken -- "report": the dict of `report()` as
        [J,B,...] tensors; "nees": `nees(x_true_seq[j], blocks=..., chi2_hi=...)` as nees [J,B] and summary [J,8], against
        x_true_seq [J,B,16] -- J = n // e slices, slice j after tick t0 + (j + 1) e - 1.  dtype: of nis, report and nees (None: the
        handle's).  Returns a `sequence.SequenceResult` of device tensors; asynchronous, no synchronisation."""
        B = self.ekf.batch
        if not isinstance(seq, _seqm.DeviceSequence) or seq.io.ekf is not self.ekf or seq.inputs is None:
            raise ValueError("seq: expected an open DeviceSequence made by this handle's DeviceIO.sequence")
        t0 = int(t0)
        n = seq.n_ticks - t0 if n is None else int(n)
        if t0 < 0 or n < 0 or t0 + n > seq.n_ticks:
            raise ValueError(f"ticks [{t0}, {t0 + n}) reach beyond the sequence of {seq.n_ticks} ticks")
        if chi2_max is None:
            if return_nis:
                raise ValueError("return_nis given without chi2_max")
        else:
            chi2_max = float(chi2_max)
            if not chi2_max > 0.0:
                raise ValueError(f"chi2_max must be > 0 (got {chi2_max})")
            self._refuse_multirate()
        kinds = (trace,) if isinstance(trace, str) else tuple(trace)
        if set(kinds) - set(_seqm.TRACE_KINDS) or not kinds:
            raise ValueError(f"trace: expected kinds out of {_seqm.TRACE_KINDS}, got {kinds}")
        if trace_every is None:
            if kinds != ("report",) or x_true_seq is not None:
                raise ValueError("trace kinds or x_true_seq given without trace_every")
            kinds, J = (), 0
        else:
            if int(trace_every) != trace_every or int(trace_every) < 1:
                raise ValueError(f"trace_every must be an integer >= 1 (got {trace_every})")
            trace_every = int(trace_every)
            J = n // trace_every
        dn = self._out_dtype(dtype)
        opts = _seqm.QsqRunOpts()
        opts.struct_size = C.sizeof(opts)
        opts.dst_dtype = _FLOATS[dn]
        opts.trace_every = trace_every or 0
        if "nees" in kinds:
            if x_true_seq is None:
                raise ValueError('trace "nees" needs x_true_seq')
            opts.true_dtype = _FLOATS[self._check(x_true_seq, "x_true_seq", (J, B, 16), _FLOATS)]
            opts.blocks = _cons.block_mask(blocks, self.ekf.num_states)
            opts.chi2_hi = _cons.check_chi2_hi(chi2_hi)
        elif x_true_seq is not None:
            raise ValueError('x_true_seq given without "nees" in trace')
        S, D = _seqm.sequence_lib(), devio_lib()
        opts.params = C.pointer(self.ekf.params)
        view = self._view()
        Bp = int(view.padded_batch)
        res = _seqm.SequenceResult()
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None   # noqa: E731
        if chi2_max is not None:
            opts.chi2_max = chi2_max
            m = seq.slots(t0, n)
            acc = self._alloc([(m, Bp)], "uint8")[0]
            nis = self._alloc([(m, Bp)], dn)[0] if return_nis else None
            opts.accepted, opts.nis = ptr(acc), ptr(nis)
            res.accepted, res.nis = acc[:, :B], None if nis is None else nis[:, :B]
        if "report" in kinds:
            bufs = self._alloc([(J, Bp) + s for _, s in self._REPORT], dn)
            opts.pose, opts.pose_cov, opts.vel, opts.bias = (ptr(b) for b in bufs)
            res.report = {k: b[:, :B] for (k, _), b in zip(self._REPORT, bufs)}
        if "nees" in kinds:
            nees, summary = self._alloc([(J, Bp)], dn)[0], self._alloc([(J, 8)], "float64")[0]
            opts.x_true_seq, opts.nees, opts.summary = ptr(x_true_seq), ptr(nees), ptr(summary)
            res.nees, res.summary = nees[:, :B], summary
            if J == 0:
                opts.true_dtype, opts.blocks, opts.chi2_hi = 0, 0, 0.0
        with self._ordered(D, view, x_true_seq):
            _seqm.scheck(S.qsq_run(self.ekf._h, seq.inputs._h, t0, n, C.byref(opts)))
        return res

    # ---- innovation scoring for noise sweeps
    def scorer(self):
        """A `score.Scorer` for this handle: it owns zeroed fp64 accumulators on the GPU, `observe(u, z, mask)` in front of a `tick` or
        `run(seq)` in place of `run` adds every tag tick's innovation to them (one read-only launch per tag tick, k_score), and
        `result()` / `summary()` read them as per-filter log-likelihood and innovation consistency statistics.  Refused with
        multirate_ekf."""
        return _score.Scorer(self)

    # ---- look-ahead: state and covariance h ticks ahead, read-only
    def lookahead(self, u, h, mask=None, sigma_r_max=float("inf"), sigma_theta_max=float("inf")):
        """The forecast h ticks ahead (0 <= h <= lookahead.MAX_HORIZON) with the IMU sample u [B,6] (float32 or float64) held: what h
        calls of `predict(u)` on a copy of the handle would leave, in ONE read-only launch -- the handle is not written.  Returns a
        `lookahead.Forecast`: it owns the records and offers `state()`, `report()`, `health(...)`, `nees(x_true, ...)` and
        `lookahead(u, h, ...)` on them.  Filters with mask 0 (uint8 / bool; None = all) or without state are skipped: their forecast
        record is all zero ("uninitialised" to every consumer).  With sigma_r_max / sigma_theta_max (> 0; inf = no limit) the
        forecast's `ticks_to_limit` [B] (int32 device tensor) is the smallest k in 0..h at which a position / attitude variance
        exceeds its limit squared -- the tick at which `health` with these limits would first set SIGMA_R or SIGMA_THETA -- or -1
        (none, or skipped).  Asynchronous, no synchronisation."""
        B = self.ekf.batch
        src = self._check(u, "u", (B, 6), _FLOATS)
        h = _look.check_horizon(h)
        if mask is not None:
            self._check_mask(mask, B)
        coast = _look.make_coast(sigma_r_max, sigma_theta_max)
        D, K = devio_lib(), _look.lookahead_lib()
        view = self._view()
        nbytes = _look.kcheck(K.qlk_workspace_bytes(C.byref(view)))
        workspace = self._alloc([(nbytes,)], "uint8")[0]
        ticks = self._alloc([(B,)], "int32")[0] if coast is not None else None
        ahead = QleDeviceView()
        with self._ordered(D, view, u, mask):
            _look.kcheck(K.qlk_lookahead(C.byref(view), C.byref(self.ekf.params), u.data_ptr(), _FLOATS[src], h,
                                         None if mask is None else mask.data_ptr(), workspace.data_ptr(), nbytes, C.byref(ahead),
                                         None if coast is None else C.byref(coast), None if ticks is None else ticks.data_ptr()))
        return _look.Forecast(self, ahead, workspace, h, ticks)

    # ---- filter banks: posterior weights and a fused estimate per bank, read-only
    def bank(self, members):
        """The handle read as B / members banks of `members` consecutive filters (a power of two in 2..bank.MAX_MEMBERS that divides B):
        a `bank.Bank`, whose `fuse(logw, mask=None)` returns a `bank.Fused` -- the members' posterior weights w_i ~ exp(logw_i) and
        every bank's moment-matched mixture, ONE read-only launch of k_bank_fuse per call.  logw: a float64 device tensor [B], or a
        `score.Scorer` (its log-likelihood).  The handle is not written; multirate handles included."""
        return _bank.Bank(self, members)

    def _check_mask(self, mask, B, name="mask", shape=None):
        shape = (B,) if shape is None else tuple(shape)
        for attr in ("data_ptr", "dtype", "shape", "device"):
            if not hasattr(mask, attr):
                raise ValueError(f"{name}: expected a device tensor, got {type(mask).__name__}")
        kind, idx = _device_index(mask)
        if kind not in ("cuda", "hip") or idx != self.ekf.device:
            raise ValueError(f"{name}: tensor is on {mask.device}, the filter handle is on GPU {self.ekf.device}")
        if _dtype_name(mask) not in _MASKS:
            raise ValueError(f"{name}: dtype {mask.dtype} not supported, expected uint8 or bool")
        if tuple(mask.shape) != shape:
            raise ValueError(f"{name}: expected shape {shape}, got {tuple(mask.shape)}")
        if hasattr(mask, "is_contiguous") and not mask.is_contiguous():
            raise ValueError(f"{name}: tensor must be contiguous")

    # ---- outputs as device tensors
    def _out_dtype(self, dtype):
        if dtype is None:
            return "float32" if self._float == QDV_F32 else "float64"
        dn = str(dtype).rsplit(".", 1)[-1]
        if dn not in _FLOATS:
            raise ValueError(f"dtype {dtype} not supported, expected float32 or float64")
        return dn

    def _alloc(self, shapes, dn):
        import torch
        dev = torch.device("cuda", self.ekf.device)
        return [torch.empty(s, dtype=getattr(torch, dn), device=dev) for s in shapes]

    def state(self, dtype=None, out=None):
        """(x [B,16], P [B,n,n]) as device tensors: `get_state()` without the host.  out = (x, P) fills given tensors."""
        B, n = self.ekf.batch, self.ekf.num_states
        if out is None:
            dn = self._out_dtype(dtype)
            x, P = self._alloc([(B, 16), (B, n, n)], dn)
        else:
            x, P = out
            dn = self._check(x, "x", (B, 16), _FLOATS)
            if self._check(P, "P", (B, n, n), _FLOATS) != dn or (dtype is not None and self._out_dtype(dtype) != dn):
                raise ValueError("x, P and dtype must agree")
        D = devio_lib()
        view = self._view()
        with self._ordered(D, view, x, P):
            _dcheck(D.qdv_unpack_state(C.byref(view), x.data_ptr(), P.data_ptr(), _FLOATS[dn]))
        return x, P

    _REPORT = (("pose", (7,)), ("pose_cov", (6, 6)), ("vel", (3,)), ("bias", (6,)))

    def report(self, dtype=None, out=None):
        """What the node publishes after a tick (relative_pose_EKF_node.cpp:192-220) as device tensors: the dict of
        `BatchedRelativePoseEKF.report()`.  out = a dict with any of its keys fills those tensors only."""
        B = self.ekf.batch
        if out is None:
            dn = self._out_dtype(dtype)
            out = dict(zip((k for k, _ in self._REPORT), self._alloc([(B,) + s for _, s in self._REPORT], dn)))
        else:
            if not out or set(out) - {k for k, _ in self._REPORT}:
                raise ValueError(f"out: expected a dict with keys among {[k for k, _ in self._REPORT]}")
            dns = {self._check(out[k], k, (B,) + s, _FLOATS) for k, s in self._REPORT if k in out}
            if len(dns) != 1 or (dtype is not None and self._out_dtype(dtype) not in dns):
                raise ValueError("the tensors of out and dtype must agree")
            dn = dns.pop()
        D = devio_lib()
        view = self._view()
        ptr = [out[k].data_ptr() if k in out else None for k, _ in self._REPORT]
        with self._ordered(D, view, *out.values()):
            _dcheck(D.qdv_unpack_report(C.byref(view), ptr[0], ptr[1], ptr[2], ptr[3], _FLOATS[dn]))
        return out

    def close(self):
        if self._seq is not None:
            self._seq.close()
            self._seq = None
