"""The read-only consumers of a `qle_device_view`: `state`, `report`, `health`, `nees`, `budget`, once, for every view they are read from.

`DeviceRecords` is what a handle's records, a forecast of them and a fused estimate of them have in common: the handle they descend
from (parameters, device, dtype, num_states -- read, never written), a batch, and a `_view()` the subclass defines.
`devio.DeviceIO` takes its view from `qle_get_device_view` and adds everything that packs inputs or writes the handle;
`ViewRecords` holds a fixed view (and the workspace tensor its records live in): `lookahead.Forecast` and `bank.Fused` are such.
"""
import ctypes as C

from . import _tensors as _t
from . import budget as _budget
from . import consistency as _cons
from . import health as _health
from ._lib import QLE_F32

REPORT = (("pose", (7,)), ("pose_cov", (6, 6)), ("vel", (3,)), ("bias", (6,)))


class DeviceRecords:
    _REPORT = REPORT

    def __init__(self, ekf, batch):
        self.ekf = ekf       # the handle: its parameters, device, dtype and num_states are read here, it is never written
        self.batch = batch   # filters in the view (the handle's, or the banks of a fused view)

    def _view(self):
        raise NotImplementedError

    # ---- argument checks (before any GPU call), outputs, ordering: _tensors, for this handle's device
    def _check(self, t, name, shape, dtypes=_t.FLOATS, align=16):
        return _t.check_tensor(t, name, shape, dtypes, self.ekf.device, align)

    def _check_mask(self, mask):
        """mask [B] (uint8 / bool), or None (all): no alignment rule."""
        if mask is not None:
            self._check(mask, "mask", (self.batch,), _t.MASKS, align=None)

    def _out_dtype(self, dtype):
        return _t.out_dtype(dtype, "float32" if self.ekf.dtype == QLE_F32 else "float64")

    def _alloc(self, shapes, dn):
        return [_t.empty(self.ekf.device, s, dn) for s in shapes]

    def _ordered(self, view, *tensors):
        return _t.ordered(view, self.ekf.device, *tensors)

    # ---- outputs as device tensors
    def state(self, dtype=None, out=None):
        """(x [B,16], P [B,n,n]) as device tensors: `get_state()` without the host.  out = (x, P) fills given tensors.  On a forecast
        or a fused view: its records (B = the view's batch); a skipped filter's or an empty bank's rows are zero."""
        B, n = self.batch, self.ekf.num_states
        if out is None:
            dn = self._out_dtype(dtype)
            x, P = self._alloc([(B, 16), (B, n, n)], dn)
        else:
            x, P = out
            dn = self._check(x, "x", (B, 16))
            if self._check(P, "P", (B, n, n)) != dn or (dtype is not None and self._out_dtype(dtype) != dn):
                raise ValueError("x, P and dtype must agree")
        D = _t.devio_lib()
        view = self._view()
        with self._ordered(view, x, P):
            _t.dcheck(D.qdv_unpack_state(C.byref(view), x.data_ptr(), P.data_ptr(), _t.FLOATS[dn]))
        return x, P

    def report(self, dtype=None, out=None):
        """What the node publishes after a tick (relative_pose_EKF_node.cpp:192-220) as device tensors: the dict of
        `BatchedRelativePoseEKF.report()`.  out = a dict with any of its keys fills those tensors only.  On a forecast: what the node
        would publish at the horizon; on a fused view: for every bank."""
        B = self.batch
        if out is None:
            dn = self._out_dtype(dtype)
            out = dict(zip((k for k, _ in REPORT), self._alloc([(B,) + s for _, s in REPORT], dn)))
        else:
            if not out or set(out) - {k for k, _ in REPORT}:
                raise ValueError(f"out: expected a dict with keys among {[k for k, _ in REPORT]}")
            dns = {self._check(out[k], k, (B,) + s) for k, s in REPORT if k in out}
            if len(dns) != 1 or (dtype is not None and self._out_dtype(dtype) not in dns):
                raise ValueError("the tensors of out and dtype must agree")
            dn = dns.pop()
        D = _t.devio_lib()
        view = self._view()
        ptr = [out[k].data_ptr() if k in out else None for k, _ in REPORT]
        with self._ordered(view, *out.values()):
            _t.dcheck(D.qdv_unpack_report(C.byref(view), ptr[0], ptr[1], ptr[2], ptr[3], _t.FLOATS[dn]))
        return out

    # ---- filter health
    def health(self, mask=None, sigma_r_max=float("inf"), sigma_v_max=float("inf"), sigma_theta_max=float("inf"), qnorm_tol=1e-3,
               select=None, return_summary=False):
        """Classify every filter in one read-only launch.  Returns (status, flagged), uint8 device tensors [B], or with
        return_summary=True (status, flagged, summary) with the nine float64 counts of health.SUMMARY_FIELDS (evaluated, flagged,
        uninitialised, then one count per status bit) as a device tensor.  status holds the bits of health.BITS for an initialised
        filter with mask != 0 (None = all) and 0 otherwise: NONFINITE (any record word NaN or Inf; nothing else is evaluated then),
        NOT_PD (a pivot of the L D L^T of P is <= 0), QNORM (|q.q - 1| > qnorm_tol), SIGMA_R / SIGMA_V / SIGMA_THETA (the largest
        variance of the block is above the limit squared; inf = no limit).  flagged = (status & select) != 0, select: None (every
        bit), names such as "nonfinite+not_pd", or the bit mask.  `flagged` is a mask for `retire`.  Asynchronous, no
        synchronisation, deterministic; changes nothing.  On a forecast: which filters will be flagged at the horizon; skipped
        filters and empty banks are uninitialised to it."""
        B = self.batch
        self._check_mask(mask)
        lim = _health.make_limits(sigma_r_max, sigma_v_max, sigma_theta_max, qnorm_tol, select)
        H = _health.health_lib()
        view = self._view()
        status, flagged = self._alloc([(B,), (B,)], "uint8")
        summary = self._alloc([(len(_health.SUMMARY_FIELDS),)], "float64")[0] if return_summary else None
        with self._ordered(view, mask):
            _health.hcheck(H.qhl_health(C.byref(view), C.byref(lim), None if mask is None else mask.data_ptr(), status.data_ptr(),
                                        flagged.data_ptr(), None if summary is None else summary.data_ptr()))
        return (status, flagged, summary) if return_summary else (status, flagged)

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
        counted in n_not_pd.  On a forecast: against a truth at the horizon; on a fused view: x_true [G,16], with the static biases
        of the handle's shared parameters."""
        B, n = self.batch, self.ekf.num_states
        src = self._check(x_true, "x_true", (B, 16))
        self._check_mask(mask)
        bits = _cons.block_mask(blocks, n)
        chi2_hi = _cons.check_chi2_hi(chi2_hi)
        dn = self._out_dtype(dtype)
        K = _cons.consistency_lib()
        view = self._view()
        nees = self._alloc([(B,)], dn)[0]
        err = self._alloc([(B, n)], dn)[0] if return_err else None
        summary = self._alloc([(8,)], "float64")[0]
        with self._ordered(view, x_true, mask):
            _cons.ccheck(K.qcs_nees(C.byref(view), C.byref(self.ekf.params), x_true.data_ptr(), _t.FLOATS[src],
                                    None if mask is None else mask.data_ptr(), bits, chi2_hi, nees.data_ptr(),
                                    None if err is None else err.data_ptr(), summary.data_ptr(), _t.FLOATS[dn]))
        return (nees, err, summary) if return_err else (nees, summary)

    # ---- the per-component error budget against a truth
    def budget(self, x_true, mask=None, group_tiles=None, return_err=False, return_status=False, dtype=None, out=None):
        """The error budget of the batch against x_true, per group of filters: a `budget.Budget` over sums [G,256] (float64 device
        tensor: the count, sum e, sum e e^T and sum P of include/qle_budget.h), from which it derives mean, mse, cov, P_mean, var_ratio,
        rms and sigma on the device.  e is the error of `nees`; x_true is [B,16] (float32 or float64), or [16] / [1,16]: one reference
        row for every filter, the dispersion of the ensemble about a common point.  mask [B] (uint8 / bool; None = all).
        group_tiles: a group is that many consecutive 64-filter tiles, G = ceil(ceil(B / 64) / group_tiles); None or 0 = one group.
        A filter is counted when its mask is not 0, it has a state and its error and covariance are finite.  return_err: the
        Budget's `err` [B,n] (dtype: None = the handle's) holds e, 0 where the filter is off; return_status: its `status` [B] (uint8)
        holds 0 off, 1 counted, 2 on but not finite.  out: a float64 device tensor [G,256] the sums are written to, for example a
        slice of a [J,G,256] buffer.  Two read-only launches; asynchronous, no synchronisation, deterministic to the bit, and additive:
        the sums of shards that are whole groups are the groups' sums of the whole batch.  Works on a forecast, a snapshot and a
        fused view (x_true [G,16] there) as `nees` does."""
        B, n = self.batch, self.ekf.num_states
        shape = tuple(getattr(x_true, "shape", ()))
        rows = 1 if shape in ((16,), (1, 16)) else B
        src = self._check(x_true, "x_true", shape if rows == 1 else (B, 16))
        self._check_mask(mask)
        gt, G = _budget.groups(B, group_tiles)
        dn = self._out_dtype(dtype)
        if out is not None:
            self._check(out, "out", (G, _budget.WORDS), ("float64",), align=8)
        K = _budget.budget_lib()
        view = self._view()
        sums = self._alloc([(G, _budget.WORDS)], "float64")[0] if out is None else out
        err = self._alloc([(B, n)], dn)[0] if return_err else None
        status = self._alloc([(B,)], "uint8")[0] if return_status else None
        with self._ordered(view, x_true, mask, out):
            _budget.bcheck(K.qbg_budget(C.byref(view), C.byref(self.ekf.params), x_true.data_ptr(), _t.FLOATS[src], rows,
                                        None if mask is None else mask.data_ptr(), gt, sums.data_ptr(),
                                        None if err is None else err.data_ptr(), _t.FLOATS[dn], None if status is None else status.data_ptr()))
        return _budget.Budget(sums, err, status)


class ViewRecords(DeviceRecords):
    """Records behind a fixed `qle_device_view` that is not a handle's: `view`, and `workspace`, the tensor they live in."""

    def __init__(self, ekf, batch, view, workspace):
        super().__init__(ekf, batch)
        self.view, self.workspace = view, workspace

    def _view(self):
        return self.view
