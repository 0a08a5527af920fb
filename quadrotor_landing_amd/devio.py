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

The error budget of a Monte-Carlo sweep (budget.py, libqle_budget.so): `budget(x_true, group_tiles=...)` returns per group of filters
the count, sum e, sum e e^T and sum P as 256 float64 values -- bias, error covariance and reported covariance of every state -- from
two read-only launches, deterministic to the bit and additive over shards; `budget_run(seq, x_true_seq, every)` gives it at every
e-th tick of a sequence.

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

Interacting multiple models (imm.py, libqle_imm.so): `imm(M, Pi)` returns an `Imm` over the same banks -- a Markov transition between the
modes with recursive mode probabilities `logmu`, and the mixing step that re-initialises every member from the moment-matched mixture of
its bank, in place, in one launch; `Imm.step(u, z, mask)` runs the cycle mix, score, tick, update around one tick and `Imm.fuse()` is
`bank(M).fuse(logmu)`.

Adaptive tag-pose noise (adapt.py, libqle_adapt.so): `adapter(window, gain, ...)` returns an `Adapter` whose `step(u, z, mask)` in place of
`tick`, or `run(seq)` in place of `run`, lets every filter estimate its own R_r / R_ang from its innovations -- one read-only launch per
tag tick, one launch per window that writes the six R words of the per-filter parameter records, the ticks themselves unchanged.

Device state I/O (stateio.py, libqle_stateio.so): `set_state(x, P, mask)` writes the state from device tensors, one launch, the bits of
the host `set_state`; `snapshot()` returns a `Snapshot` -- a bitwise copy of the records in a workspace of its own, readable through the
same calls (`state`, `report`, `health`, `nees`, `lookahead`); `restore(snap, mask, index)` writes it back, into this handle or another
of the same dtype and layout; `gather(index)` permutes or resamples the filters in place and `fork(members)` starts every member of a
bank from one filter.  A snapshot holds the state, not the multirate history and not the counters.

Still host-fed through `BatchedRelativePoseEKF`: the per-filter stamps of `dynamic_meas_delay`
(`filter_update(t_curr=..., apriltag_time=...)`).
"""
import ctypes as C
import math

from . import _tensors as _t
from . import adapt as _adapt
from . import bank as _bank
from . import budget as _budget
from . import gate as _gate
from . import health as _health
from . import imm as _imm
from . import lookahead as _look
from . import score as _score
from . import sequence as _seqm
from . import stateio as _sio
from ._lib import QleInputsView, check, lib
from ._tensors import DEVIO, QDV_F32, QDV_F64, SYMBOLS, devio_lib  # noqa: F401
from .records import DeviceRecords

DEVIO_LIB_PATH, _dcheck, _FLOATS = DEVIO.path, DEVIO.check, _t.FLOATS


class DeviceIO(DeviceRecords):
    """A handle's own records: the view is `qle_get_device_view`'s.  `state`, `report`, `health` and `nees` are `DeviceRecords`';
    everything here packs inputs or writes the handle."""

    def __init__(self, ekf):
        super().__init__(ekf, ekf.batch)
        self._seq = None   # two ticks: 0 without a tag slot, 1 with one (made on the first tick)
        self._zero_u = {}  # innovation(): an all-zero IMU tensor per source dtype for the pack
        self._gather_snap = None   # gather(): the snapshot an in-place permutation goes through (made on the first gather)

    def _view(self):
        return _t.device_view(self.ekf)

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
        B = self.batch
        src = self._check(u, "u", (B, 6))
        if z is not None and self._check(z, "z", (B, 7)) != src:
            raise ValueError("u and z must have the same dtype")
        if mask is not None:
            if z is None:
                raise ValueError("mask given without z")
            self._check_mask(mask)
        if chi2_max is None:
            if return_nis:
                raise ValueError("return_nis given without chi2_max")
        else:
            if z is None:
                raise ValueError("chi2_max given on a tick without tag poses (z is None)")
            chi2_max = _gate.check_chi2_max(chi2_max)
            _gate.refuse_multirate(self.ekf.params)
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
        with self._ordered(view, u, z, mask):
            _dcheck(D.qdv_pack_inputs(C.byref(view), C.byref(iv), u.data_ptr(), None if z is None else z.data_ptr(),
                                      None if mask is None else mask.data_ptr(), _FLOATS[src]))
            if out is not None:
                ptr = [None if o is None else o.data_ptr() for o in out]
                _gate.gcheck(G.qgt_gate_tick(C.byref(view), C.byref(iv), C.byref(self.ekf.params), chi2_max, ptr[1], ptr[0], ptr[2], ptr[3],
                                             _FLOATS[dn]))
        check(lib().qle_run(self.ekf._h, self._seq._h, t, 1))
        if out is not None:
            return tuple(out) if return_nis else out[0]

    def innovation(self, z, mask=None, dtype=None):
        """(nu [B,6], S [B,6,6], nis [B]) of tag poses z [B,7] against the stored state as device tensors: `innovation(z, mask)` of the
        host path without the host.  Changes nothing.  Filters with mask 0 or without state: nu = 0, S = 0, nis = NaN.
        (The pack always moves an IMU record, so an all-zero one is kept per source dtype; a pack entry that takes u = NULL is a
        follow-up for include/qle_devio.h.)"""
        B = self.batch
        src = self._check(z, "z", (B, 7))
        self._check_mask(mask)
        dn = self._out_dtype(dtype)
        _gate.refuse_multirate(self.ekf.params)
        D, G = devio_lib(), _gate.gate_lib()
        view = self._view()
        iv = self._inputs_view(1)
        zero_u = self._zeros_u(src)
        nu, S, nis = self._alloc([(B, 6), (B, 6, 6), (B,)], dn)
        with self._ordered(view, z, mask):
            _dcheck(D.qdv_pack_inputs(C.byref(view), C.byref(iv), zero_u.data_ptr(), z.data_ptr(),
                                      None if mask is None else mask.data_ptr(), _FLOATS[src]))
            _gate.gcheck(G.qgt_innovation(C.byref(view), C.byref(iv), C.byref(self.ekf.params), nis.data_ptr(), nu.data_ptr(), S.data_ptr(),
                                          _FLOATS[dn]))
        return nu, S, nis

    def _zeros_u(self, src):
        """The pack always moves an IMU record too: an all-zero one per source dtype (the slot is private and every tick packs its own)."""
        if self._zero_u.get(src) is None:
            self._zero_u[src] = _t.empty(self.ekf.device, (self.batch, 6), src, zero=True)
        return self._zero_u[src]

    # ---- filter lifecycle: seed, retire, reseed (health: DeviceRecords)
    def seed(self, z, mask=None, reinit_bias=False):
        """`initialize_state(z, reinit_bias, mask)` of the host path from device tensors: seeds the filters with mask != 0 (None = all)
        from their tag poses z [B,7] (float32 or float64), bit for bit what `qle_initialize_state_masked` writes for the same values.
        Works on a handle that was never seeded from the host.  Asynchronous; the tensors may be reused as soon as the call returns."""
        src = self._check(z, "z", (self.batch, 7))
        self._check_mask(mask)
        D = devio_lib()
        view = self._view()
        iv = self._inputs_view(1)
        zero_u = self._zeros_u(src)
        with self._ordered(view, z, mask):
            self._seed_from_slot(D, view, iv, zero_u, z, mask, src, reinit_bias)

    def _seed_from_slot(self, D, view, iv, zero_u, z, mask, src, reinit_bias):
        _dcheck(D.qdv_pack_inputs(C.byref(view), C.byref(iv), zero_u.data_ptr(), z.data_ptr(), None if mask is None else mask.data_ptr(),
                                  _FLOATS[src]))
        check(lib().qle_initialize_state_slot(self.ekf._h, self._seq._h, 1, int(bool(reinit_bias))))

    def retire(self, mask):
        """The filters with mask != 0 lose their state: they become "uninitialised" (their record is zeroed), every tick leaves them
        untouched and a later `seed` treats them as fresh (upds_since_correction = 0, a one-entry multirate history).  One launch,
        asynchronous."""
        self._check(mask, "mask", (self.batch,), _t.MASKS, align=None)
        H = _health.health_lib()
        view = self._view()
        with self._ordered(view, mask):
            _health.hcheck(H.qhl_retire(C.byref(view), mask.data_ptr()))

    def reseed(self, z, mask=None, reinit_bias=True, **limits):
        """Health check, then seed the flagged filters that have a detection: `health(**limits)` over every filter, reseeded =
        flagged AND mask (mask: the filters z holds a tag pose for; None = all), `seed(z, reseeded, reinit_bias)`.  Returns
        (status, reseeded), uint8 device tensors.  A flagged filter without a detection stays as it is (and stays flagged):
        `retire` it to keep it out of the ticks.

        reinit_bias defaults to True here, unlike `seed`: seeding keeps the bias words of x unless asked to zero them
        (relative_pose_EKF.cpp:317-321), so a NaN bias -- the usual company of a diverged filter -- would survive the reseed and
        break the filter again on its next tick."""
        B = self.batch
        src = self._check(z, "z", (B, 7))
        self._check_mask(mask)
        unknown = set(limits) - {"sigma_r_max", "sigma_v_max", "sigma_theta_max", "qnorm_tol", "select"}
        if unknown:
            raise ValueError(f"reseed: unknown limits {sorted(unknown)}")
        lim = _health.make_limits(**limits)
        D, H = devio_lib(), _health.health_lib()
        view = self._view()
        iv = self._inputs_view(1)
        zero_u = self._zeros_u(src)
        status, reseeded = self._alloc([(B,), (B,)], "uint8")
        with self._ordered(view, z, mask):
            _health.hcheck(H.qhl_health(C.byref(view), C.byref(lim), None, status.data_ptr(), reseeded.data_ptr(), None))
            if mask is not None:
                _health.hcheck(H.qhl_and_masks(C.byref(view), reseeded.data_ptr(), mask.data_ptr(), reseeded.data_ptr()))
            self._seed_from_slot(D, view, iv, zero_u, z, reseeded, src, reinit_bias)
        return status, reseeded

    # ---- a whole tensor sequence per call
    def sequence(self, u_seq, z_seq=None, meas_ticks=None, mask_seq=None):
        """K ticks of tensors -> a `sequence.DeviceSequence`: u_seq [K,B,6]; meas_ticks, a host list of the M strictly increasing tick
        indices in [0, K) that carry a tag pose; z_seq [M,B,7] and mask_seq [M,B] (uint8 / bool; None = all) for those ticks, in tick
        order (float32 or float64, u_seq and z_seq alike).  Creates the K-tick sequence and packs it with ONE call (ceil(K / 32)
        launches of k_sq_pack instead of K packs).  Asynchronous; the tensors may be reused as soon as the call returns."""
        return _seqm.make(self, u_seq, z_seq, meas_ticks, mask_seq)

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
        return _seqm.run(self, seq, t0, n, chi2_max, return_nis, trace_every, trace, x_true_seq, blocks, chi2_hi, dtype)

    def budget_run(self, seq, x_true_seq, every, t0=0, n=None, mask=None, group_tiles=None, **run_kw):
        """The error budget at every `every`-th tick of a run: J = n // every times `run(seq, t0 + j every, every, **run_kw)` followed by
        `budget(x_true_seq[j], mask, group_tiles, out=sums[j])` -- the ticks and the layout of x_true_seq [J,B,16] are those of
        `run(..., trace_every=every, trace=("nees",), x_true_seq=...)`: slice j is taken after tick t0 + (j + 1) every - 1; the ticks
        of a remainder n % every are not run.  Returns a `budget.Budget` over sums [J,G,256]: 256 doubles per group and slice,
        whatever the batch.  J native calls of `run`, a Python loop (run_kw: its chi2_max and the like; no trace);
        asynchronous, no synchronisation.  The state after it is the state after one `run` over the J every ticks, bit for bit."""
        if isinstance(every, bool) or int(every) != every or int(every) < 1:
            raise ValueError(f"every must be an integer >= 1 (got {every})")
        every = int(every)
        if set(run_kw) & {"trace_every", "trace", "x_true_seq"}:
            raise ValueError("budget_run takes no trace: the budget is what it takes every `every` ticks")
        t0, n = _seqm.check_window(t0, n, seq.n_ticks)
        J, B = n // every, self.batch
        self._check(x_true_seq, "x_true_seq", (J, B, 16))
        self._check_mask(mask)
        _, G = _budget.groups(B, group_tiles)
        _budget.budget_lib()   # a missing library is an error before anything is allocated or run
        sums = self._alloc([(J, G, _budget.WORDS)], "float64")[0]
        for j in range(J):
            self.run(seq, t0 + j * every, every, **run_kw)
            self.budget(x_true_seq[j], mask=mask, group_tiles=group_tiles, out=sums[j])
        return _budget.Budget(sums)

    # ---- innovation scoring for noise sweeps
    def scorer(self):
        """A `score.Scorer` for this handle: it owns zeroed fp64 accumulators on the GPU, `observe(u, z, mask)` in front of a `tick` or
        `run(seq)` in place of `run` adds every tag tick's innovation to them (one read-only launch per tag tick, k_score), and
        `result()` / `summary()` read them as per-filter log-likelihood and innovation consistency statistics.  Refused with
        multirate_ekf."""
        return _score.Scorer(self)

    # ---- adaptive tag-pose noise
    def adapter(self, window=20, gain=1.0, n_min=None, chi2_max=float("inf"), R_lo=None, R_hi=None):
        """An `adapt.Adapter` for this handle: every filter estimates its diagonal tag-pose noise R from its own innovations.
        `observe(u, z, mask)` in front of a `tick` adds a noise sample per component of R to fp64 accumulators on the GPU (ONE read-only
        launch, k_adapt_observe); `apply()` moves R towards the window's mean sample, R_k <- clamp(R_k + gain (mean - R_k), R_lo[k],
        R_hi[k]), for every filter that scored at least n_min ticks (None: window // 2) and writes words 18..23 of its parameter record
        (ONE launch, k_adapt_apply); `step(u, z, mask)` is observe, tick and an apply after every window-th tag tick; `run(seq)` is
        the sequence form.  chi2_max: tag ticks with NIS above it are not scored (inf: no limit; the tick still applies them).  Bounds
        default to the shared R / 100 and x 100.  Puts per-filter parameters in force when they are not (one host upload, here only).
        The estimate is the R under which the filter's own model explains its innovations, not the sensor's noise wherever the model is
        off.  Refused with multirate_ekf."""
        return _adapt.Adapter(self, window, gain, n_min, chi2_max, R_lo, R_hi)

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
        return _look.forecast(self, u, h, mask, sigma_r_max, sigma_theta_max)

    # ---- filter banks: posterior weights and a fused estimate per bank, read-only
    def bank(self, members):
        """The handle read as B / members banks of `members` consecutive filters (a power of two in 2..bank.MAX_MEMBERS that divides B):
        a `bank.Bank`, whose `fuse(logw, mask=None)` returns a `bank.Fused` -- the members' posterior weights w_i ~ exp(logw_i) and
        every bank's moment-matched mixture, ONE read-only launch of k_bank_fuse per call.  logw: a float64 device tensor [B], or a
        `score.Scorer` (its log-likelihood).  The handle is not written; multirate handles included."""
        return _bank.Bank(self, members)

    # ---- interacting multiple models: mixing and mode probabilities over the banks
    def imm(self, members, Pi, logmu0=None, logmu_min=math.log(1e-12)):
        """The handle's banks of `members` consecutive filters as an IMM estimator: an `imm.Imm` with the transition matrix Pi [M,M]
        (a nested list, a numpy array or a tensor; checked on the host -- finite, >= 0, rows that add to 1 within 1e-12 -- and uploaded
        once as float64), the log mode probabilities logmu0 [B] (None: uniform) and the floor logmu_min of the recursion (-inf: none).
        `mix(mask)` re-initialises every member from its bank's mixture in ONE launch of k_imm_mix, in place; `update(loglik, mask)` is
        the recursion in ONE launch of k_imm_update; `step(u, z, mask)` runs mix, score, tick, update around one tick; `fuse(mask)` is
        `bank(members).fuse(logmu, mask)`; `mu()` the normalised probabilities.  Refused with multirate_ekf."""
        return _imm.Imm(self, members, Pi, logmu0, logmu_min)

    # ---- device state I/O: set_state from tensors, snapshot, restore, gather, fork
    def set_state(self, x, P=None, mask=None):
        """`set_state(x, P)` of the host path from device tensors: x [B,16] and P [B,n,n] (float32 or float64, alike) become the state
        records in ONE launch (k_si_pack), bit for bit what `qle_set_state` writes for the same values -- (P + P^T) / 2 formed in
        double, then the cast to the compute dtype.  Either may be None: that part of every record is kept.  Filters with mask 0
        (uint8 / bool; None = all) keep their records.  Works on a handle that was never given a state from the host.  As after the
        host call, a multirate history restarts at the next tick and the counters of `enable_gating` go on (a handle without a state
        starts them at 0); with multirate_ekf a mask is refused, because that restart is every filter's.  Asynchronous; the tensors
        may be reused as soon as the call returns."""
        _sio.set_state(self, x, P, mask)

    def snapshot(self, with_params=False):
        """A checkpoint: a `stateio.Snapshot` that owns a bitwise copy of every filter's record (ONE launch of k_si_copy into a
        workspace of its own; with_params=True: of the per-filter parameter records too) and offers `state()`, `report()`,
        `health(...)`, `nees(...)` and `lookahead(...)` on it.  The handle is not written.  A snapshot is the state at this tick:
        it holds neither the multirate history nor the counters (upds_since_correction, the rate limiter)."""
        return _sio.snapshot(self, with_params)

    def restore(self, snap, mask=None, index=None, with_params=False):
        """Write a snapshot back in ONE launch: filter i becomes a bitwise copy of the snapshot's filter index[i] (index: an int32
        device tensor [B]; None = i), for the filters with mask != 0 (None = all) whose index is inside the snapshot.  With an index
        returns `written` [B] (uint8): 0 where mask or index left a filter as it was.  snap may be another `DeviceIO`'s, of the same
        dtype, layout and device -- with an index of any batch size; the two handles' streams are ordered here.  with_params=True:
        the parameter records of a snapshot taken `with_params` travel too.  NaN words and all-zero ("uninitialised") records
        arrive as they are: restoring a retired filter retires the destination.  Then as `set_state`: the history restarts, the
        counters go on, a mask is refused with multirate_ekf."""
        return _sio.restore(self, snap, mask, index, with_params)

    def gather(self, index, mask=None):
        """In place: filter i becomes filter index[i] (a permutation, a resampling step, duplicates welcome) -- a snapshot into a
        workspace this object keeps, then `restore(snapshot, mask, index)`: two launches.  Returns `written` [B].  The per-filter
        parameter records stay where they are."""
        return _sio.gather(self, index, mask)

    def fork(self, members, source=0):
        """Every filter becomes a copy of member `source` of its bank of `members` consecutive filters: `gather` with
        index[i] = (i // members) * members + source.  The per-filter parameter records are not copied: they are what tells a bank's
        members apart (`bank`, `imm`)."""
        return _sio.gather(self, _sio.fork_index(self, members, source))

    def close(self):
        self._gather_snap = None
        if self._seq is not None:
            self._seq.close()
            self._seq = None
