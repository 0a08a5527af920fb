"""Host-side mirror of the reference filter interface over the C-ABI.

`BatchedRelativePoseEKF` keeps the names and argument meaning of the
reference's `class RelativePoseEKF` (quad_state_estimation/include/
relative_pose_EKF.hpp:20-141; Python twin test/rel_pose_EKF_test_class.py)
for a batch of independent filters resident on one MI355X:

    reference (one filter, Eigen)                 here (B filters, numpy in/out)
    prediction_step(x, P, u, &x', &P', &accel)    prediction_step(x, P, u) -> x', P', accel
    correction_step(x, P, r_c_tc, q_ct, &x, &P)   correction_step(x, P, r_c_tc, q_ct) -> x, P
    initialize_state(reinit_bias)                 initialize_state(z, reinit_bias)
    initialize_params()                           initialize_params()
    filter_update(t) single-rate tick             step(u, z, mask) / run(inputs, t0, n)

All compute happens in the HIP kernels behind libqle_ekf.so; nothing here
computes filter arithmetic.
"""
import ctypes as C
import weakref

import numpy as np

from . import _tensors as _t
from . import params as _params
from ._lib import QLE_F32, QLE_F64, QleDeviceView, QlePolicy, QleSynthCfg, check, lib
from .records import ViewRecords

_pd = C.POINTER(C.c_double)
_pu8 = C.POINTER(C.c_uint8)


def _dp(a):
    return None if a is None else a.ctypes.data_as(_pd)


def _f64(a, shape):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != tuple(shape):
        raise ValueError(f"expected shape {tuple(shape)}, got {a.shape}")
    return a


def _u8(a, shape):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.shape != tuple(shape):
        raise ValueError(f"expected mask shape {tuple(shape)}, got {a.shape}")
    return a


class InputSequence:
    """Device-resident IMU / tag-pose sequence (`qle_inputs`)."""

    def __init__(self, ekf, n_ticks, tick_has_meas=None):
        self.ekf = ekf
        self.n_ticks = int(n_ticks)
        thm = np.zeros(self.n_ticks, dtype=np.uint8) if tick_has_meas is None else _u8(tick_has_meas, (self.n_ticks,))
        self.tick_has_meas = thm.copy()
        self._h = C.c_void_p()
        check(lib().qle_inputs_create(ekf._h, self.n_ticks, thm.ctypes.data_as(_pu8), C.byref(self._h)))
        ekf._sequences.append(weakref.ref(self))

    def upload_tick(self, t, u, z=None, mask=None):
        B = self.ekf.batch
        u = _f64(u, (B, 6))
        z = None if z is None else _f64(z, (B, 7))
        mask = _u8(mask, (B,))
        check(lib().qle_inputs_upload_tick(self._h, int(t), _dp(u), _dp(z), None if mask is None else mask.ctypes.data_as(_pu8)))

    def download_tick(self, t):
        B = self.ekf.batch
        u = np.empty((B, 6)); z = np.zeros((B, 7)); m = np.zeros(B, dtype=np.uint8)
        check(lib().qle_inputs_download_tick(self._h, int(t), _dp(u), _dp(z), m.ctypes.data_as(_pu8)))
        return u, z, m

    def close(self):
        if self._h:
            lib().qle_inputs_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BatchedRelativePoseEKF:
    def __init__(self, batch, dtype="f32", device=0, params=None, **param_overrides):
        self.batch = int(batch)
        self.dtype = {"f32": QLE_F32, "fp32": QLE_F32, "float32": QLE_F32, "f64": QLE_F64, "fp64": QLE_F64,
                      "float64": QLE_F64}[str(dtype)]
        self.device = int(device)
        self.params = params if params is not None else _params.default_params()
        _params.set_fields(self.params, **param_overrides)
        self._h = C.c_void_p()
        self._sequences = []
        check(lib().qle_create(C.byref(self._h), self.batch, self.dtype, self.device, C.byref(self.params)))
        self.derived = _params.derive(self.params)

    # ---- lifetime
    def close(self):
        for ref in getattr(self, "_sequences", []):  # sequences live in this handle's device context
            seq = ref()
            if seq is not None:
                seq.close()
        self._sequences = []
        if self._h:
            lib().qle_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- parameters
    @property
    def num_states(self):
        return int(self.derived.num_states)

    def initialize_params(self, **param_overrides):
        """RelativePoseEKF::initialize_params (relative_pose_EKF.cpp:87-125) after changing public members."""
        _params.set_fields(self.params, **param_overrides)
        check(lib().qle_set_params(self._h, C.byref(self.params)))
        self.derived = _params.derive(self.params)

    def set_filter_params(self, pfp):
        """Per-filter [Q diag 12, ab_static 3, wb_static 3, R diag 6]; None = shared parameters."""
        check(lib().qle_set_filter_params(self._h, None if pfp is None else _dp(_f64(pfp, (self.batch, 24)))))

    def get_filter_params(self):
        """The per-filter [Q diag 12, ab_static 3, wb_static 3, R diag 6] records as the device holds them."""
        out = np.empty((self.batch, 24))
        check(lib().qle_get_filter_params(self._h, _dp(out)))
        return out

    # ---- state
    def set_state(self, x, P):
        n = self.num_states
        check(lib().qle_set_state(self._h, _dp(_f64(x, (self.batch, 16))), _dp(_f64(P, (self.batch, n, n)))))

    def get_state(self):
        n = self.num_states
        x = np.empty((self.batch, 16)); P = np.empty((self.batch, n, n))
        check(lib().qle_get_state(self._h, _dp(x), _dp(P)))
        return x, P

    def gather_state(self, index, mask=None):
        """In place, on the device: filter i becomes a bitwise copy of filter index[i] (int32 [B]; a permutation, a resampling step,
        the members of a bank forked from one filter) for the filters with mask != 0 (None = all) whose index is in 0..B-1 -- what
        `DeviceIO.gather` does, for host arrays: the state never passes through the host.  Returns `written` [B] (uint8).  Then as
        `set_state`: a multirate history restarts at the next tick (a mask is refused with multirate_ekf), the counters go on."""
        from . import stateio as sio
        return sio.gather_host(self, index, mask)

    def initialize_state(self, z, reinit_bias=False, mask=None):
        """RelativePoseEKF::initialize_state (relative_pose_EKF.cpp:305-344) from each filter's first tag pose.
        mask [batch]: seed only those filters (the node seeds a filter on its own first detection,
        relative_pose_EKF_node.cpp:169-174); filters never seeded are skipped by every tick (relative_pose_EKF.cpp:129-130)."""
        m = _u8(mask, (self.batch,))
        check(lib().qle_initialize_state_masked(self._h, _dp(_f64(z, (self.batch, 7))), None if m is None else m.ctypes.data_as(_pu8),
                                                int(bool(reinit_bias))))

    def state_initialized(self):
        out = np.zeros(self.batch, np.uint8)
        check(lib().qle_get_state_initialized(self._h, out.ctypes.data_as(_pu8)))
        return out

    def enable_aux(self, on=True):
        check(lib().qle_enable_aux(self._h, int(bool(on))))

    def get_aux(self):
        acc = np.empty((self.batch, 3)); obs = np.empty((self.batch, 7))
        check(lib().qle_get_aux(self._h, _dp(acc), _dp(obs)))
        return acc, obs

    # ---- hot path on the resident state
    def predict(self, u):
        check(lib().qle_predict(self._h, _dp(_f64(u, (self.batch, 6)))))

    def update(self, z, mask=None):
        m = _u8(mask, (self.batch,))
        check(lib().qle_update(self._h, _dp(_f64(z, (self.batch, 7))), None if m is None else m.ctypes.data_as(_pu8)))

    def step(self, u, z=None, mask=None):
        """One single-rate filter_update tick (relative_pose_EKF.cpp:238-249,265-290)."""
        m = _u8(mask, (self.batch,))
        zz = None if z is None else _f64(z, (self.batch, 7))
        check(lib().qle_step(self._h, _dp(_f64(u, (self.batch, 6))), _dp(zz), None if m is None else m.ctypes.data_as(_pu8)))

    # ---- innovation diagnostics and the chi-square outlier gate
    def innovation(self, z, mask=None):
        """(nu [B,6], S [B,6,6], nis [B]) of tag poses z against the current state: the innovation delta_y and its covariance
        S = G P G^T + R_k of correction_step (relative_pose_EKF.cpp:447-475) and NIS = delta_y^T S^-1 delta_y.  The state is
        unchanged.  Filters with mask 0 or without state: nu = 0, S = 0, nis = NaN."""
        B = self.batch
        m = _u8(mask, (B,))
        nu = np.empty((B, 6)); S = np.empty((B, 36)); nis = np.empty(B)
        check(lib().qle_innovation(self._h, _dp(_f64(z, (B, 7))), None if m is None else m.ctypes.data_as(_pu8), _dp(nu), _dp(S), _dp(nis)))
        return nu, S.reshape(B, 6, 6), nis

    def update_gated(self, z, chi2_max, mask=None):
        """update(z, mask) on the filters whose NIS <= chi2_max only (16.81 / 22.46: the 0.99 / 0.999 quantiles of chi-square
        with 6 degrees of freedom).  Returns (accepted [B] bool, nis [B])."""
        B = self.batch
        m = _u8(mask, (B,))
        acc = np.zeros(B, np.uint8); nis = np.empty(B)
        check(lib().qle_update_gated(self._h, _dp(_f64(z, (B, 7))), None if m is None else m.ctypes.data_as(_pu8), float(chi2_max),
                                     acc.ctypes.data_as(_pu8), _dp(nis)))
        return acc.astype(bool), nis

    def step_gated(self, u, z, chi2_max, mask=None):
        """step(u, z, mask) with the same gate between predict and correct (three launches, not the fused tick).
        Returns (accepted [B] bool, nis [B])."""
        B = self.batch
        m = _u8(mask, (B,))
        acc = np.zeros(B, np.uint8); nis = np.empty(B)
        check(lib().qle_step_gated(self._h, _dp(_f64(u, (B, 6))), _dp(_f64(z, (B, 7))), None if m is None else m.ctypes.data_as(_pu8),
                                   float(chi2_max), acc.ctypes.data_as(_pu8), _dp(nis)))
        return acc.astype(bool), nis

    # ---- filter_update with the decision logic on the device (relative_pose_EKF.cpp:147-186)
    def enable_gating(self, on=True):
        check(lib().qle_enable_gating(self._h, int(bool(on))))

    def filter_update(self, u, z=None, measurement_ready=None, t_curr=None, apriltag_time=None):
        """One filter_update tick: rate limit + corner gate + predict (+ correct) per filter; with
        multirate_ekf the correction goes to the delayed history entry and the predicts are replayed.
        t_curr / apriltag_time [batch] feed dynamic_meas_delay (relative_pose_EKF.cpp:199)."""
        m = _u8(measurement_ready, (self.batch,))
        zz = None if z is None else _f64(z, (self.batch, 7))
        mp = None if m is None else m.ctypes.data_as(_pu8)
        if t_curr is None:
            check(lib().qle_filter_update(self._h, _dp(_f64(u, (self.batch, 6))), _dp(zz), mp))
        else:
            st = None if apriltag_time is None else _f64(apriltag_time, (self.batch,))
            check(lib().qle_filter_update_stamped(self._h, _dp(_f64(u, (self.batch, 6))), _dp(zz), mp, float(t_curr), _dp(st)))

    def measurement_delay(self):
        out = np.zeros(self.batch)
        check(lib().qle_get_measurement_delay(self._h, _dp(out)))
        return out

    def set_uniform_measurement_age(self, seconds):
        check(lib().qle_set_uniform_measurement_age(self._h, float(seconds)))

    def history_info(self):
        """Bookkeeping of the multirate history (read-only): dict of k, Nc, Cu, tick, e_tick, e_want as the host holds them and
        hist_first [batch] int32 from the device (k_step_mr, ekf_multirate.hpp)."""
        info = (C.c_int64 * 6)(); hf = np.zeros(self.batch, np.int32)
        check(lib().qle_get_history_info(self._h, info, hf.ctypes.data_as(C.POINTER(C.c_int32))))
        d = dict(zip(("k", "Nc", "Cu", "tick", "e_tick", "e_want"), (int(v) for v in info)))
        d["hist_first"] = hf
        return d

    def tick_flags(self):
        """(performed_correction, consumed, upds_since_correction) after the last tick."""
        pc = np.zeros(self.batch, np.uint8); co = np.zeros(self.batch, np.uint8); up = np.zeros(self.batch, np.int32)
        check(lib().qle_get_tick_flags(self._h, pc.ctypes.data_as(_pu8), co.ctypes.data_as(_pu8), up.ctypes.data_as(C.POINTER(C.c_int32))))
        return pc, co, up

    # ---- reference-shaped value-in / value-out calls
    def prediction_step(self, x_km1, P_km1, u):
        """prediction_step(x_km1, P_km1, u) -> (x_check, P_check, pose_accel)   (relative_pose_EKF.cpp:346-415)."""
        self.set_state(x_km1, P_km1)
        self.enable_aux(True)
        self.predict(u)
        x, P = self.get_state()
        return x, P, self.get_aux()[0]

    def correction_step(self, x_check, P_check, r_c_tc, q_ct):
        """correction_step(x_check, P_check, r_c_tc, q_ct) -> (x_hat, P_hat)   (relative_pose_EKF.cpp:417-502)."""
        self.set_state(x_check, P_check)
        z = np.concatenate([_f64(r_c_tc, (self.batch, 3)), _f64(q_ct, (self.batch, 4))], axis=1)
        self.update(z)
        return self.get_state()

    # ---- device-resident sequences
    def make_inputs(self, n_ticks, tick_has_meas=None):
        return InputSequence(self, n_ticks, tick_has_meas)

    def run(self, inputs, t0, n):
        check(lib().qle_run(self._h, inputs._h, int(t0), int(n)))

    def run_resident(self, inputs, t0, n):
        """n ticks in one launch with the state held on-chip (reported separately from the per-tick metric)."""
        check(lib().qle_run_resident(self._h, inputs._h, int(t0), int(n)))

    def synth_generate(self, inputs, seed, filter_offset=0, perturb_filter_params=False, **kw):
        c = QleSynthCfg()
        check(lib().qle_synth_cfg_default(C.byref(c)))
        c.seed = int(seed); c.filter_offset = int(filter_offset); c.perturb_filter_params = int(bool(perturb_filter_params))
        for k, v in kw.items():
            setattr(c, k, v)
        check(lib().qle_synth_generate(self._h, inputs._h, C.byref(c)))

    def synth_truth(self, inputs):
        """(pose [batch,7], imu_bias [batch,6]) of the generator's truth at the end of the sequence."""
        pose = np.empty((self.batch, 7)); bias = np.empty((self.batch, 6))
        check(lib().qle_synth_get_truth(self._h, inputs._h, _dp(pose), _dp(bias)))
        return pose, bias

    def synth_rmse(self, inputs):
        out = np.zeros(3)
        check(lib().qle_synth_rmse(self._h, inputs._h, _dp(out)))
        return out

    # ---- filter consistency against a truth (include/qle_consistency.h)
    def nees(self, x_true, mask=None, blocks="all", chi2_hi=float("inf")):
        """Normalised estimation error squared e^T P^-1 e of every filter against the truth x_true [B,16] (r, v, q xyzw, ab, wb: the
        layout of the state, with the total true biases), e = truth minus estimate in the filter's error-state convention, over all
        states or the marginal of `blocks` ("all", "pose", "r", "r+theta+ab+wb", ... or the bit mask of include/qle_consistency.h).
        Host arrays in and out; the arithmetic runs on the device (k_nees), the state is unchanged.  Returns a dict: nees [B]
        (NaN for a filter with mask 0, without state, or with a covariance that is not positive definite), err [B,n] and the fields
        of the batch summary (consistency.SUMMARY_FIELDS) with mean_nees = sum_nees / count added."""
        from . import consistency as cs
        B, n = self.batch, self.num_states
        xt = _f64(x_true, (B, 16))
        m = _u8(mask, (B,))
        bits = cs.block_mask(blocks, n)
        chi2_hi = cs.check_chi2_hi(chi2_hi)
        K = cs.consistency_lib()
        view = _t.device_view(self)
        nees = np.empty(B); err = np.empty((B, n)); s = cs.QcsSummary()
        cs.ccheck(K.qcs_nees_host(C.byref(view), C.byref(self.params), _dp(xt), None if m is None else m.ctypes.data_as(_pu8), bits, chi2_hi,
                                  _dp(nees), _dp(err), C.byref(s)))
        out = {"nees": nees, "err": err}
        out.update({k: float(getattr(s, k)) for k in cs.SUMMARY_FIELDS})
        out["mean_nees"] = out["sum_nees"] / out["count"] if out["count"] > 0 else float("nan")
        return out

    def synth_nees(self, inputs, chi2_hi=float("inf")):
        """nees() against the generator's truth at the end of `inputs` (synth_truth: pose and IMU bias; the generator keeps no
        velocity, so the velocity block is left out): blocks r, theta, ab, wb, or r, theta for a filter without bias states.
        The generator's bias truth is the unknown part of the IMU bias; the total true bias adds the static (known) biases, per filter
        where per-filter parameters are in force."""
        xt = self._synth_truth_rows(inputs)
        return self.nees(xt, blocks="r+theta+ab+wb" if self.num_states == 15 else "r+theta", chi2_hi=chi2_hi)

    def _synth_truth_rows(self, inputs):
        """the generator's truth at the end of `inputs` as x_true rows [B,16] (no velocity: zeros), with the total true biases"""
        pose, bias = self.synth_truth(inputs)
        if _t.device_view(self).filter_params:
            static = self.get_filter_params()[:, 12:18]
        else:
            static = np.array(list(self.params.ab_static) + list(self.params.wb_static))[None, :]
        xt = np.zeros((self.batch, 16))
        xt[:, 0:3] = pose[:, 0:3]; xt[:, 6:10] = pose[:, 3:7]; xt[:, 10:16] = bias + static
        return xt

    # ---- the per-component error budget against a truth (include/qle_budget.h)
    def error_budget(self, x_true, mask=None, group_tiles=None):
        """The error budget of the batch against the truth x_true [B,16] (the layout of `nees`), or [16] / [1,16]: one reference row
        for every filter.  Host arrays in and out; the arithmetic runs on the device (k_budget, k_budget_reduce), the state is
        unchanged.  Returns a `budget.Budget` over numpy arrays: sums [G,256] per group of group_tiles 64-filter tiles (None: one
        group), err [B,n] and status [B] (0 off, 1 counted, 2 on but not finite); its mean, cov, P_mean, var_ratio, rms and sigma
        are the budget.  The bits are those of `DeviceIO.budget` on the same values."""
        from . import budget as bg
        B, n = self.batch, self.num_states
        xt = np.ascontiguousarray(x_true, np.float64)
        rows = 1 if xt.shape in ((16,), (1, 16)) else B
        xt = _f64(xt.reshape(1, 16) if rows == 1 else xt, (rows, 16))
        m = _u8(mask, (B,))
        gt, G = bg.groups(B, group_tiles)
        K = bg.budget_lib()
        view = _t.device_view(self)
        sums = np.empty((G, bg.WORDS)); err = np.empty((B, n)); status = np.empty(B, np.uint8)
        bg.bcheck(K.qbg_budget_host(C.byref(view), C.byref(self.params), _dp(xt), rows, None if m is None else m.ctypes.data_as(_pu8), gt,
                                    _dp(sums), _dp(err), status.ctypes.data_as(_pu8)))
        return bg.Budget(sums, err, status)

    def synth_budget(self, inputs, group_tiles=None):
        """error_budget() against the generator's truth at the end of `inputs`, beside `synth_nees`.  The generator keeps no velocity:
        the velocity components of the budget are the estimate's own (against zero) and mean nothing."""
        return self.error_budget(self._synth_truth_rows(inputs), group_tiles=group_tiles)

    # ---- innovation scoring for noise sweeps (include/qle_score.h)
    def score(self, inputs, t0, n):
        """Ticks [t0, t0 + n) of `inputs`, scored: what `run(inputs, t0, n)` does, with every tag pose's innovation against the
        predicted state accumulated per filter on the device (k_score, read-only, in front of the unchanged tick).  Returns a dict of
        numpy arrays: acc [40,B] (the accumulator words of include/qle_score.h) and the fields of `score.Score` -- n, n_bad, nis_mean,
        loglik [B], var_ratio, rho1, nu_mean [B,6].  Refused with multirate_ekf."""
        from . import score as sc
        acc = sc.run_host(self, inputs, t0, n)
        with np.errstate(divide="ignore", invalid="ignore"):
            s = sc.Score(acc)
        return {"acc": acc, "n": s.n, "n_bad": s.n_bad, "nis_mean": s.nis_mean, "loglik": s.loglik, "var_ratio": s.var_ratio, "rho1": s.rho1,
                "nu_mean": s.nu_mean}

    def adapt_noise(self, inputs, t0, n, **cfg):
        """Ticks [t0, t0 + n) of `inputs`, with every filter's tag-pose noise R adapted from its innovations on the device: what
        `DeviceIO.adapter(**cfg).run` does (cfg: window, gain, n_min, chi2_max, R_lo, R_hi), for host arrays.  Puts per-filter
        parameters in force when they are not.  Returns a dict of numpy arrays: acc [24,B] (the accumulator words of
        include/qle_adapt.h), R [B,6] (the values in force after the run) and the fields of `adapt.Adaptation` -- n, n_bad, n_rejected,
        n_total, windows [B], r_hat, ratio [B,6].  Refused with multirate_ekf."""
        from . import adapt as ad
        acc, R = ad.run_host(self, inputs, t0, n, **cfg)
        with np.errstate(divide="ignore", invalid="ignore"):
            a = ad.Adaptation(acc)
        return {"acc": acc, "R": R, "n": a.n, "n_bad": a.n_bad, "n_rejected": a.n_rejected, "n_total": a.n_total, "windows": a.windows,
                "r_hat": a.r_hat, "ratio": a.ratio}

    # ---- filter health
    def health(self, mask=None, sigma_r_max=float("inf"), sigma_v_max=float("inf"), sigma_theta_max=float("inf"), qnorm_tol=1e-3, select=None):
        """Which filters are broken?  Host arrays in and out; the classification runs on the device (k_health), the state is unchanged.
        Returns a dict: status [B] (uint8, the bits of health.BITS; 0 for a filter with mask 0 or without state), flagged [B]
        (bool: status & select) and the counts of the batch summary (health.SUMMARY_FIELDS).  Arguments: `DeviceIO.health`."""
        from . import health as hl
        B = self.batch
        m = _u8(mask, (B,))
        lim = hl.make_limits(sigma_r_max, sigma_v_max, sigma_theta_max, qnorm_tol, select)
        H = hl.health_lib()
        view = _t.device_view(self)
        status = np.zeros(B, np.uint8); flagged = np.zeros(B, np.uint8); s = hl.QhlSummary()
        hl.hcheck(H.qhl_health_host(C.byref(view), C.byref(lim), None if m is None else m.ctypes.data_as(_pu8), status.ctypes.data_as(_pu8),
                                    flagged.ctypes.data_as(_pu8), C.byref(s)))
        out = {"status": status, "flagged": flagged.astype(bool)}
        out.update({k: int(getattr(s, k)) for k in hl.SUMMARY_FIELDS})
        return out

    # ---- look-ahead
    def lookahead(self, u, h, mask=None, sigma_r_max=float("inf"), sigma_theta_max=float("inf")):
        """State and covariance h ticks ahead with the IMU sample u [B,6] held: what h calls of `predict(u)` would leave, without
        writing the handle (one launch of k_lookahead; arguments: `DeviceIO.lookahead`).  Host arrays in and out.  Returns
        (x [B,16], P [B,n,n], ticks_to_limit [B] int32 or None when no limit is given); skipped filters: zero rows, -1."""
        from . import lookahead as lk
        B = self.batch
        uu = _f64(u, (B, 6))
        h = lk.check_horizon(h)
        m = _u8(mask, (B,))
        coast = lk.make_coast(sigma_r_max, sigma_theta_max)
        K = lk.lookahead_lib()
        view = _t.device_view(self)
        nbytes = lk.kcheck(K.qlk_workspace_bytes(C.byref(view)))
        workspace = _t.empty(self.device, (nbytes,), "uint8")
        ticks = np.empty(B, np.int32) if coast is not None else None
        ahead = QleDeviceView()
        lk.kcheck(K.qlk_lookahead_host(C.byref(view), C.byref(self.params), _dp(uu), h, None if m is None else m.ctypes.data_as(_pu8),
                                       workspace.data_ptr(), nbytes, C.byref(ahead), None if coast is None else C.byref(coast),
                                       None if ticks is None else ticks.ctypes.data_as(C.POINTER(C.c_int32))))
        x, P = ViewRecords(self, B, ahead, workspace).state(dtype="float64")
        return x.cpu().numpy(), P.cpu().numpy(), ticks

    def fuse_banks(self, members, logw, mask=None):
        """The handle read as B / members banks of `members` consecutive filters (`DeviceIO.bank`): the members' posterior weights
        w_i ~ exp(logw_i) and every bank's moment-matched estimate, without writing the handle (one launch of k_bank_fuse).  Host arrays
        in and out: logw [B] float64, mask [B] or None (all).  Returns (x [G,16], P [G,n,n], w [B], best [G] int32); an empty bank: zero
        rows and best = -1."""
        from . import bank as bk
        B = self.batch
        M = bk.check_members(members, B)
        G = B // M
        lw = _f64(logw, (B,))
        m = _u8(mask, (B,))
        K = bk.bank_lib()
        view = _t.device_view(self)
        nbytes = bk.bcheck(K.qbk_workspace_bytes(C.byref(view), M))
        workspace = _t.empty(self.device, (nbytes,), "uint8")
        w = np.empty(B); best = np.empty(G, np.int32)
        fused = QleDeviceView()
        bk.bcheck(K.qbk_fuse_host(C.byref(view), M, _dp(lw), None if m is None else m.ctypes.data_as(_pu8), workspace.data_ptr(), nbytes,
                                  C.byref(fused), _dp(w), best.ctypes.data_as(C.POINTER(C.c_int32))))
        x, P = ViewRecords(self, G, fused, workspace).state(dtype="float64")
        return x.cpu().numpy(), P.cpu().numpy(), w, best

    def mix_banks(self, members, logmu, Pi, mask=None):
        """The IMM mixing step of the handle's banks of `members` consecutive filters (`DeviceIO.imm`, `imm.Imm.mix`) with host arrays:
        logmu [B] float64 (unnormalised log mode probabilities), Pi [M,M] (Pi[i][j] = P(mode i -> mode j); checked on the host), mask
        [B] or None (all).  Every mixed member's record becomes the moment-matched mixture of its bank under mu_{i|j}, in place (one
        launch of k_imm_mix).  Returns (logc [B] float64, mixed [B] uint8).  Refused with multirate_ekf."""
        from . import imm as _imm
        return _imm.mix_host(self, members, logmu, Pi, mask)

    # ---- reporting / control
    def report(self):
        """What the node publishes after a tick (relative_pose_EKF_node.cpp:192-220)."""
        B = self.batch
        pose = np.empty((B, 7)); cov = np.empty((B, 36)); vel = np.empty((B, 3)); bias = np.empty((B, 6))
        check(lib().qle_get_report(self._h, _dp(pose), _dp(cov), _dp(vel), _dp(bias)))
        return {"pose": pose, "pose_cov": cov.reshape(B, 6, 6), "vel": vel, "bias": bias}

    def node_report(self):
        """Everything the node publishes after a tick (relative_pose_EKF_node.cpp:192-281) in one call: a numpy record array
        with one entry per filter (fields of `struct qle_node_report`)."""
        from ._lib import QleNodeReport
        buf = (QleNodeReport * self.batch)()
        check(lib().qle_get_node_report(self._h, buf))
        return np.ctypeslib.as_array(buf).copy() if hasattr(np.ctypeslib, "as_array") else np.frombuffer(buf, dtype=np.dtype(QleNodeReport)).copy()

    def count_nonfinite(self):
        c = C.c_int64(0)
        check(lib().qle_count_nonfinite(self._h, C.byref(c)))
        return int(c.value)

    def synchronize(self):
        check(lib().qle_synchronize(self._h))

    def timer_begin(self):
        check(lib().qle_timer_begin(self._h))

    def timer_end(self):
        ms = C.c_float(0)
        check(lib().qle_timer_end(self._h, C.byref(ms)))
        return float(ms.value)

    def policy(self):
        """How this handle launches its ticks (dict of `struct qle_policy`) plus `served_by`: where the state lives between ticks."""
        pol = QlePolicy()
        check(lib().qle_get_policy(self._h, C.byref(pol)))
        d = {n: int(getattr(pol, n)) for n, _ in QlePolicy._fields_}
        # 256 MiB Infinity Cache (MI355X_MICROARCH.md): a state ring that fits stays resident from tick to tick under policies 0-2;
        # the split policy keeps a fixed part resident and streams the rest; anything larger streams from HBM
        # "split": part of what a tick touches is served on die, part by HBM -- the cached / streamed split policy, a state a
        # little larger than the cache under the cached policy, or the multirate filter (state on die, history streamed to HBM)
        cache = 250 * 2 ** 20
        if d["state_policy"] == 3 or (d["ring_bytes"] > cache and (d["state_bytes"] <= cache or d["state_policy"] == 0)):
            d["served_by"] = "split"
        elif d["ring_bytes"] <= cache:
            d["served_by"] = "infinity_cache"
        else:
            d["served_by"] = "hbm"
        return d

    def algorithmic_bytes(self, kind):
        return int(lib().qle_algorithmic_bytes(self._h, int(kind)))
