"""ctypes binding of include/qle_adapt.h (libqle_adapt.so): adaptive tag-pose noise, R estimated from the innovations on the device.

Scoring, banks and IMM answer "which R_r / R_ang is right?" by enumeration over hand-picked candidates.  Here every filter estimates
its own diagonal R from the innovations it already forms: per tag tick one read-only kernel (k_adapt_observe, csrc/ekf_adapt.hpp: the
arithmetic of k_score with a noise sample r^_k = R_k + R_k^2 (a_k^2 - c_k) per component into an fp64 accumulator record per filter) in
front of the unchanged tick, and once per window one kernel (k_adapt_apply) that moves R towards the window's mean sample and writes
words 18..23 of the filter's parameter record, which the next tick reads.  `DeviceIO.adapter()` (devio.py) makes an `Adapter` for
device tensors, `BatchedRelativePoseEKF.adapt_noise` (ekf.py) is the host-array form.  There is no fallback: a missing library is an
error.

What the estimate means: the R under which this filter's own model explains its innovations -- not the noise of the sensor wherever
the model is off.  Not provided: adaptation of Q, multirate handles, a full (non-diagonal) R, per-filter bounds, adaptation inside
`io.run` or `Scorer.run` (those keep their bits; `Adapter.run` is the sequence form).
"""
import ctypes as C
import math

from . import _tensors as _t
from . import gate as _gate
from ._lib import QleDeviceView, QleInputsView, QleParams, SideLibrary
from ._observer import TagTickObserver

WORDS = 24   # QAD_WORDS
# the words of an accumulator record: name -> (first word, count)
LAYOUT = {"n": (0, 1), "n_bad": (1, 1), "sum_r_hat": (2, 6), "sum_a_sq": (8, 6), "sum_c": (14, 6), "n_total": (20, 1), "windows": (21, 1),
          "n_rejected": (22, 1)}


class QadConfig(C.Structure):
    """`struct qad_config`"""
    _fields_ = [("struct_size", C.c_uint32), ("window", C.c_int32), ("gain", C.c_double), ("n_min", C.c_int32), ("reserved", C.c_int32),
                ("chi2_max", C.c_double), ("R_lo", C.c_double * 6), ("R_hi", C.c_double * 6)]


_vp = C.c_void_p
_pview, _pin, _ppar, _pcfg = C.POINTER(QleDeviceView), C.POINTER(QleInputsView), C.POINTER(QleParams), C.POINTER(QadConfig)
_pd = C.POINTER(C.c_double)
# every symbol include/qle_adapt.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "qad_last_error": (C.c_char_p, []),
    "qad_launch_count": (C.c_int64, []),
    "qad_launch_census_begin": (C.c_int, []),
    "qad_launch_census_end": (C.c_int, [C.c_char_p, C.c_int64, C.POINTER(C.c_int64)]),
    "qad_observe_tick": (C.c_int, [_pview, _pin, _ppar, _vp, C.c_double]),
    "qad_apply": (C.c_int, [_pview, _vp, _pcfg, _vp, _vp]),
    "qad_run": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, _ppar, _vp, _pcfg]),
    "qad_run_host": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, _ppar, _pcfg, _pd, _pd]),
}

ADAPT = SideLibrary("adapt", "QLE_ADAPT_LIB", SYMBOLS, "noise adaptation", "qad_last_error", needs_tick_library=True)
ADAPT_LIB_PATH, adapt_lib, qcheck = ADAPT.path, ADAPT.load, ADAPT.check


def make_config(ekf, window=20, gain=1.0, n_min=None, chi2_max=float("inf"), R_lo=None, R_hi=None):
    """A `QadConfig`, checked on the host as the library checks it: window >= 1, gain in (0, 1], n_min >= 1 (None: window // 2, at
    least 1), chi2_max > 0 (inf: no limit), and the bounds R_lo / R_hi [6] of the applied R (None: the handle's shared R / 100 and
    x 100), finite, > 0, R_hi >= R_lo."""
    window = int(window)
    if window < 1:
        raise ValueError(f"window must be >= 1 (got {window})")
    gain = float(gain)
    if not 0.0 < gain <= 1.0:
        raise ValueError(f"gain must lie in (0, 1] (got {gain})")
    n_min = max(window // 2, 1) if n_min is None else int(n_min)
    if n_min < 1:
        raise ValueError(f"n_min must be >= 1 (got {n_min})")
    chi2_max = _gate.check_chi2_max(chi2_max)
    shared = [float(r) for r in ekf.derived.R]
    lo = [r / 100.0 for r in shared] if R_lo is None else [float(r) for r in R_lo]
    hi = [r * 100.0 for r in shared] if R_hi is None else [float(r) for r in R_hi]
    if len(lo) != 6 or len(hi) != 6:
        raise ValueError("R_lo and R_hi must have 6 entries (R_r x, y, z, then R_ang x, y, z)")
    for k in range(6):
        if not (math.isfinite(lo[k]) and lo[k] > 0.0):
            raise ValueError(f"R_lo[{k}] must be finite and > 0 (got {lo[k]})")
        if not hi[k] >= lo[k]:
            raise ValueError(f"R_hi[{k}] = {hi[k]} is below R_lo[{k}] = {lo[k]}")
    c = QadConfig()
    c.struct_size = C.sizeof(QadConfig)
    c.window, c.gain, c.n_min, c.chi2_max = window, gain, n_min, chi2_max
    c.R_lo, c.R_hi = (C.c_double * 6)(*lo), (C.c_double * 6)(*hi)
    return c


def shared_record(ekf):
    """The handle's shared parameters as one 24-word per-filter record: Q diag 12, ab_static 3, wb_static 3, R diag 6."""
    return [*ekf.derived.Q, *ekf.params.ab_static, *ekf.params.wb_static, *ekf.derived.R]


def _in_force(ekf):
    """Per-filter parameters in force: where they are not, the shared record replicated (one host upload)."""
    import numpy as np
    if not _t.device_view(ekf).filter_params:
        ekf.set_filter_params(np.tile(np.asarray(shared_record(ekf), dtype=np.float64), (ekf.batch, 1)))


class Adaptation:
    """The accumulators of an `Adapter` read per filter (torch tensors on the device, or numpy arrays from
    `BatchedRelativePoseEKF.adapt_noise`): n (scored ticks in the open window), n_bad, n_rejected, n_total, windows [B]; r_hat [B,6] =
    sum r^ / n, the mean noise sample of the open window (what an apply with gain 1 would write; NaN for an empty window); ratio [B,6] =
    sum a^2 / sum c, 1 where the filter's R explains its innovations, above 1 where R is too small."""

    def __init__(self, acc):
        """acc: [WORDS, B] float64, a torch tensor or a numpy array."""
        w = lambda name: acc[LAYOUT[name][0]:LAYOUT[name][0] + LAYOUT[name][1]]   # noqa: E731
        self.n, self.n_bad, self.n_total, self.windows, self.n_rejected = acc[0], acc[1], acc[20], acc[21], acc[22]
        self.r_hat = (w("sum_r_hat") / acc[0]).T
        self.ratio = (w("sum_a_sq") / w("sum_c")).T


class Adapter(TagTickObserver):
    """Noise adaptation of a handle fed from device tensors (`DeviceIO.adapter()`).  Owns a zeroed accumulator tensor `acc`
    [WORDS, padded batch] (float64, include/qle_adapt.h) on the handle's GPU and the configuration `cfg`.  Puts per-filter parameters
    in force when they are not (the shared record replicated: a host upload, at construction only); after that every call is
    asynchronous and none synchronises.  `ekf.get_filter_params()` reads the adapted R back (words 18..23)."""
    LIB, WORDS, WHAT, RESULT = ADAPT, WORDS, "noise adaptation", Adaptation

    def __init__(self, io, window=20, gain=1.0, n_min=None, chi2_max=float("inf"), R_lo=None, R_hi=None):
        super().__init__(io)
        self.cfg = make_config(io.ekf, window, gain, n_min, chi2_max, R_lo, R_hi)
        _in_force(io.ekf)
        self._tags = 0   # tag ticks `step` has taken since the last reset: the window counter, kept on the host

    def reset(self):
        """Zero the accumulators and the window counter of `step`; the adapted R stays in the parameter records."""
        super().reset()
        self._tags = 0

    def observe(self, u, z, mask=None):
        """Add the tag poses of the tick `io.tick(u, z, mask)` is about to run -- call it BEFORE that tick: packs u [B,6], z [B,7] and
        mask [B] (uint8 / bool; None = all) into the slot the tick will pack again, and adds every filter's noise sample, taken
        against the predicted state, to its accumulators.  One pack and ONE launch of k_adapt_observe; neither the state nor the
        parameter records are touched."""
        super().observe(u, z, mask)

    def _observe_tick(self, Q, view, iv):
        return Q.qad_observe_tick(C.byref(view), C.byref(iv), C.byref(self.io.ekf.params), self.acc.data_ptr(), self.cfg.chi2_max)

    def apply(self):
        """The M-step: every filter with n >= n_min gets R_k <- clamp(R_k + gain (sum r^_k / n - R_k), R_lo[k], R_hi[k]) written into
        its parameter record and its window zeroed; the others are not written and keep their open window.  ONE launch of
        k_adapt_apply.  Returns (R [B,6] float64, the values now in force whether applied or not; applied [B] uint8)."""
        io = self.io
        B = io.ekf.batch
        Q = adapt_lib()
        view = io._view()
        R = io._alloc([(B, 6)], "float64")[0]
        applied = io._alloc([(B,)], "uint8")[0]
        with io._ordered(view, self.acc):
            qcheck(Q.qad_apply(C.byref(view), self.acc.data_ptr(), C.byref(self.cfg), applied.data_ptr(), R.data_ptr()))
        return R, applied

    def step(self, u, z=None, mask=None):
        """One adapted tick: `observe(u, z, mask)` where the tick has tag poses, `io.tick(u, z, mask)`, and `apply()` after every
        window-th tag tick since the last `reset` (the counter is kept on the host).  Returns what `apply` returned, or None on a
        tick without one.  Never synchronises."""
        if z is not None:
            self.observe(u, z, mask)
        self.io.tick(u, z, mask)
        if z is not None:
            self._tags += 1
            if self._tags % self.cfg.window == 0:
                return self.apply()
        return None

    def run(self, seq, t0=0, n=None):
        """Ticks [t0, t0 + n) of a `DeviceSequence` (n None: to its end), adapted, in ONE native call (qad_run): k_adapt_observe in front
        of every tick that has a tag slot, the tick, and k_adapt_apply after every window-th tag-slot tick, counted from the start of
        this call -- the bits of the loop of `step` over the same ticks after a `reset`."""
        super().run(seq, t0, n)

    def _run(self, Q, seq, t0, n):
        return Q.qad_run(self.io.ekf._h, seq.inputs._h, t0, n, C.byref(self.io.ekf.params), self.acc.data_ptr(), C.byref(self.cfg))

    def result(self):
        """The accumulators as an `Adaptation` of device tensors [B] / [B,6]; no synchronisation."""
        return super().result()


def run_host(ekf, inputs, t0, n, **cfg):
    """qad_run_host: ticks [t0, t0 + n) of an `InputSequence`, adapted; (acc [WORDS, B], R [B, 6]) as numpy arrays.  Puts per-filter
    parameters in force when they are not."""
    import numpy as np
    _gate.refuse_multirate(ekf.params, "noise adaptation")
    c = make_config(ekf, **cfg)
    _in_force(ekf)
    acc, R = np.zeros((WORDS, ekf.batch)), np.zeros((ekf.batch, 6))
    qcheck(adapt_lib().qad_run_host(ekf._h, inputs._h, int(t0), int(n), C.byref(ekf.params), C.byref(c), acc.ctypes.data_as(_pd),
                                    R.ctypes.data_as(_pd)))
    return acc, R
