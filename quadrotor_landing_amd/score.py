"""ctypes binding of include/qle_score.h (libqle_score.so): innovation scoring for noise sweeps.

Which per-filter parameter set of a Monte-Carlo sweep is better?  Without a truth: the innovation log-likelihood of every filter over
the run, log L = -1/2 sum (NIS + log det S + 6 ln 2 pi), and per-component consistency statistics of the innovation.  One read-only
kernel per tag tick (k_score, csrc/ekf_score.hpp: the arithmetic of the gate's k_pregate with an fp64 accumulator record per filter)
in front of the unchanged tick; it never writes the mask word, so a scored run is the plain run.  `DeviceIO.scorer()` (devio.py) makes
a `Scorer` for device tensors, `BatchedRelativePoseEKF.score` (ekf.py) is the host-array form.  There is no fallback: a missing library
is an error.
"""
import ctypes as C
import math

from . import gate as _gate
from ._lib import QleDeviceView, QleInputsView, QleParams, SideLibrary
from ._observer import TagTickObserver

WORDS, SUMS = 40, 30   # QSC_WORDS, QSC_SUMS
# the words of an accumulator record: name -> (first word, count)
LAYOUT = {"n": (0, 1), "sum_nis": (1, 1), "sum_nis_sq": (2, 1), "sum_logdet": (3, 1), "n_bad": (4, 1), "n_pairs": (5, 1), "sum_nu": (6, 6),
          "sum_nu_sq": (12, 6), "sum_S_diag": (18, 6), "sum_lag": (24, 6), "nu_prev": (30, 6)}
LN_2PI = math.log(2.0 * math.pi)

_vp = C.c_void_p
_pview, _pin, _ppar = C.POINTER(QleDeviceView), C.POINTER(QleInputsView), C.POINTER(QleParams)
# every symbol include/qle_score.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "qsc_last_error": (C.c_char_p, []),
    "qsc_launch_count": (C.c_int64, []),
    "qsc_launch_census_begin": (C.c_int, []),
    "qsc_launch_census_end": (C.c_int, [C.c_char_p, C.c_int64, C.POINTER(C.c_int64)]),
    "qsc_score_tick": (C.c_int, [_pview, _pin, _ppar, _vp]),
    "qsc_run": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, _ppar, _vp]),
    "qsc_summary": (C.c_int, [_pview, _vp, _vp, _vp]),
    "qsc_run_host": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, _ppar, C.POINTER(C.c_double)]),
}

SCORE = SideLibrary("score", "QLE_SCORE_LIB", SYMBOLS, "innovation scoring", "qsc_last_error", needs_tick_library=True)
SCORE_LIB_PATH, score_lib, qcheck = SCORE.path, SCORE.load, SCORE.check


class Score:
    """The accumulators of a `Scorer` read as statistics, per filter (torch tensors on the device, or numpy arrays from
    `BatchedRelativePoseEKF.score`): n and n_bad [B] (scored innovations; ticks the filter was on but its NIS was not finite),
    nis_mean [B] (6 for a consistent filter), loglik [B] = -1/2 (sum NIS + sum log det S + 6 n ln 2 pi), var_ratio [B,6] = sum nu_k^2 /
    sum S_kk (1 for a consistent filter; the components are those of R_r and R_ang), rho1 [B,6] = sum nu_k nu_k^- / sum nu_k^2 (the
    whiteness test, 0 for a consistent filter) and nu_mean [B,6].  A filter that was never scored has NaN ratios and loglik 0."""

    def __init__(self, acc):
        """acc: [WORDS, B] float64, a torch tensor or a numpy array."""
        w = lambda name: acc[LAYOUT[name][0]:LAYOUT[name][0] + LAYOUT[name][1]]   # noqa: E731
        n = acc[0]
        self.n, self.n_bad, self.n_pairs = n, acc[4], acc[5]
        self.nis_mean = acc[1] / n
        self.loglik = -0.5 * (acc[1] + acc[3] + 6.0 * LN_2PI * n)
        self.var_ratio = (w("sum_nu_sq") / w("sum_S_diag")).T
        self.rho1 = (w("sum_lag") / w("sum_nu_sq")).T
        self.nu_mean = (w("sum_nu") / n).T


class Scorer(TagTickObserver):
    """Innovation scoring of a handle fed from device tensors (`DeviceIO.scorer()`).  Owns a zeroed accumulator tensor `acc`
    [WORDS, padded batch] (float64, include/qle_score.h) on the handle's GPU.  Every call is asynchronous and none synchronises."""
    LIB, WORDS, WHAT, RESULT, RECHECK = SCORE, WORDS, "scoring", Score, True

    def observe(self, u, z, mask=None):
        """Score the tag poses of the tick `io.tick(u, z, mask)` is about to run -- call it BEFORE that tick: packs u [B,6], z [B,7] and
        mask [B] (uint8 / bool; None = all) into the slot the tick will pack again, and adds every filter's innovation against the
        predicted state to its accumulators.  One pack and ONE launch of k_score; the state is not touched."""
        super().observe(u, z, mask)

    def _observe_tick(self, Q, view, iv):
        return Q.qsc_score_tick(C.byref(view), C.byref(iv), C.byref(self.io.ekf.params), self.acc.data_ptr())

    def run(self, seq, t0=0, n=None):
        """Ticks [t0, t0 + n) of a `DeviceSequence` (n None: to its end), scored, in ONE native call (qsc_run): what `io.run(seq, t0, n)`
        does -- state and sequence end with its bits -- with k_score in front of every tick that has a tag slot."""
        super().run(seq, t0, n)

    def _run(self, Q, seq, t0, n):
        return Q.qsc_run(self.io.ekf._h, seq.inputs._h, t0, n, C.byref(self.io.ekf.params), self.acc.data_ptr())

    def result(self):
        """The accumulators as a `Score` of device tensors [B] / [B,6]; no synchronisation."""
        return super().result()

    def summary(self, mask=None):
        """Words 0..29 of the accumulators added over the filters with mask != 0 (uint8 / bool [B]; None = all): a float64 device tensor
        [30] in the order of LAYOUT (n, sum_nis, sum_nis_sq, sum_logdet, n_bad, n_pairs, then sum_nu, sum_nu_sq, sum_S_diag, sum_lag,
        six each).  Two launches; deterministic, and additive over shards."""
        io = self.io
        io._check_mask(mask)
        Q = score_lib()
        view = io._view()
        out = io._alloc([(SUMS,)], "float64")[0]
        with io._ordered(view, self.acc, mask):
            qcheck(Q.qsc_summary(C.byref(view), self.acc.data_ptr(), None if mask is None else mask.data_ptr(), out.data_ptr()))
        return out


def run_host(ekf, inputs, t0, n):
    """qsc_run_host: ticks [t0, t0 + n) of an `InputSequence`, scored; the accumulators [WORDS, B] as a numpy array."""
    import numpy as np
    _gate.refuse_multirate(ekf.params, "scoring")
    acc = np.zeros((WORDS, ekf.batch))
    qcheck(score_lib().qsc_run_host(ekf._h, inputs._h, int(t0), int(n), C.byref(ekf.params), acc.ctypes.data_as(C.POINTER(C.c_double))))
    return acc
