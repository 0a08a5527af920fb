"""ctypes binding of include/qle_imm.h (libqle_imm.so): the banks of a handle as an interacting multiple model (IMM) estimator.

`bank.Bank.fuse` under the log-likelihoods of a `score.Scorer` is a static multiple-model estimator: the weights never forget and the
members never interact.  IMM adds a Markov transition between the modes (Pi [M,M], Pi[i][j] = P(mode i -> mode j)) with recursive mode
probabilities, and a mixing step in front of every measurement cycle that re-initialises member j from the moment-matched mixture of
all members under the mixing weights mu_{i|j} = Pi[i][j] mu_i / c_j.  `qim_mix` does the mixing in ONE launch, in place (k_imm_mix:
csrc/ekf_imm.hpp), `qim_update` the recursion logmu_j = logc_j + loglik_j - logsumexp(...) in ONE launch (k_imm_update); the likelihood is
the scorer's and the combination step is `Bank.fuse` with `logmu` as the log-weights.  `DeviceIO.imm(M, Pi)` (devio.py) makes an `Imm` for
device tensors, `BatchedRelativePoseEKF.mix_banks` (ekf.py) is the host-array form of the mixing step.  There is no fallback: a missing
library is an error.

Not provided: IMM inside `DeviceIO.run` (a C loop over a whole sequence), transition matrices per bank, multirate handles (the next
correcting tick replays from the history and would discard what was mixed into the current state), transport of P_i between tangent
spaces (first order, as `Bank.fuse`), and `lookahead` of anything fused.
"""
import ctypes as C
import math

from . import _tensors as _t
from . import gate as _gate
from ._lib import QleDeviceView, QleParams, SideLibrary
from .bank import check_members

_vp = C.c_void_p
_pview, _ppar = C.POINTER(QleDeviceView), C.POINTER(QleParams)
_pd, _pu8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
# every symbol include/qle_imm.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "qim_last_error": (C.c_char_p, []),
    "qim_launch_count": (C.c_int64, []),
    "qim_launch_census_begin": (C.c_int, []),
    "qim_launch_census_end": (C.c_int, [C.c_char_p, C.c_int64, C.POINTER(C.c_int64)]),
    "qim_mix": (C.c_int, [_pview, _ppar, C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    "qim_update": (C.c_int, [_pview, C.c_int32, _vp, _vp, _vp, C.c_double, _vp]),
    "qim_mix_host": (C.c_int, [_pview, _ppar, C.c_int32, _pd, _pd, _pu8, _pd, _pu8]),
}

IMM = SideLibrary("imm", "QLE_IMM_LIB", SYMBOLS, "the IMM mixing kernel", "qim_last_error")
IMM_LIB_PATH, imm_lib, icheck = IMM.path, IMM.load, IMM.check

ROW_SUM_TOL = 1e-12


def check_Pi(Pi, M):
    """Pi as a float64 numpy array [M,M], checked on the host: shape, finite, >= 0, rows that add to 1 within ROW_SUM_TOL.  A nested
    list, a numpy array or a tensor; anything else, or a violation, raises ValueError before any native call."""
    import numpy as np
    if hasattr(Pi, "detach"):
        Pi = Pi.detach().cpu().numpy()
    try:
        a = np.ascontiguousarray(Pi, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"Pi: expected [{M},{M}] numbers ({e})") from None
    if a.shape != (M, M):
        raise ValueError(f"Pi: expected shape ({M}, {M}), got {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError("Pi: every entry must be finite")
    if (a < 0).any():
        raise ValueError("Pi: every entry must be >= 0")
    worst = float(np.abs(a.sum(axis=1) - 1.0).max())
    if worst > ROW_SUM_TOL:
        raise ValueError(f"Pi: every row must add to 1 (worst deviation {worst:.3e})")
    return a


def check_logmu_min(v):
    v = float(v)
    if v != v:
        raise ValueError("logmu_min must not be NaN (-inf disables the floor)")
    return v


def _upload(device, a):
    """A float64 numpy array as a device tensor"""
    import torch
    t = _t.empty(device, a.shape, "float64")
    t.copy_(torch.from_numpy(a))
    return t


class Imm:
    """The banks of a `DeviceIO` as an IMM estimator: `members` consecutive filters per bank, one transition matrix `Pi` [M,M] for all
    banks (a float64 device tensor, uploaded once), the unnormalised log mode probabilities `logmu` [B] (float64 device tensor; uniform
    unless logmu0 is given) and, after a `mix`, the predicted log mode probabilities `logc` [B].  logmu_min: the floor of `update`
    against mode extinction (-inf: none).  Every call is asynchronous and none synchronises."""

    def __init__(self, io, members, Pi, logmu0=None, logmu_min=math.log(1e-12)):
        self.io = io
        B = io.ekf.batch
        self.members = check_members(members, B)
        self.banks = B // self.members
        pi = check_Pi(Pi, self.members)
        self.logmu_min = check_logmu_min(logmu_min)
        _gate.refuse_multirate(io.ekf.params, "IMM mixing")
        if logmu0 is not None and hasattr(logmu0, "data_ptr"):
            io._check(logmu0, "logmu0", (B,), ("float64",))
        self.Pi = _upload(io.ekf.device, pi)
        if logmu0 is None:
            self.logmu = _t.empty(io.ekf.device, (B,), "float64")
            self.logmu.fill_(-math.log(self.members))
        elif hasattr(logmu0, "data_ptr"):
            self.logmu = logmu0.clone()
        else:
            import numpy as np
            a = np.ascontiguousarray(logmu0, dtype=np.float64)
            if a.shape != (B,):
                raise ValueError(f"logmu0: expected shape ({B},), got {a.shape}")
            self.logmu = _upload(io.ekf.device, a)
        self.logc = None
        self._scorer = None

    def mix(self, mask=None):
        """The mixing step, in place, in ONE launch of k_imm_mix: every mixed member's record becomes the moment-matched mixture of its
        bank under mu_{i|j}.  A member counts when mask[i] != 0 (uint8 / bool [B]; None = all), it holds a state and its logmu is
        finite.  Returns (logc, mixed): the predicted log mode probabilities [B] (float64; kept as `self.logc`) and which filters were
        written [B] (uint8)."""
        io = self.io
        B = io.ekf.batch
        io._check_mask(mask)
        _gate.refuse_multirate(io.ekf.params, "IMM mixing")
        K = imm_lib()
        view = io._view()
        logc = io._alloc([(B,)], "float64")[0]
        mixed = io._alloc([(B,)], "uint8")[0]
        with io._ordered(view, self.logmu, self.Pi, mask):
            icheck(K.qim_mix(C.byref(view), C.byref(io.ekf.params), self.members, self.logmu.data_ptr(), self.Pi.data_ptr(),
                             None if mask is None else mask.data_ptr(), logc.data_ptr(), mixed.data_ptr()))
        self.logc = logc
        return logc, mixed

    def update(self, loglik, mask=None):
        """The mode-probability recursion after the members have ticked, in ONE launch of k_imm_update: logmu_j = logc_j + loglik_j -
        logsumexp over the bank, floored at logmu_min, from the `logc` of the last `mix` and loglik [B] (a float64 device tensor:
        `Scorer.result().loglik` of a one-tick scorer; 0 for a member without a tag pose this tick).  Replaces `self.logmu` and returns
        it."""
        io = self.io
        B = io.ekf.batch
        if self.logc is None:
            raise ValueError("update: there is no predicted mode probability yet (call mix first)")
        io._check(loglik, "loglik", (B,), ("float64",), align=8)
        io._check_mask(mask)
        K = imm_lib()
        view = io._view()
        logmu = io._alloc([(B,)], "float64")[0]
        with io._ordered(view, self.logc, loglik, mask):
            icheck(K.qim_update(C.byref(view), self.members, self.logc.data_ptr(), loglik.data_ptr(), None if mask is None else mask.data_ptr(),
                                self.logmu_min, logmu.data_ptr()))
        self.logmu = logmu
        return logmu

    def step(self, u, z=None, mask=None):
        """One IMM cycle around one tick.  With tag poses z [B,7] (and mask [B]: which filters have one; None = all): `mix()`, the
        tick's likelihood from a one-tick `Scorer` of its own (`reset()`, `observe(u, z, mask)`), `io.tick(u, z, mask)`, then
        `update(scorer.result().loglik)`.  Without z: `io.tick(u)`, the mode probabilities stay.  Returns what `tick` returns."""
        io = self.io
        if z is None:
            return io.tick(u)
        if self._scorer is None:
            self._scorer = io.scorer()
        self.mix()
        self._scorer.reset()
        self._scorer.observe(u, z, mask)
        out = io.tick(u, z, mask)
        self.update(self._scorer.result().loglik.contiguous())
        return out

    def fuse(self, mask=None):
        """The combination step: `io.bank(members).fuse(logmu, mask)`, a `bank.Fused`."""
        return self.io.bank(self.members).fuse(self.logmu, mask)

    def mu(self):
        """The normalised mode probabilities [B] (float64 device tensor): exp(logmu) over its bank's sum; 0 where logmu is -inf."""
        import torch
        lm = self.logmu.view(self.banks, self.members)
        top = lm.max(dim=1, keepdim=True).values
        e = torch.exp(lm - torch.where(torch.isfinite(top), top, torch.zeros_like(top)))
        s = e.sum(dim=1, keepdim=True)
        return (e / torch.where(s > 0, s, torch.ones_like(s))).reshape(-1)


def mix_host(ekf, members, logmu, Pi, mask):
    """qim_mix_host for `BatchedRelativePoseEKF.mix_banks`: (logc [B] float64, mixed [B] uint8) as numpy arrays."""
    import numpy as np
    B = ekf.batch
    M = check_members(members, B)
    pi = check_Pi(Pi, M)
    lm = np.ascontiguousarray(logmu, dtype=np.float64)
    if lm.shape != (B,):
        raise ValueError(f"logmu: expected shape ({B},), got {lm.shape}")
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    if m is not None and m.shape != (B,):
        raise ValueError(f"expected mask shape ({B},), got {m.shape}")
    _gate.refuse_multirate(ekf.params, "IMM mixing")
    view = _t.device_view(ekf)
    logc, mixed = np.empty(B), np.empty(B, np.uint8)
    icheck(imm_lib().qim_mix_host(C.byref(view), C.byref(ekf.params), M, lm.ctypes.data_as(_pd), pi.ctypes.data_as(_pd),
                                  None if m is None else m.ctypes.data_as(_pu8), logc.ctypes.data_as(_pd), mixed.ctypes.data_as(_pu8)))
    return logc, mixed
