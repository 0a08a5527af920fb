"""Shared by test_adapt_cpu.py and test_gpu_adapt.py: the reference of noise adaptation (include/qle_adapt.h) -- per tag tick the dense
oracle's prediction_step followed by the numpy restatement of the innovation (gate_util.predict_then_innovation), N as
innovation_util.innovation_ref builds it, a_k = n_k^T S^-1 nu and c_k = n_k^T S^-1 n_k by numpy.linalg.solve, plain fp64 sums, and the
apply formula in numpy -- and the tolerances (tests/tolerances_adapt.md)."""
import numpy as np

import oracle
from gate_util import TOL as GATE_TOL, predict_then_innovation
from oracle.ekf_np import rot, skew

WORDS = 24
# the word groups the tolerances are stated for: name -> words (six-word blocks, each relative to the block's sum of absolute terms)
GROUPS = {"rhat": list(range(2, 8)), "a2": list(range(8, 14)), "c": list(range(14, 20))}
COUNTS = [0, 1, 20, 21, 22]

# Stated tolerances per word group: tests/tolerances_adapt.md holds the measurements they come from -- at most 16 x the worst measured
# deviation, and never looser than the gate's own for NIS (gate_util.TOL: a and c are quadratic forms in S^-1, as NIS is).  "cpu": the
# host-compiled arithmetic (test_adapt_cpu.py); "gpu": k_adapt_observe.
TOL = {
    "cpu": {"f64": dict(rhat=3e-14, a2=5e-13, c=1.5e-14), "f32": dict(rhat=8e-6, a2=1e-4, c=2e-5)},
    "gpu": {"f64": dict(rhat=2e-14, a2=8e-13, c=8e-15), "f32": dict(rhat=7e-6, a2=1e-4, c=2e-6)},
}
for _where in TOL.values():
    for _d, _t in _where.items():
        assert all(_t[g] <= GATE_TOL[_d]["nis"] for g in GROUPS), "an adaptation tolerance is never looser than the gate's own for NIS"
# the applied R against the numpy apply of the same accumulators: relative, where not clamped (clamped: equal to the rounded bound)
APPLY_TOL = {"f64": 4e-16, "f32": float(np.finfo(np.float32).eps)}


def noise_jacobian(p, x):
    """N [6,6] of one filter at state x, as innovation_util.innovation_ref builds it"""
    Cc = rot(x[6:10])
    N = np.zeros((6, 6))
    N[0:3, 0:3] = -Cc @ p.C_vc
    N[3:6, 3:6] = p.C_vc
    if p.direct_orien_method:
        N[0:3, 3:6] = skew(x[0:3])
    return N


class AdaptRef:
    """The accumulators in fp64, [B, 24], with the sum of absolute terms of every sum word beside them (scale)."""

    def __init__(self, B):
        self.acc = np.zeros((B, WORDS))
        self.scale = np.zeros((B, WORDS))
        self.min_sample = np.inf

    def add(self, p, nu, S, nis, x_pred, R, on, chi2_max=np.inf):
        """One tag tick: nu [B,6], S [B,6,6], nis [B] against the predicted states x_pred [B,16], with noise R [B,6], of the filters
        that are `on` [B] (bool)."""
        a, s = self.acc, self.scale
        for i in np.flatnonzero(on):
            ok = np.isfinite(S[i]).all() and np.isfinite(nu[i]).all() and np.isfinite(nis[i]) and np.linalg.eigvalsh(S[i]).min() > 0
            if ok:
                N = noise_jacobian(p, x_pred[i])
                ak = N.T @ np.linalg.solve(S[i], nu[i])
                ck = np.einsum("mk,mk->k", N, np.linalg.solve(S[i], N))
                rhat = R[i] + R[i] ** 2 * (ak ** 2 - ck)
                ok = np.isfinite(rhat).all()
            if not ok:
                a[i, 1] += 1
            elif not nis[i] <= chi2_max:
                a[i, 22] += 1
            else:
                self.min_sample = min(self.min_sample, float(rhat.min()))
                a[i, 0] += 1; a[i, 20] += 1
                a[i, 2:8] += rhat; s[i, 2:8] += np.abs(R[i]) + R[i] ** 2 * ak ** 2 + R[i] ** 2 * ck
                a[i, 8:14] += ak ** 2; s[i, 8:14] += ak ** 2
                a[i, 14:20] += ck; s[i, 14:20] += np.abs(ck)


def deviations(acc, ref, rows=None):
    """Worst deviation over the filters (rows: a subset) of accumulators acc [B,24] from an AdaptRef, per word group: each six-word
    block relative to the block's sum of absolute terms (score_util.deviations' rule for component blocks)."""
    rows = np.arange(acc.shape[0]) if rows is None else rows
    out = {}
    for g, blk in GROUPS.items():
        sc = ref.scale[rows][:, blk].sum(axis=1)
        live = sc > 0
        out[g] = float((np.abs(acc[rows][:, blk] - ref.acc[rows][:, blk]).max(axis=1)[live] / sc[live]).max()) if live.any() else 0.0
    return out


def apply_ref(acc, R, gain, n_min, lo, hi, dtype):
    """The M-step in numpy on accumulators acc [B,24] and noise R [B,6]: -> (acc after, R after, applied [B] bool, clamped [B,6] bool).
    R after is rounded once to the compute dtype."""
    acc, R = acc.copy(), R.copy()
    applied = acc[:, 0] >= n_min
    with np.errstate(divide="ignore", invalid="ignore"):
        v = R + gain * (acc[:, 2:8] / acc[:, 0:1] - R)
    clamped = (v < lo) | (v > hi)
    v = np.minimum(np.maximum(v, lo), hi)
    if dtype == "f32":
        v = v.astype(np.float32).astype(np.float64)
    R[applied] = v[applied]
    acc[applied, 0] = 0
    acc[applied, 2:20] = 0
    acc[applied, 21] += 1
    return acc, R, applied, clamped & applied[:, None]


def apply_error(R_got, R_want, clamped):
    """(worst relative deviation of the components that are not clamped, whether every clamped one is equal)"""
    free = ~clamped
    rel = float((np.abs(R_got - R_want)[free] / np.abs(R_want)[free]).max()) if free.any() else 0.0
    return rel, bool((R_got[clamped] == R_want[clamped]).all())


def reference_run(po, p, x0, P0, U, Z, M, meas_ticks, pfp, window, gain, n_min, lo, hi, dtype, chi2_max=np.inf, forced=None, gpu=None,
                  trace=None):
    """The adapted run on the CPU over the K ticks of U, with tag poses Z [M,B,7] and masks M [M,B] on meas_ticks, stepped by
    oracle.run_batch from (x0, P0) with per_filter_params carrying the current R, an apply after every window-th tag tick.
    forced: {tick: (x, P)} replaces the state in front of those ticks (teacher forcing).  gpu: {apply index: (acc before it [B,24],
    R after it [B,6])} -- the apply is then taken on the device's own accumulators, so that it is checked on its own and not through
    accumulated drift, and the run goes on from the device's R.  trace: a list that receives, per tag tick, (x, P, pfp, nis) in front
    of it.  A state handed on is rounded to the compute dtype.
    -> (AdaptRef at the end, [per apply: (AdaptRef before it (a copy), R the numpy apply gives, applied, clamped)])"""
    ref = AdaptRef(x0.shape[0])
    pfp = pfp.copy()
    x, P = x0, P0
    j, applies = 0, []
    for t in range(U.shape[0]):
        if forced is not None and t in forced:
            x, P = forced[t]
        if t in meas_ticks:
            on = (M[j] != 0) & ~(x[:, 6:10] == 0).all(axis=1)   # a filter without a state is not on
            if dtype == "f32":
                x, P = x.astype(np.float32).astype(np.float64), P.astype(np.float32).astype(np.float64)
            nu, S, nis, xp, _ = predict_then_innovation(po, p, x, P, U[t], Z[j], pfp, mask=on)
            if trace is not None:
                trace.append((x, P, pfp.copy(), nis))
            ref.add(p, nu, S, nis, xp, pfp[:, 18:24], on, chi2_max)
            m = (on & np.isfinite(Z[j]).all(axis=1)).astype(np.uint8)
            x, P = oracle.run_batch(po, x, P, U[t:t + 1], np.nan_to_num(Z[j])[None], m[None], per_filter_params=pfp)
            j += 1
            if j % window == 0:
                before = AdaptRef(0)
                before.acc, before.scale = ref.acc.copy(), ref.scale.copy()
                src = ref.acc if gpu is None else gpu[len(applies)][0]
                acc_after, R_after, applied, clamped = apply_ref(src, pfp[:, 18:24], gain, n_min, lo, hi, dtype)
                applies.append((before, R_after, applied, clamped))
                # the reference's own window closes where the device's did (counts are exact: the same filters)
                ref.acc[applied, 0] = 0; ref.acc[applied, 2:20] = 0; ref.acc[applied, 21] += 1
                ref.scale[applied, 2:20] = 0
                pfp[:, 18:24] = R_after if gpu is None else gpu[len(applies) - 1][1]
        else:
            x, P = oracle.run_batch(po, x, P, U[t:t + 1], per_filter_params=pfp)
    return ref, applies
