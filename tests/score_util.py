"""Shared by test_score_cpu.py and test_gpu_score.py: the reference of innovation scoring (include/qle_score.h) -- per tag tick the dense
oracle's prediction_step followed by the numpy restatement of the innovation (gate_util.predict_then_innovation), numpy's slogdet for
log det S, and plain fp64 sums -- the sequences the tests run, and the tolerances (tests/tolerances_score.md)."""
import numpy as np

import oracle
from gate_util import TOL as GATE_TOL, predict_then_innovation
from util import meas_near, rand_imu

WORDS = 40
# the word groups the tolerances are stated for: name -> words
GROUPS = {"nis": [1, 2], "logdet": [3], "nu": list(range(6, 18)), "skk": list(range(18, 24)), "lag": list(range(24, 30))}
COUNTS = [0, 4, 5]
PREV = list(range(30, 36))

# Stated tolerances per word group (deviations() below says relative to what): tests/tolerances_score.md holds the measurements they come
# from -- at most 16 x the worst measured deviation, and never looser than the gate's own, gate_util.TOL: nis for the NIS, logdet and lag
# sums, nu for the nu and nu^2 sums, S for the S_kk sums.  "cpu": the host-compiled arithmetic (test_score_cpu.py); "gpu": k_score.
TOL = {
    "cpu": {"f64": dict(nis=5e-13, logdet=5e-15, nu=2e-13, skk=5e-15, lag=2e-13),
            "f32": dict(nis=1e-4, logdet=8e-7, nu=3e-5, skk=5e-6, lag=1e-4)},
    "gpu": {"f64": dict(nis=1e-12, logdet=5e-15, nu=5e-13, skk=1e-14, lag=8e-13),
            "f32": dict(nis=1e-4, logdet=8e-7, nu=3e-5, skk=5e-6, lag=1e-4)},
}
_CAP = {"nis": "nis", "logdet": "nis", "nu": "nu", "skk": "S", "lag": "nis"}
for _where in TOL.values():
    for _d, _t in _where.items():
        assert all(_t[g] <= GATE_TOL[_d][_CAP[g]] for g in GROUPS), "a scoring tolerance is never looser than the gate's own"


class ScoreRef:
    """The accumulators in fp64, [B, 40], with the sum of absolute terms of every word beside them (scale)."""

    def __init__(self, B):
        self.acc = np.zeros((B, WORDS))
        self.scale = np.zeros((B, WORDS))

    def add(self, nu, S, nis, on):
        """One tag tick: nu [B,6], S [B,6,6], nis [B] of the filters that are `on` [B] (bool)."""
        a, s = self.acc, self.scale
        pd = np.zeros(len(on), bool)
        logdet = np.zeros(len(on))
        for i in np.flatnonzero(on):
            if np.isfinite(S[i]).all() and np.linalg.eigvalsh(S[i]).min() > 0:
                pd[i] = True
                logdet[i] = np.linalg.slogdet(S[i])[1]
        scored = on & pd & np.isfinite(nis)
        pair = scored & (a[:, 0] >= 1)
        k = scored
        a[on & ~scored, 4] += 1
        a[pair, 5] += 1
        a[pair, 24:30] += nu[pair] * a[pair, 30:36]; s[pair, 24:30] += np.abs(nu[pair] * a[pair, 30:36])
        a[k, 0] += 1
        a[k, 1] += nis[k]; s[k, 1] += np.abs(nis[k])
        a[k, 2] += nis[k] ** 2; s[k, 2] += nis[k] ** 2
        a[k, 3] += logdet[k]; s[k, 3] += np.abs(logdet[k])
        a[k, 6:12] += nu[k]; s[k, 6:12] += np.abs(nu[k])
        a[k, 12:18] += nu[k] ** 2; s[k, 12:18] += nu[k] ** 2
        d = np.diagonal(S, axis1=1, axis2=2)
        a[k, 18:24] += d[k]; s[k, 18:24] += np.abs(d[k])
        a[k, 30:36] = nu[k]
        return scored


def deviations(acc, ref):
    """Worst deviation over the filters of accumulators acc [B,40] from a ScoreRef, per word group.  A scalar word (sum NIS, sum NIS^2,
    sum log det S) is taken relative to its own sum of absolute terms; a six-component word block (sum nu, sum nu^2, sum S_kk, the lag
    sums) relative to the block's sum of absolute terms, the six components together -- the way gate_util.rel takes nu and S relative to
    their largest element: the rounding error of one component of nu is set by the size of the pose it is the difference of, not by the
    component, and a component that happens to be small in every term would otherwise measure the conditioning of the subtraction."""
    out = {}
    for g, words in GROUPS.items():
        worst = 0.0
        for blk in ([[w] for w in words] if len(words) < 6 else [words[k:k + 6] for k in range(0, len(words), 6)]):
            sc = ref.scale[:, blk].sum(axis=1)
            live = sc > 0
            if live.any():
                worst = max(worst, float((np.abs(acc[:, blk] - ref.acc[:, blk]).max(axis=1)[live] / sc[live]).max()))
        out[g] = worst
    return out


def loglik(acc):
    """[B,40] -> the innovation log-likelihood per filter"""
    return -0.5 * (acc[:, 1] + acc[:, 3] + 6.0 * np.log(2.0 * np.pi) * acc[:, 0])


def make_sequence(rng, po, x0, P0, K, meas_ticks, pfp=None, ang=0.05, pos=0.02):
    """K ticks of IMU samples and, on meas_ticks, tag poses near the state the dense oracle predicts there (it runs the whole sequence, every
    correction included).  -> U [K,B,6], Z [M,B,7]"""
    B = x0.shape[0]
    U = np.stack([rand_imu(rng, B) for _ in range(K)])
    Z = []
    x, P = x0, P0
    ones = np.ones((1, B), np.uint8)
    for t in range(K):
        if t in meas_ticks:
            xp, _ = oracle.run_batch(po, x, P, U[t:t + 1], per_filter_params=pfp)
            Z.append(meas_near(rng, po, xp, ang=ang, pos=pos))
            x, P = oracle.run_batch(po, x, P, U[t:t + 1], Z[-1][None], ones, per_filter_params=pfp)
        else:
            x, P = oracle.run_batch(po, x, P, U[t:t + 1], per_filter_params=pfp)
    return U, np.stack(Z)


def reference_run(po, p, x0, P0, U, Z, M, meas_ticks, pfp=None, forced=None, score_from=0):
    """The scored run on the CPU: a ScoreRef over the K ticks of U, with tag poses Z [M,B,7] and masks M [M,B] on meas_ticks, stepped by
    oracle.run_batch from (x0, P0).  forced: {tick: (x, P)} replaces the state in front of those ticks (teacher forcing); the ticks in
    front of score_from are run and not scored."""
    ref = ScoreRef(x0.shape[0])
    x, P = x0, P0
    j = 0
    for t in range(U.shape[0]):
        if forced is not None and t in forced:
            x, P = forced[t]
        if t in meas_ticks:
            on = M[j] != 0
            if t >= score_from:
                nu, S, nis, _, _ = predict_then_innovation(po, p, x, P, U[t], Z[j], pfp, mask=on)
                ref.add(nu, S, nis, on)
            x, P = oracle.run_batch(po, x, P, U[t:t + 1], Z[j][None], M[j][None], per_filter_params=pfp)
            j += 1
        else:
            x, P = oracle.run_batch(po, x, P, U[t:t + 1], per_filter_params=pfp)
    return ref
