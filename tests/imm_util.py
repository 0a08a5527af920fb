"""Shared by the IMM tests (test_imm_cpu.py, test_gpu_imm.py): the truth, the construction of cases, and how a deviation is measured.

Truth: `mix_ref(x, P, logmu, Pi, mask, M)` and `update_ref(logc, loglik, mask, logmu_min, M)`, numpy float64 restatements of the
arithmetic of include/qle_imm.h with plain sums, on exactly the values the code under test was given.  `mix_ref` is pinned on the CPU
(test_imm_cpu.py) by forms that do not share its code: conservation of the first two moments under a row-stochastic Pi, a rank-one Pi
against `bank_util.fuse_ref`, and an identity Pi.

What a deviation is relative to (`deviations`; the convention of bank_util.py and tests/tolerances_bank.md): a three-component block
of a mixed state (r, v, ab, wb) relative to the block's sum of absolute terms, |x_j| + sum mu_{i|j} |d_ij|; the mixed quaternion
absolutely, up to sign; a 3 x 3 block of a mixed covariance relative to the block's sum of absolute terms,
sum mu_{i|j} (|P_i| + |c c^T|), c = d_ij - m_j; log c_j relative to itself.  Only mixed members are measured: every other record is
compared by its bits.  Tolerances: tests/tolerances_imm.md.
"""
import numpy as np

import bank_util as bu
from util import qmul

RECORDS = bu.RECORDS
SHAPES = [(2, 70), (8, 11), (64, 3)]   # (M, G) of tests/test_gpu_bank.py: a ragged last tile, banks beside an unused half tile, a bank per tile
# stated tolerances per dtype and word group: 8 x the worst deviation of the host-compiled arithmetic from `mix_ref`
# (test_imm_cpu.py, at SHAPES), rounded up to one digit -- the margin covers the device's own exp / log / sincos / atan2 and
# contraction.  tests/tolerances_imm.md holds the measurements.
TOL = {
    "f64": {"logc": 7e-15, "x": 3e-15, "q": 2e-15, "P": 3e-15},
    "f32": {"logc": 7e-15, "x": 4e-7, "q": 4e-7, "P": 3e-6},
}
# update: logmu = t - (tmax + log sum exp(t - tmax)), t = logc + loglik.  The deviation is taken relative to |logc| + |loglik| + |lse|, the sum
# of absolute terms: one rounding each for t, t - tmax, the sum of M terms (log2 M levels of a tree against a plain sum), tmax + log(.) and
# the last difference, and an exp and a log of at most 2 ulp each (condition number <= 1 against that scale) -- under 16 roundings of 2^-53
# for M <= 64.  Stated from that count, not from a measurement.
TOL_UPDATE = 16 * 2.0 ** -53


# ---------------------------------------------------------------- truth
class Mixed:
    """logc [B], mixed [B] (bool), x [B,16], P [B,n,n] (an unmixed member: its own words), c [B] (0 where logc = -inf), and the sums of
    absolute terms the deviations are relative to: sx [B,15] (the attitude words unused), sP [B,n,n]."""


def mode_probabilities(valid, logmu):
    """mu [M] of one bank: the weights of bank_util.fuse_ref, 0 for an invalid member"""
    mu = np.zeros(len(logmu))
    if valid.any():
        lmax = logmu[valid].max()
        wt = np.where(valid, np.exp(np.where(valid, logmu, 0.0) - lmax), 0.0)
        mu = wt / wt.sum()
    return mu


def mix_ref(x, P, logmu, Pi, mask, M):
    x, P, logmu, Pi = (np.asarray(a, np.float64) for a in (x, P, logmu, Pi))
    B, n = x.shape[0], P.shape[1]
    assert B % M == 0 and Pi.shape == (M, M)
    mask = np.ones(B, bool) if mask is None else np.asarray(mask) != 0
    out = Mixed()
    out.logc, out.mixed, out.c = np.full(B, -np.inf), np.zeros(B, bool), np.zeros(B)
    out.x, out.P, out.sx, out.sP = x.copy(), P.copy(), np.zeros((B, 15)), np.zeros((B, n, n))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for g in range(B // M):
            s = slice(g * M, (g + 1) * M)
            xb, Pb, lb = x[s], P[s], logmu[s]
            valid = mask[s] & xb[:, 6:10].any(axis=1) & np.isfinite(lb)
            mu = mode_probabilities(valid, lb)
            for j in np.flatnonzero(valid):
                c = float((Pi[valid, j] * mu[valid]).sum())
                if not (np.isfinite(c) and c > 0):
                    continue
                out.c[g * M + j], out.logc[g * M + j] = c, np.log(c)
                w = np.where(valid, Pi[:, j] * mu / c, 0.0)
                take = np.flatnonzero(w > 0)
                if not (take != j).any():
                    continue
                w = w[take]
                d = bu.box_minus(xb[take], xb[j][None, :])
                m = (w[:, None] * d).sum(axis=0)
                k = g * M + j
                out.mixed[k] = True
                out.x[k, 0:6] = xb[j, 0:6] + m[0:6]
                out.x[k, 10:16] = xb[j, 10:16] + m[9:15]
                out.x[k, 6:10] = bu.quat_norm(qmul(xb[j, 6:10][None, :], bu.quat_exp(m[None, 6:9])))[0]
                out.sx[k] = (w[:, None] * np.abs(d)).sum(axis=0)
                out.sx[k, 0:6] += np.abs(xb[j, 0:6]); out.sx[k, 9:15] += np.abs(xb[j, 10:16])
                cc = (d - m)[:, :n]
                cc = cc[:, :, None] * cc[:, None, :]
                out.P[k] = (w[:, None, None] * (Pb[take] + cc)).sum(axis=0)
                out.sP[k] = (w[:, None, None] * (np.abs(Pb[take]) + np.abs(cc))).sum(axis=0)
    return out


def update_ref(logc, loglik, mask, logmu_min, M):
    """(logmu [B], scale [B]): the recursion with plain sums, and |logc| + |loglik| + |lse| (what a deviation is relative to)"""
    logc, loglik = np.asarray(logc, np.float64), np.asarray(loglik, np.float64)
    B = logc.shape[0]
    mask = np.ones(B, bool) if mask is None else np.asarray(mask) != 0
    out, scale = np.full(B, -np.inf), np.ones(B)
    with np.errstate(invalid="ignore", divide="ignore"):
        for g in range(B // M):
            s = slice(g * M, (g + 1) * M)
            ok = mask[s] & np.isfinite(logc[s])
            t = np.where(ok & ~np.isnan(loglik[s]), logc[s] + np.where(np.isnan(loglik[s]), 0.0, loglik[s]), -np.inf)
            live = t > -np.inf
            v = np.full(M, -np.inf)
            if live.any():
                tmax = t[live].max()
                lse = tmax + np.log(np.exp(t[live] - tmax).sum())
                v[live] = t[live] - lse
                scale[s][live] = np.abs(logc[s][live]) + np.abs(loglik[s][live]) + abs(lse)
            out[s] = np.where(ok, np.maximum(v, logmu_min), -np.inf)
    return out, scale


# ---------------------------------------------------------------- cases
def make_Pi(rng, M):
    """A random row-stochastic matrix with one exact zero per row: on the diagonal for M = 2 (the swap: every member takes the other's
    place, and no c_j is a sum that rounds to 1), at a random column else.  Rows add to 1 within a rounding."""
    Pi = rng.uniform(0.05, 1.0, size=(M, M))
    for i in range(M):
        Pi[i, i if M == 2 else int(rng.integers(M))] = 0.0
    return Pi / Pi.sum(axis=1, keepdims=True)


def make_case(rng, M, G, n, dtype, **kw):
    """(x, P, logmu, mask, Pi): bank_util.make_case (per bank one masked member, one without a state, one with logmu = -inf, one stored
    as -q; the last bank all-invalid) and a transition matrix of make_Pi."""
    x, P, logmu, mask = bu.make_case(rng, M, G, n, dtype, **kw)
    return x, P, logmu, mask, make_Pi(rng, M)


# ---------------------------------------------------------------- deviations
def deviations(logc, xm, Pm, ref):
    """{"logc", "x", "q", "P"}: the worst deviation of each word group from the truth `ref` (a Mixed), over the mixed members (logc: over
    the members whose logc is finite)"""
    live = ref.mixed
    n = ref.P.shape[1]
    fin = np.isfinite(ref.logc)
    out = {"logc": bu._rel(np.abs(logc[fin] - ref.logc[fin]), np.abs(ref.logc[fin]))}
    vec, word = [0, 3, 9, 12], {0: 0, 3: 3, 9: 10, 12: 13}                     # r, v, ab, wb in the 15 words of d
    dx = np.stack([np.abs(xm[live, word[b]:word[b] + 3] - ref.x[live, word[b]:word[b] + 3]).max(axis=1) for b in vec], axis=1)
    sx = np.stack([ref.sx[live, b:b + 3].sum(axis=1) for b in vec], axis=1)
    out["x"] = bu._rel(dx, sx)
    q, qr = xm[live, 6:10], ref.x[live, 6:10]
    out["q"] = float(np.minimum(np.abs(q - qr).max(axis=1), np.abs(q + qr).max(axis=1)).max()) if live.any() else 0.0
    nb = n // 3
    dP = np.abs(Pm[live] - ref.P[live]).reshape(-1, nb, 3, nb, 3).max(axis=(2, 4))
    sP = ref.sP[live].reshape(-1, nb, 3, nb, 3).sum(axis=(2, 4))
    out["P"] = bu._rel(dP, sP)
    return out


def update_case(rng, M, G):
    """(logc, loglik, mask) with the members the recursion treats specially: per bank a loglik of -inf, a NaN one, a masked member and
    a logc of -inf (M >= 8: all four; M = 2: one in turn), loglik otherwise spread over tens of nats; the last bank has no member left."""
    B = M * G
    logc = np.log(rng.dirichlet(np.ones(M), size=G)).reshape(B)
    loglik = rng.uniform(-40.0, 5.0, size=B)
    mask = np.ones(B, np.uint8)
    for g in range(G - 1):
        lanes = rng.permutation(M)[:4] if M >= 8 else [int(rng.integers(M))] * 4
        for kind, l in enumerate(lanes):
            if M < 8 and kind != g % 5:
                continue
            i = g * M + int(l)
            if kind == 0:
                loglik[i] = -np.inf
            elif kind == 1:
                loglik[i] = np.nan
            elif kind == 2:
                mask[i] = 0
            else:
                logc[i] = -np.inf
    mask[-M::2] = 0
    logc[-M + 1::2] = -np.inf
    return logc, loglik, mask
