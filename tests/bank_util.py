"""Shared by the filter-bank tests (test_bank_cpu.py, test_gpu_bank.py): the truth, the construction of cases, and how a deviation is
measured.

Truth: `fuse_ref(x, P, logw, mask, M)`, a numpy float64 restatement of steps 1-5 of include/qle_bank.h with plain sums, on exactly the
values the code under test was given.  It is pinned by an independent form (test_bank_cpu.py): for banks whose members share one
quaternion the fused covariance is that of the Gaussian mixture, sum w (P + y y^T) - ybar ybar^T over the vector states.

What a deviation is relative to (`deviations`; the convention of tests/tolerances_score.md): the sum of absolute terms.  A weight is taken
relative to itself; a three-component block of the fused state (r, v, ab, wb) relative to the block's sum of absolute terms,
|x_ref| + sum w |d|, the three components together; the fused quaternion absolutely (a unit quaternion, compared up to sign: q and -q
are one attitude); a 3 x 3 block of the fused covariance relative to the block's sum of absolute terms, sum w (|P| + |c c^T|), c = d - m.
Tolerances: tests/tolerances_bank.md.
"""
import numpy as np

from util import qmul, rand_states

RECORDS = {"full15": (15, False), "full9": (9, False), "compact9": (9, True)}
# stated tolerances per dtype and word group: 8 x the worst deviation of the host-compiled arithmetic (test_bank_cpu.py), rounded up to
# one digit -- the margin covers the device's own exp / sincos and contraction.  tests/tolerances_bank.md holds the measurements.
TOL = {
    "f64": {"w": 3e-15, "x": 1e-15, "q": 2e-15, "P": 5e-15},
    "f32": {"w": 3e-15, "x": 3e-7, "q": 3e-7, "P": 4e-6},
}


def held(dtype, a):
    return a.astype(np.float32).astype(np.float64) if dtype == "f32" else np.asarray(a, np.float64)


# ---------------------------------------------------------------- quaternions (x, y, z, w), rows
def quat_norm(q):
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    return np.where(q[..., 3:4] < -0.75, -q, q)


def quat_log(q):
    m = np.linalg.norm(q[..., :3], axis=-1, keepdims=True)
    k = np.where(m < 1e-10, 2.0 / q[..., 3:4], 2.0 * np.arctan2(m, q[..., 3:4]) / np.where(m < 1e-10, 1.0, m))
    return k * q[..., :3]


def quat_exp(v):
    a = np.linalg.norm(v, axis=-1, keepdims=True)
    k = np.where(a > 1e-12, np.sin(a / 2) / np.where(a > 1e-12, a, 1.0), 0.5)
    return quat_norm(np.concatenate([v * k, np.cos(a / 2)], axis=-1))


def qconj(q):
    return q * np.array([-1.0, -1.0, -1.0, 1.0])


def box_minus(x, xr):
    """d [.., 15] = x (-) xr: plain for r, v, ab, wb; log(norm(qr^-1 (x) q)) for the attitude"""
    d = np.zeros(x.shape[:-1] + (15,))
    d[..., 0:6] = x[..., 0:6] - xr[..., 0:6]
    d[..., 6:9] = quat_log(quat_norm(qmul(qconj(xr[..., 6:10]), x[..., 6:10])))
    d[..., 9:15] = x[..., 10:16] - xr[..., 10:16]
    return d


class Fused:
    """w [B], best [G], x [G,16], P [G,n,n], and the sums of absolute terms the deviations are relative to: sx [G,15] (the attitude
    words unused), sP [G,n,n]."""


def fuse_ref(x, P, logw, mask, M):
    x, P, logw = np.asarray(x, np.float64), np.asarray(P, np.float64), np.asarray(logw, np.float64)
    B, n = x.shape[0], P.shape[1]
    assert B % M == 0
    G = B // M
    mask = np.ones(B, bool) if mask is None else np.asarray(mask) != 0
    out = Fused()
    out.w, out.best = np.zeros(B), np.full(G, -1, np.int32)
    out.x, out.P, out.sx, out.sP = np.zeros((G, 16)), np.zeros((G, n, n)), np.zeros((G, 15)), np.zeros((G, n, n))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for g in range(G):
            s = slice(g * M, (g + 1) * M)
            xb, Pb, lb = x[s], P[s], logw[s]
            valid = mask[s] & xb[:, 6:10].any(axis=1) & np.isfinite(lb)
            if not valid.any():
                continue
            lmax = lb[valid].max()
            ref = int(np.flatnonzero(valid & (lb == lmax))[0])
            out.best[g] = g * M + ref
            wt = np.where(valid, np.exp(np.where(valid, lb, 0.0) - lmax), 0.0)
            w = wt / wt.sum()
            out.w[s] = w
            v = np.flatnonzero(valid)
            d = box_minus(xb[v], xb[ref][None, :])
            m = (w[v, None] * d).sum(axis=0)
            out.x[g, 0:6] = xb[ref, 0:6] + m[0:6]
            out.x[g, 10:16] = xb[ref, 10:16] + m[9:15]
            out.x[g, 6:10] = quat_norm(qmul(xb[ref, 6:10][None, :], quat_exp(m[None, 6:9])))[0]
            out.sx[g] = (w[v, None] * np.abs(d)).sum(axis=0)
            out.sx[g, 0:6] += np.abs(xb[ref, 0:6]); out.sx[g, 9:15] += np.abs(xb[ref, 10:16])
            c = (d - m)[:, :n]
            cc = c[:, :, None] * c[:, None, :]
            out.P[g] = (w[v, None, None] * (Pb[v] + cc)).sum(axis=0)
            out.sP[g] = (w[v, None, None] * (np.abs(Pb[v]) + np.abs(cc))).sum(axis=0)
    return out


def mixture_cov(x, P, w):
    """The independent form for members that share one quaternion: sum w (P + y y^T) - ybar ybar^T, y = (r, v, 0, ab, wb), and the sum of
    absolute terms."""
    n = P.shape[1]
    y = np.zeros((x.shape[0], 15)); y[:, 0:6] = x[:, 0:6]; y[:, 9:15] = x[:, 10:16]
    y = y[:, :n]
    yb = (w[:, None] * y).sum(axis=0)
    yy = y[:, :, None] * y[:, None, :]
    cov = (w[:, None, None] * (P + yy)).sum(axis=0) - np.outer(yb, yb)
    scale = (w[:, None, None] * (np.abs(P) + np.abs(yy))).sum(axis=0) + np.abs(np.outer(yb, yb))
    return cov, scale


# ---------------------------------------------------------------- cases
def make_case(rng, M, G, n, dtype, x=None, P=None, empty_bank=True, spread=0.15, specials=True):
    """(x, P, logw, mask) of G banks of M members, rounded to what a handle of `dtype` holds: states and covariances from
    util.rand_states(cov_scale=0.05) (or x, P as given: the special members are then applied to them), the members' attitudes within
    2 * spread = 0.3 rad of one another, logw uniform in [-3, 0] (every weight above 1e-3 / M, no bank decided by one member).  The
    special members: one masked, one without a state, one with logw = -inf, one stored as -q of its neighbour -- all four in every bank
    with M >= 8; a bank of 2 takes one of them in turn (bank g: kind g % 5, 4 = none), so that a valid member is left.  The last bank
    is all-invalid (empty_bank): its members are masked, stateless or of non-finite logw in turn.  specials=False: no special member."""
    B = M * G
    if x is None:
        x, P = rand_states(rng, B, n, cov_scale=0.05)
        qb = x[::M, 6:10].repeat(M, axis=0)                                   # the bank's attitude, each member within `spread` of it
        ax = rng.normal(size=(B, 3)); ax /= np.linalg.norm(ax, axis=1, keepdims=True)
        x[:, 6:10] = qmul(qb, quat_exp(ax * rng.uniform(0.0, spread, size=(B, 1))))
    else:
        x, P = x.copy(), P.copy()
    logw = rng.uniform(-3.0, 0.0, size=B)
    mask = np.ones(B, np.uint8)

    def special(i, kind):
        if kind == 0:
            mask[i] = 0
        elif kind == 1:
            x[i] = 0.0
        elif kind == 2:
            logw[i] = -np.inf
        elif kind == 3:
            x[i, 6:10] = -x[i - 1 if i % M else i + 1, 6:10]                  # the neighbour's attitude, stored as -q

    for g in range(G if specials else 0):
        if M >= 8:
            for kind, l in zip((3, 0, 1, 2), rng.permutation(M)[:4]):             # -q first: of the neighbour's attitude as drawn
                special(g * M + int(l), kind)
        elif g % 5 < 4:
            special(g * M + int(rng.integers(M)), g % 5)
    if empty_bank:
        for l in range(M):
            i = (G - 1) * M + l
            special(i, l % 3)
            if l % 3 == 2 and l % 2:
                logw[i] = np.nan
    return held(dtype, x), held(dtype, P), logw, mask


# ---------------------------------------------------------------- deviations
def _rel(dev, scale):
    """dev / scale, 0 where both are 0, inf where only the scale is (or the deviation is not finite)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(scale > 0, dev / np.where(scale > 0, scale, 1.0), np.where(dev == 0, 0.0, np.inf))
    return float(np.where(np.isfinite(r), r, np.inf).max()) if r.size else 0.0


def deviations(w, xf, Pf, ref):
    """{"w", "x", "q", "P"}: the worst deviation of each word group from the truth `ref` (a Fused), over the banks that are not empty"""
    live = ref.best >= 0
    n = ref.P.shape[1]
    out = {"w": _rel(np.abs(w - ref.w), ref.w)}
    vec = [0, 3, 9, 12]                                                        # r, v, ab, wb in the 15 words of d
    word = {0: 0, 3: 3, 9: 10, 12: 13}
    dx = np.stack([np.abs(xf[live, word[b]:word[b] + 3] - ref.x[live, word[b]:word[b] + 3]).max(axis=1) for b in vec], axis=1)
    sx = np.stack([ref.sx[live, b:b + 3].sum(axis=1) for b in vec], axis=1)
    out["x"] = _rel(dx, sx)
    q, qr = xf[live, 6:10], ref.x[live, 6:10]
    out["q"] = float(np.minimum(np.abs(q - qr).max(axis=1), np.abs(q + qr).max(axis=1)).max()) if live.any() else 0.0
    nb = n // 3
    dP = np.abs(Pf[live] - ref.P[live]).reshape(-1, nb, 3, nb, 3).max(axis=(2, 4))
    sP = ref.sP[live].reshape(-1, nb, 3, nb, 3).sum(axis=(2, 4))
    out["P"] = _rel(dP, sP)
    return out
