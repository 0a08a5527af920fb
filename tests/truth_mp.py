"""The correction step as a measurement model, in mpmath at 80 digits: a truth that is not a restatement of correction_step.

Not a test.  From the project this module takes only what the reference twin's goldens already pin:
  * the frame chain of the direct observation (relative_pose_EKF.cpp:431-438): q_obs = norm(conj(q_vc q_ct)),
    r_obs = -C(q_obs) (C_vc r_c_tc + r_v_cv);
  * quaternion_norm with its w >= -0.75 cover, quaternion_exp and quaternion_log (closed forms, no small-angle branches; an angle of
    exactly zero is the only special case), the Hamilton product and toRotationMatrix (x, y, z, w).
The Jacobian G, the conventional position observation and the place of the flip are NOT typed in from oracle/ or csrc/:

  model.  A tag pose z = (r_c_tc, q_ct) seen from a true state x_true is synth(x_true), the pose the direct observation maps back onto
    x_true.  The residual of a state x against z is delta_y = (r_obs - r, log(norm(conj(q) q_obs))).  The conventional position
    observation is, by definition of the method, the direct one evaluated with the state's attitude in place of the observed one.
  derivatives (central differences in mpmath, step 1e-30, truncation 1e-60, rounding 1e-50):
    G       = d residual(x, synth(x [+] dx)) / d dx at dx = 0                      -- every block, both methods;
    N[:,0:3] = d residual(x, synth(x) + (n_r, 0)) / d n_r at n_r = 0               -- the position-noise columns.
  stated (the reference's modelling choice, as the twin-pinned direct form has it): the angle-noise columns N[3:6,3:6] = C_vc and
    N[0:3,3:6] = [r]x in the direct method, 0 in the conventional one.

The reference's G is the model's derivative on the unit sphere: for a stored quaternion of norm s the two differ by O(1 - s^2), so the
fixture's state quaternions are float32 values whose norm is 1 to ~1e-15 (tests/golden/make_linearisation_truth.py).

correct() is the textbook step on these: S = G P G^T + N R N^T, K = P G^T S^-1, P_hat = (I - K G) P, injection q [*] exp(dx_theta) then
quaternion_norm, bias words zero when est_bias = 0; everything is rounded to float64 at the very end.
"""
import mpmath
import numpy as np

mp = mpmath.mp.clone()
mp.dps = 80
mpf = mp.mpf
STEP = mpf(10) ** -30
W_COVER = mpf(-3) / 4                      # quaternion_helper.cpp:61-73: q -> -q when w < -0.75
THETA_STAR = 2 * mp.acos(W_COVER)          # the rotation angle at which the cover flips: 4.8378...


def vec(a):
    return [mpf(float(v)) for v in np.asarray(a, dtype=np.float64).reshape(-1)]


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [aw * bx + bw * ax + ay * bz - az * by,
            aw * by + bw * ay + az * bx - ax * bz,
            aw * bz + bw * az + ax * by - ay * bx,
            aw * bw - ax * bx - ay * by - az * bz]


def qconj(q):
    return [-q[0], -q[1], -q[2], q[3]]


def unit(q):
    n = mp.sqrt(mp.fsum(c * c for c in q))
    return [c / n for c in q]


def quaternion_norm(q):
    q = unit(q)
    return [-c for c in q] if q[3] < W_COVER else q


def quaternion_exp(v):
    n = mp.sqrt(mp.fsum(c * c for c in v))
    if n == 0:
        return [mpf(0), mpf(0), mpf(0), mpf(1)]
    s = mp.sin(n / 2) / n
    return quaternion_norm([v[0] * s, v[1] * s, v[2] * s, mp.cos(n / 2)])


def quaternion_log(q):
    m = mp.sqrt(mp.fsum(c * c for c in q[:3]))
    if m == 0:
        return [mpf(0)] * 3
    s = 2 * mp.atan2(m, q[3]) / m
    return [s * c for c in q[:3]]


def rot(q):
    x, y, z, w = q
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]


def mv(A, v):
    return [mp.fdot(row, v) for row in A]


def mm(A, B):
    Bt = list(zip(*B))
    return [[mp.fdot(row, col) for col in Bt] for row in A]


def tr(A):
    return [list(r) for r in zip(*A)]


class Params:
    """q_vc (normalised as relative_pose_EKF.cpp:121 does), C_vc, r_v_cv, the number of error states."""

    def __init__(self, est_bias, q_vc, r_v_cv):
        self.est_bias = int(est_bias)
        self.n = 15 if est_bias else 9
        self.q_vc = quaternion_norm(vec(q_vc))
        self.C_vc = rot(self.q_vc)
        self.r_v_cv = vec(r_v_cv)


def boxplus(x, dx):
    """x [+] dx: additive except the attitude, q [*] exp(dx_theta); words a 9-state dx does not reach stay."""
    out = list(x)
    for i in range(3):
        out[i] = x[i] + dx[i]
        out[3 + i] = x[3 + i] + dx[3 + i]
    out[6:10] = qmul(x[6:10], quaternion_exp(dx[6:9]))
    for i in range(9, len(dx)):
        out[i + 1] = x[i + 1] + dx[i]
    return out


def synth(p, x_true):
    """The noise-free tag pose (r_c_tc [3], q_ct [4]) that the direct observation maps back onto x_true."""
    q = unit(x_true[6:10])
    q_ct = qmul(qconj(p.q_vc), qconj(q))
    t = [-a - b for a, b in zip(mv(tr(rot(q)), x_true[0:3]), p.r_v_cv)]
    return mv(tr(p.C_vc), t), q_ct


def residual(p, direct, x, z, ws=None):
    """delta_y [6] of state x against the tag pose z = (r_c_tc, q_ct); ws, if a list, receives the two w that quaternion_norm inspects."""
    r_c, q_ct = z
    raw = unit(qconj(qmul(p.q_vc, q_ct)))
    q_obs = quaternion_norm(raw)
    attitude = q_obs if direct else x[6:10]
    lever = [a + b for a, b in zip(mv(p.C_vc, r_c), p.r_v_cv)]
    r_obs = [-c for c in mv(rot(attitude), lever)]
    dq_raw = unit(qmul(qconj(x[6:10]), q_obs))
    if ws is not None:
        ws[:] = [raw[3], dq_raw[3]]
    return [a - b for a, b in zip(r_obs, x[0:3])] + quaternion_log(quaternion_norm(dq_raw))


def _central(f, m):
    """Columns d f / d e_k, k < m, of a function of an m-vector, at zero -> rows [len(f)][m]."""
    cols = []
    for k in range(m):
        d = [mpf(0)] * m
        d[k] = STEP
        hi = f(d)
        d[k] = -STEP
        lo = f(d)
        cols.append([(a - b) / (2 * STEP) for a, b in zip(hi, lo)])
    return tr(cols)


def G(p, direct, x):
    return _central(lambda dx: residual(p, direct, x, synth(p, boxplus(x, dx))), p.n)


def N(p, direct, x):
    r_c, q_ct = synth(p, x)
    Nr = _central(lambda d: residual(p, direct, x, ([a + b for a, b in zip(r_c, d)], q_ct)), 3)
    r = x[0:3]
    skew = [[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]]
    out = [row + [mpf(0)] * 3 for row in Nr]
    for i in range(3):
        for j in range(3):
            out[i][3 + j] = mpf(skew[i][j]) if direct else mpf(0)
            out[3 + i][3 + j] = p.C_vc[i][j]
    return out


def R_k(p, direct, x, R):
    Nk = N(p, direct, x)
    return mm([[a * r for a, r in zip(row, R)] for row in Nk], tr(Nk))


def f64(a):
    return np.array([[float(v) for v in row] for row in a]) if isinstance(a[0], (list, tuple)) else np.array([float(v) for v in a])


def correct(p, direct, x, P, z, Rs):
    """One correction of state x [16] / covariance P [n,n] with tag pose z [7], for each noise vector of Rs (a list of [6]).
    -> (nu [6], w_obs, w_dq, [dict(S, nis, x_hat, P_hat) per R]), float64."""
    n = p.n
    x = vec(x)
    P = [vec(row) for row in np.asarray(P, dtype=np.float64).reshape(n, n)]
    z = vec(z)
    ws = []
    nu = residual(p, direct, x, (z[0:3], z[3:7]), ws)
    Gk = G(p, direct, x)
    Nk = N(p, direct, x)
    PGt = mm(P, tr(Gk))
    GPGt = mm(Gk, PGt)
    out = []
    for R in Rs:
        R = vec(R)
        Rk = mm([[a * r for a, r in zip(row, R)] for row in Nk], tr(Nk))
        S = [[a + b for a, b in zip(ra, rb)] for ra, rb in zip(GPGt, Rk)]
        Sinv = (mp.matrix(S) ** -1).tolist()
        K = mm(PGt, Sinv)
        KG = mm(K, Gk)
        ImKG = [[(1 if i == j else 0) - KG[i][j] for j in range(n)] for i in range(n)]
        P_hat = mm(ImKG, P)
        dx = mv(K, nu)
        xh = boxplus(x, dx)
        xh[6:10] = quaternion_norm(xh[6:10])
        if not p.est_bias:
            xh[10:16] = [mpf(0)] * 6
        out.append(dict(S=f64(S), nis=float(mp.fdot(nu, mv(Sinv, nu))), x_hat=f64(xh), P_hat=f64(P_hat)))
    return f64(nu), float(ws[0]), float(ws[1]), out
