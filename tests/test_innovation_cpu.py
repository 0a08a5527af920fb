"""Innovation diagnostics and the chi-square gate, host side.

innovation_util.innovation_ref is the numpy restatement the GPU tests (test_gpu_innovation.py) check the engine against: the first half of
oracle/ekf_np.correction_step (relative_pose_EKF.cpp:417-475) -- the innovation delta_y, G, N, R_k = N R N^T, S = G P G^T + R_k --
and NIS = delta_y^T S^-1 delta_y.  The tests here hold it to correction_step itself and check the ctypes binding of the new entry points.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
from oracle import ekf_np
from innovation_util import innovation_ref
from oracle.ekf_np import qmul, quaternion_exp, quaternion_norm
from quadrotor_landing_amd import _lib
from util import meas_near, rand_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("est_bias", [1, 0])
@pytest.mark.parametrize("direct", [1, 0])
def test_restatement_reproduces_correction_step(direct, est_bias):
    """K = P G^T S^-1 from the restatement gives correction_step's posterior (x and P) to 1e-12."""
    po = oracle.make_params(update_freq=400.0, direct_orien_method=direct, est_bias=est_bias,
                            r_v_cv=[0.06036412, -0.00145196, -0.04439579], q_vc=[-0.7035177, 0.7106742, 0.0014521, -0.0017207])
    p = ekf_np.Params.from_orc(po)
    n = p.num_states
    rng = np.random.default_rng(11 + 2 * direct + est_bias)
    B = 40
    x, P = rand_states(rng, B, n, cov_scale=0.3)
    z = meas_near(rng, po, x, ang=np.deg2rad(170.0))
    for i in range(B):
        dy, G, S, nis = innovation_ref(p, x[i], P[i], z[i])
        K = P[i] @ G.T @ np.linalg.inv(S)
        Po = (np.eye(n) - K @ G) @ P[i]
        dx = K @ dy
        xo = np.zeros(16)
        xo[0:3] = x[i, 0:3] + dx[0:3]
        xo[3:6] = x[i, 3:6] + dx[3:6]
        xo[6:10] = quaternion_norm(qmul(x[i, 6:10], quaternion_exp(dx[6:9])))
        if est_bias:
            xo[10:13] = x[i, 10:13] + dx[9:12]; xo[13:16] = x[i, 13:16] + dx[12:15]
        xr, Pr, _, _ = ekf_np.correction_step(p, x[i], P[i], z[i, :3], z[i, 3:])
        np.testing.assert_allclose(xo, xr, rtol=0, atol=1e-12)
        np.testing.assert_allclose(Po, Pr, rtol=0, atol=1e-12 * np.abs(Pr).max())
        assert nis > 0 and np.isfinite(nis)
        np.testing.assert_allclose(S, S.T, rtol=0, atol=1e-15 * np.abs(S).max())


def _ctype(decl):
    decl = " ".join(decl.split())
    table = {"qle_batch *": C.c_void_p, "const double *": C.POINTER(C.c_double), "double *": C.POINTER(C.c_double),
             "const uint8_t *": C.POINTER(C.c_uint8), "uint8_t *": C.POINTER(C.c_uint8), "double": C.c_double}
    return table[decl]


def test_lib_binds_innovation_entry_points_with_header_types():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qle_ekf.h")).read(), flags=re.S)
    for name in ("qle_innovation", "qle_update_gated", "qle_step_gated"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{name} not declared"
        args = [re.sub(r"\s*\w+$", "", a.strip()).replace("*", " *").strip() for a in m.group(1).split(",")]
        want = [_ctype(a) for a in args]
        res, got = _lib.SYMBOLS[name]
        assert res is C.c_int
        assert got == want, (name, got, want)
