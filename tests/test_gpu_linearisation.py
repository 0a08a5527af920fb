"""The engine's correction against the model-derived truth of tests/golden/linearisation_truth.npz (tests/truth_mp.py, mpmath): the
conventional linearisation (relative_pose_EKF.cpp:440-444,455-458) and the delta_q flip (:449) held directly, not through the oracle.

Reads only the fixture.  Every input of it is a float32 value, so both dtypes hold exactly what the truth was computed on (asserted:
get_state returns the inputs bit for bit).  Parametrised as test_gpu_innovation.py: dtype, orientation method, full record / 9-state
record on the full and on the compact layout, and the three kernel families; per-filter tag noise through set_filter_params in the
half of the grid where the indices of dtype, method and record sum to an odd number, the shared noise of the fixture otherwise.

Tolerances: innovation outputs as test_gpu_innovation.py (1e-12 / 3e-5 of the largest element, NIS 1e-12 / 1e-4); the corrected state as
test_update_teacher_forced holds the same kernels to against the oracle (F64U; fp32 state 5e-6, quaternion 2e-6, covariance 7e-5).
tests/tolerances_linearisation.md lists what an MI355X measured.
"""
import numpy as np
import pytest

import quadrotor_landing_amd as qla
import test_gpu_parity as tp
from linearisation_util import params_kw, probe_covs, probes, rel, table
from test_gpu_innovation import TOL, _same
from util import assert_state_close, note

pytestmark = pytest.mark.gpu

UPD = {"f64": tp.F64U, "f32": dict(rtol=5e-6, atol=5e-6, qtol=2e-6, ptol=7e-5)}
RECORDS = [("bias1", 1, None), ("bias0-full", 0, "0"), ("bias0-compact", 0, "1")]     # (id, est_bias, QLE_COMPACT)
GRID = [(d, o, r) for d in ("f64", "f32") for o in (1, 0) for r in range(len(RECORDS))]
GRID_IDS = [f"{d}-direct{o}-{RECORDS[r][0]}" for d, o, r in GRID]
grid = pytest.mark.parametrize("dtype,direct,record", GRID, ids=GRID_IDS)
TABLE_IDX = np.concatenate([np.arange(40), np.arange(40), np.arange(24)])                # 104: one full wave and a partial one


@pytest.fixture(autouse=True, params=["default", "lanes-only", "coop-forced"])
def kernel_family(request, monkeypatch):
    """As in test_gpu_innovation.py (same ids, so the keys of util.note stay family-free); QLE_QUAD is read at handle creation."""
    if request.param == "lanes-only":
        monkeypatch.setenv("QLE_QUAD", "0")
    elif request.param == "coop-forced":
        monkeypatch.setenv("QLE_QUAD", "3")
    else:
        monkeypatch.delenv("QLE_QUAD", raising=False)
    return request.param


def _handle(batch, dtype, direct, record, monkeypatch):
    _, est_bias, compact = RECORDS[record]
    if compact is None:
        monkeypatch.delenv("QLE_COMPACT", raising=False)
    else:
        monkeypatch.setenv("QLE_COMPACT", compact)
    kw = params_kw(direct, est_bias)
    return qla.BatchedRelativePoseEKF(batch, dtype, params=qla.make_params(**kw)), est_bias


@grid
def test_probe_covariances_give_the_truths_G_and_Rk(dtype, direct, record, monkeypatch):
    """S of qle_innovation on P = 0, e_i e_i^T, (e_i + e_j)(e_i + e_j)^T against the truth's G P G^T + R_k: every column of G."""
    est_bias = RECORDS[record][1]
    n = 15 if est_bias else 9
    Ps = probe_covs(n)
    B = len(Ps)
    assert B == 1 + n * (n + 1) // 2
    ekf, _ = _handle(B, dtype, direct, record, monkeypatch)
    xs, Gt, Rkt = probes(direct, est_bias)
    z = np.tile(np.array([0.1, -0.2, 2.0, 0.0, 0.0, 0.0, 1.0]), (B, 1))
    for k, (x, Gk, Rk) in enumerate(zip(xs, Gt, Rkt)):
        ekf.set_state(np.tile(x, (B, 1)), Ps)
        xd, Pd = ekf.get_state()
        assert _same(xd, np.tile(x, (B, 1))) and _same(Pd, Ps)
        _, S, _ = ekf.innovation(z)
        e = rel(S, Gk @ Ps @ Gk.T + Rk)
        print(f"probe {k} {dtype} direct{direct}: S {e:.2e}")
        note(f"probe{k}_S", e, TOL[dtype]["S"])
        assert e < TOL[dtype]["S"]
    ekf.close()


@grid
def test_case_table_against_truth(dtype, direct, record, monkeypatch):
    """The 40 corrections of the branch (attitude innovations from 0 to 2 pi - 1e-6, both sides of the cover at theta* = 4.84 rad, eight
    states with a negative stored w) in a batch of 104: innovation, then update, against the truth; repeated rows bit for bit."""
    use_pfp = (int(dtype == "f32") + direct + record) % 2 == 1
    ekf, est_bias = _handle(len(TABLE_IDX), dtype, direct, record, monkeypatch)
    t = table(direct, est_bias)
    n = t["n"]
    x, P, z = t["x"][TABLE_IDX], t["P"][TABLE_IDX], t["z"][TABLE_IDX]
    truth = t["pfp" if use_pfp else "shared"]
    if use_pfp:
        pq = qla.make_params(**params_kw(direct, est_bias))
        pfp = np.zeros((len(TABLE_IDX), 24))
        pfp[:, 0:12] = np.concatenate([list(pq.Q_a), list(pq.Q_w), list(pq.Q_ab), list(pq.Q_wb)])   # the shared process noise
        pfp[:, 12:15] = tp.HW["ab_static"]; pfp[:, 15:18] = tp.HW["wb_static"]
        pfp[:, 18:24] = t["R"][TABLE_IDX]
        if n == 9:
            pfp[:, 6:12] = 0.0
        ekf.set_filter_params(pfp)
        assert _same(ekf.get_filter_params()[:, 18:24], t["R"][TABLE_IDX])
    ekf.set_state(x, P)
    xd, Pd = ekf.get_state()
    assert _same(xd, x) and _same(Pd, P)
    tol = TOL[dtype]
    nu, S, nis = ekf.innovation(z)
    nur, Sr, nisr = t["nu"][TABLE_IDX], truth["S"][TABLE_IDX], truth["nis"][TABLE_IDX]
    e_nu, e_S, e_nis = rel(nu, nur), rel(S, Sr), float(np.abs(nis / nisr - 1).max())
    print(f"{dtype} direct{direct} {RECORDS[record][0]} pfp={use_pfp}: nu {e_nu:.2e} S {e_S:.2e} nis {e_nis:.2e}")
    note("nu", e_nu, tol["nu"]); note("S", e_S, tol["S"]); note("nis", e_nis, tol["nis"])
    assert e_nu < tol["nu"] and e_S < tol["S"] and e_nis < tol["nis"], (e_nu, e_S, e_nis)
    ekf.update(z)
    xg, Pg = ekf.get_state()
    xr, Pr = truth["x_hat"][TABLE_IDX], truth["P_hat"][TABLE_IDX]
    for i in range(40):                                          # per row, printed before anything is asserted
        dq = np.minimum(np.abs(xg[i, 6:10] - xr[i, 6:10]).max(), np.abs(xg[i, 6:10] + xr[i, 6:10]).max())
        keep = [j for j in range(16) if not 6 <= j < 10]
        ds = (np.abs(xg[i, keep] - xr[i, keep]) / (1 + np.abs(xr[i, keep]))).max()
        sc = np.sqrt(np.outer(np.diag(Pr[i]), np.diag(Pr[i])))
        print(f"  row {i:2d} angle {t['angle'][i]:.6f}: state {ds:.2e} quat {dq:.2e} cov {(np.abs(Pg[i] - Pr[i]) / sc).max():.2e}")
    assert_state_close(xg, Pg, xr, Pr, **UPD[dtype])
    first = np.arange(40)
    for a in (nu, S, nis, xg, Pg):
        assert _same(a[40:80], a[first]) and _same(a[80:104], a[:24])
    ekf.close()
