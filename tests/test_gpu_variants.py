"""Every tick-kernel instantiation of the library, launched and checked (tests/variant_table.py lists them; the CPU test holds the list
to the built library).

Per semantic key, every row runs the same inputs on a ragged batch (a grid of >= 8 workgroups, remapped over the XCDs) under its own
QLE_* overrides, inside a launch census that must name exactly the row's kernels (helper kernels that stage the inputs aside).  The
canonical row is compared with the fp64 oracle on a strided sample of filters (every wave slot of a 256-thread workgroup included)
with the tolerances of test_gpu_parity.py / test_gpu_innovation.py; every other row must equal it bit for bit.  The fp64 rows at
QLE_BLOCK=256 (four LDS windows per workgroup) are also compared with the oracle.  Inputs: random states, a mix of mask bits with a
whole wave correcting and one not, large-angle lanes (gyro rates of ~11 rad/s, 170-degree attitude innovations); gating rows see both
outcomes of the corner gate, multirate rows replay delayed corrections across a checkpoint."""
import zlib

import numpy as np
import pytest

import oracle
import quadrotor_landing_amd as qla
import variant_table as vt
from oracle import ekf_np
from test_gpu_innovation import TOL as INNOV_TOL
from test_gpu_parity import F32, F32U, F64, F64U, HW, HW_TAGS, free_run_close
from innovation_util import CHI2_6_099, innovation_ref_batch
from util import assert_state_close, meas_near, rand_imu, rand_states

pytestmark = pytest.mark.gpu

ENV_KEYS = ("QLE_COMPACT", "QLE_NT", "QLE_REFRESH", "QLE_SPLIT", "QLE_LOADS_FIRST", "QLE_QUAD", "QLE_BLOCK")
SAMPLE = np.r_[0:16, 16:vt.B_MAX:7]                 # stride 7: every residue modulo 256, so every wave slot of every workgroup size
UPD = {"f64": F64U, "f32": dict(F32U, ptol=7e-5)}   # stand-alone update: as test_update_teacher_forced
ONE = {"f64": F64, "f32": F32}
MR_T, MR_MEAS = 40, (6, 12, 18, 24, 30, 36)         # delay 5 ticks: the tick-36 correction replays 31..36 across the tick-32 checkpoint


def _r32(a, dtype):
    return a.astype(np.float32).astype(np.float64) if dtype == "f32" else a


def _kwargs(row):
    kw = dict(update_freq=100.0, **HW, **row["params"])
    if row["gating"] or row["entry"] == "step_mr":
        kw.update(HW_TAGS, corner_margin_enbl=1, limit_measurement_freq=0)
    if row["entry"] == "step_mr":
        kw.update(dynamic_meas_delay=0, measurement_delay=0.05)
    return kw


class Inputs:
    """One set of inputs per semantic key at the largest batch; a row uses its first B filters."""

    def __init__(self, row):
        kw = _kwargs(row)
        self.po = oracle.make_params(**kw)
        self.pq = qla.make_params(**kw)
        n, dt = self.po.num_states, row["dtype"]
        rng = np.random.default_rng(zlib.crc32(repr(row["key"]).encode()))
        B = vt.B_MAX
        x, P = rand_states(rng, B, n, cov_scale=0.3)
        if n == 9:
            x[:, 10:16] = 0.0
        if row["gating"] or row["entry"] == "step_mr":      # half of the filters level and near the tags: both corner-gate outcomes
            lv = rng.uniform(size=B) < 0.5
            x[lv, 0:3] = rng.uniform([-0.3, -0.3, 0.8], [0.3, 0.3, 2.0], size=(int(lv.sum()), 3))
            x[lv, 6:10] = [0, 0, 0, 1.0]
        self.x, self.P = _r32(x, dt), _r32(P, dt)
        self.U = np.stack([rand_imu(rng, B) for _ in range(MR_T)])
        if row["entry"] == "step_mr":
            self.U *= np.array([0.05, 0.05, 1, 0.2, 0.2, 0.2])
        self.U[:, 2::101, 3:6] = [8.0, -6.0, 5.0]             # large-angle lanes
        self.U = _r32(self.U, dt)
        z = meas_near(rng, self.po, x, ang=0.3 if row["gating"] else 0.8, pos=0.05)
        big = slice(5, None, 97)
        z[big] = meas_near(rng, self.po, x[big], ang=3.0)     # ~170-degree attitude innovations
        if row["gating"]:
            z[:, 0:2] += rng.choice([0.0, 0.0, 1.5], size=(B, 1)) * rng.normal(size=(B, 2))
        self.z = _r32(z, dt)
        m = rng.uniform(size=B) < 0.6
        m[0:64] = True; m[64:128] = False                      # one whole wave corrects, one does not
        self.mask = m.astype(np.uint8)
        self.pfp = None
        if row["pfp"]:
            pfp = np.zeros((B, 24))
            pfp[:, 0:12] = np.array(list(self.po.Q)) * 10 ** rng.uniform(-0.5, 0.5, size=(B, 12))
            pfp[:, 12:15] = rng.normal(size=(B, 3)) * 0.1
            pfp[:, 15:18] = rng.normal(size=(B, 3)) * 0.01
            pfp[:, 18:24] = np.array(list(self.po.R)) * rng.uniform(0.5, 2.0, size=(B, 6))
            if n == 9:
                pfp[:, 6:12] = 0.0
                pfp[:, 12:18] = np.array(kw["ab_static"] + kw["wb_static"])
            self.pfp = _r32(pfp, dt)
        self.kw = kw

    def orc_params(self, i):
        if self.pfp is None:
            return self.po
        q = self.pfp[i]
        return oracle.make_params(**dict(self.kw, Q_a=q[0:3], Q_w=q[3:6], Q_ab=q[6:9], Q_wb=q[9:12], ab_static=q[12:15], wb_static=q[15:18],
                                         R_r=q[18:21], R_ang=q[21:24]))


def _handle(row, d, monkeypatch):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in row["env"].items():
        monkeypatch.setenv(k, v)
    e = qla.BatchedRelativePoseEKF(row["B"], row["dtype"], params=d.pq)
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    if d.pfp is not None:
        e.set_filter_params(d.pfp[:row["B"]])
    return e


def _tick_kernels(names):
    ids = {vt.kernel_id(n) for n in names}
    return {k for k in ids if k.split("<")[0] not in vt.HELPER_FAMILIES}


def _oracle_filters(d, idx, x, P):
    out = []
    for i in idx:
        f = oracle.Filter(d.orc_params(i))
        for k in range(3):
            f.f.r_nom[k] = x[i, k]; f.f.v_nom[k] = x[i, 3 + k]; f.f.ab_nom[k] = x[i, 10 + k]; f.f.wb_nom[k] = x[i, 13 + k]
        for k in range(4):
            f.f.q_nom[k] = x[i, 6 + k]
        n = d.po.num_states
        for k in range(n * n):
            f.f.cov_pert[k] = P[i].reshape(-1)[k]
        f.f.state_initialized = 1
        out.append(f)
    return out


def run_row(row, d, monkeypatch):
    """-> (outputs: dict of arrays over the row's B filters, census: tick kernels launched, check: oracle comparison of outputs)"""
    B, dt, ent = row["B"], row["dtype"], row["entry"]
    x, P, U, z, mask = d.x[:B], d.P[:B], d.U[:, :B], d.z[:B], d.mask[:B]
    e = _handle(row, d, monkeypatch)
    census, out = set(), {}
    S = SAMPLE[SAMPLE < B]
    pfpS = None if d.pfp is None else d.pfp[S]

    def census_of(fn):
        with qla.launch_census() as names:
            r = fn()
        census.update(_tick_kernels(names))
        return r

    if ent == "step_mr":
        e.enable_gating(True)
        z0 = np.zeros((B, 7))
        z0[:, 0:2] = d.x[:B, 0:2] * 0.1; z0[:, 2] = 1.0 + np.abs(d.x[:B, 2]) * 0.3
        z0[:, 3:7] = [0.7071067811865476, -0.7071067811865476, 0.0, 0.0]
        z0 = _r32(z0, dt)
        e.initialize_state(z0, reinit_bias=True)
        xs0, _ = e.get_state()
        filt = []
        for i in S:
            f = oracle.Filter(d.orc_params(i))
            f.set_apriltag(z0[i, :3], z0[i, 3:], -1.0)
            f.f.measurement_ready = 0
            if dt == "f32":
                for k in range(3):
                    f.f.r_nom[k] = xs0[i, k]
                for k in range(4):
                    f.f.q_nom[k] = xs0[i, 6 + k]
                for k in range(16):
                    f.f.x_hist[k] = xs0[i, k]
            filt.append(f)
        rng = np.random.default_rng(99)
        pending = np.zeros(B, np.uint8); zlast = z0.copy(); n_perf = 0
        for t in range(MR_T):
            tc = 0.01 * t
            new = np.zeros(B, bool)
            if t in MR_MEAS:
                new = rng.uniform(size=B) < 0.6
                zn = _r32(meas_near(rng, d.po, e.get_state()[0], ang=0.2, pos=0.05), dt)
                zlast[new] = zn[new]
                pending |= new.astype(np.uint8)
            for j, i in enumerate(S):
                filt[j].set_imu(U[t, i, :3], U[t, i, 3:])
                if new[i]:
                    filt[j].set_apriltag(zlast[i, :3], zlast[i, 3:], tc)
                filt[j].filter_update(tc)
            census_of(lambda: e.filter_update(U[t], zlast if pending.any() else None, pending if pending.any() else None, t_curr=tc,
                                              apriltag_time=np.full(B, tc)))
            perf, cons, upds = e.tick_flags()
            np.testing.assert_array_equal(perf[S], [f.f.performed_correction for f in filt])
            pending &= (1 - cons)
            n_perf += int(perf.sum())
        assert n_perf > B // 2
        out["x"], out["P"] = e.get_state()
        xr = np.stack([f.x() for f in filt]); Pr = np.stack([f.P() for f in filt])

        def check(o):
            if dt == "f64":
                assert_state_close(o["x"][S], o["P"][S], xr, Pr, 1e-10, 1e-12, 1e-10)
            else:
                assert_state_close(o["x"][S], o["P"][S], xr, Pr, 2e-5, 2e-5, 5e-6, ptol=5e-5)
    elif ent == "run_resident":
        thm = np.zeros(6, np.uint8); thm[[1, 4]] = 1
        seq = e.make_inputs(6, thm)
        M = np.zeros((6, B), np.uint8); Z = np.zeros((6, B, 7))
        for t in range(6):
            if thm[t]:
                M[t] = mask if t == 1 else mask[::-1]; Z[t] = z
                seq.upload_tick(t, U[t], z, M[t])
            else:
                seq.upload_tick(t, U[t])
        e.set_state(x, P)
        census_of(lambda: e.run_resident(seq, 0, 6))
        out["x"], out["P"] = e.get_state()
        xr, Pr = oracle.run_batch(d.po, x[S], P[S], U[:6, S], Z[:, S], M[:, S], per_filter_params=pfpS)

        def check(o):
            tol = 1e-9 if dt == "f64" else 6e-5
            free_run_close(o["x"][S], o["P"][S], xr, Pr, tol, qtol=tol / 8)
        seq.close()
    elif ent in ("innovation", "update_gated"):
        e.set_state(x, P)
        xd, Pd = e.get_state()
        p = ekf_np.Params.from_orc(d.po)
        nur, Sr, nisr = innovation_ref_batch(p, xd[S], Pd[S], z[S], R=None if pfpS is None else pfpS[:, 18:24], mask=mask[S])
        if ent == "innovation":
            out["nu"], out["S"], out["nis"] = census_of(lambda: e.innovation(z, mask))
            out["x"], out["P"] = e.get_state()

            def check(o):
                m = mask[S].astype(bool)
                np.testing.assert_array_equal(o["x"], xd); np.testing.assert_array_equal(o["P"], Pd)
                assert np.isnan(o["nis"][S][~m]).all() and np.isfinite(o["nis"][S][m]).all()
                scale = lambda a: np.abs(a).max(axis=tuple(range(1, a.ndim)), keepdims=True)
                e_nu = (np.abs(o["nu"][S][m] - nur[m]) / np.maximum(scale(nur[m]), 1e-300)).max()
                e_S = (np.abs(o["S"][S][m] - Sr[m]) / np.maximum(scale(Sr[m]), 1e-300)).max()
                e_nis = np.abs(o["nis"][S][m] / nisr[m] - 1).max()
                tol = INNOV_TOL[dt]
                assert e_nu < tol["nu"] and e_S < tol["S"] and e_nis < tol["nis"], (e_nu, e_S, e_nis)
        else:
            acc, nis = census_of(lambda: e.update_gated(z, CHI2_6_099, mask))
            out["acc"], out["nis"] = acc, nis
            out["x"], out["P"] = e.get_state()
            assert acc[mask.astype(bool)].any() and not acc[mask.astype(bool)].all(), "the gate must accept some and reject some"
            xr, Pr, _ = oracle_update(d, S, xd, Pd, z, acc)

            def check(o):
                far = np.abs(nisr / CHI2_6_099 - 1) > 1e-3
                np.testing.assert_array_equal(o["acc"][S][far], (mask[S].astype(bool) & (nisr <= CHI2_6_099))[far])
                assert_state_close(o["x"][S], o["P"][S], xr, Pr, **UPD[dt])
    else:
        e.set_state(x, P)
        if ent in ("predict", "kw_predict"):
            census_of(lambda: e.predict(U[0]))
            xr, Pr = oracle.run_batch(d.po, x[S], P[S], U[:1, S], per_filter_params=pfpS)
            tol = ONE[dt]
        elif ent == "update":
            census_of(lambda: e.update(z, mask))
            xr, Pr, _ = oracle_update(d, S, x, P, z, mask)
            tol = UPD[dt]
        elif not row["gating"]:                                 # step, kw_step: one fused tick
            census_of(lambda: e.step(U[0], z, mask))
            xr, Pr = oracle.run_batch(d.po, x[S], P[S], U[:1, S], z[None, S], mask[None, S], per_filter_params=pfpS)
            tol = dict(F64U) if dt == "f64" else dict(F32U)
        else:                                                   # step, kw_step with the decision logic on the device
            e.enable_gating(True)
            e.set_state(x, P)
            filt = _oracle_filters(d, S, x, P)
            for j, i in enumerate(S):
                filt[j].set_imu(U[0, i, :3], U[0, i, 3:])
                if mask[i]:
                    filt[j].set_apriltag(z[i, :3], z[i, 3:], 0.0)
                filt[j].filter_update(0.0)
            census_of(lambda: e.filter_update(U[0], z, mask))
            perf, cons, upds = e.tick_flags()
            out["perf"] = perf
            np.testing.assert_array_equal(perf[S], [f.f.performed_correction for f in filt])
            m = mask.astype(bool)
            assert perf[m].any() and not perf[m].all(), "the corner gate must pass some tag poses and reject some"
            xr = np.stack([f.x() for f in filt]); Pr = np.stack([f.P() for f in filt])
            tol = dict(rtol=1e-10, atol=1e-12, qtol=1e-10) if dt == "f64" else dict(rtol=2e-5, atol=2e-5, qtol=3e-6, ptol=3e-5)
        out["x"], out["P"] = e.get_state()

        def check(o):
            assert_state_close(o["x"][S], o["P"][S], xr, Pr, **tol)
    assert e.count_nonfinite() == 0
    if ent not in ("predict", "kw_predict", "innovation"):
        assert np.abs(out["x"] - x).max() > 1e-3, "a correcting row must change the state"
    e.close()
    return out, census, check


def oracle_update(d, S, x, P, z, mask):
    xo, Po = x[S].copy(), P[S].copy()
    obs = np.zeros((S.size, 7))
    for j, i in enumerate(S):
        if mask[i]:
            xo[j], Po[j], obs[j, :3], obs[j, 3:] = oracle.correction_step(d.orc_params(i), x[i], P[i], z[i, :3], z[i, 3:])
    return xo, Po, obs


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float64:
        return np.array_equal(a.view(np.uint64), b.view(np.uint64))
    return np.array_equal(a, b)


GROUPS = vt.groups()


@pytest.mark.parametrize("key", list(GROUPS), ids=[GROUPS[k][0]["id"].split("[")[0] for k in GROUPS])
def test_every_row_launches_its_kernels_and_matches(key, monkeypatch):
    rows = GROUPS[key]
    d = Inputs(rows[0])
    ref = own = None
    for row in rows:
        out, census, check = run_row(row, d, monkeypatch)
        assert census == set(row["kernels"]), f"{row['id']}: launched {sorted(census)}, expected {sorted(row['kernels'])}"
        if row["canonical"]:
            check(out)
            ref = out
            continue
        if row["own_oracle"]:           # not bit-invariant against the canonical value (variant_table.py): the oracle, and each other
            if own is None:
                check(out)
                own = out
            else:
                for k, v in own.items():
                    assert _same(out[k], v), f"{row['id']}: {k} differs from the first row of its policy value"
            continue
        if row["dtype"] == "f64" and row["env"].get("QLE_BLOCK") == "256":
            check(out)                  # four LDS windows per workgroup, against the oracle as well
        n = min(row["B"], rows[0]["B"])
        for k, v in ref.items():
            assert _same(out[k][:n], v[:n]), f"{row['id']}: {k} differs from the canonical row {rows[0]['id']}"


def test_helper_kernels_census(monkeypatch):
    """Every helper family is launched through launch() and seen by the census."""
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("QLE_TICK_REBASE", "16")
    monkeypatch.setenv("QLE_QUAD", "0")
    seen = set()
    for dt in ("f32", "f64"):
        with qla.launch_census() as names:
            pq = qla.make_params(update_freq=100.0, est_bias=1, **HW)   # single-rate: the tick-origin shift is a multiple of 1
            e = qla.BatchedRelativePoseEKF(300, dt, params=pq)
            e.enable_gating(True)
            seq = e.make_inputs(20, np.r_[np.zeros(9), 1, np.zeros(10)].astype(np.uint8))
            e.synth_generate(seq, seed=3)
            e.synth_rmse(seq)
            u, z, m = seq.download_tick(9)
            e.initialize_state(z)
            x, P = e.get_state()
            e.set_state(x, P)
            for t in range(20):
                e.filter_update(u, z if t == 9 else None, m if t == 9 else None)
            e.report(); e.node_report(); e.count_nonfinite()
            e.initialize_params(est_bias=0)   # re-lays out the live state
            e.close()
        seen |= {vt.kernel_id(n) for n in names}
    fams = {k.split("<")[0] for k in seen}
    assert set(vt.HELPER_FAMILIES) <= fams, sorted(set(vt.HELPER_FAMILIES) - fams)
