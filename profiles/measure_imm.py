#!/usr/bin/env python3
"""Time of one IMM mixing step by HIP events, next to one bank fuse on the same batch and to the route a caller had before
(profiles/imm.md).

    python profiles/measure_imm.py [--filters B] [--repeats N] [--head HEAD] [--out PATH]

For fp32 and fp64 handles of B filters (default 65536, full 15-state records) and M = 2, 4 and 8 members per bank the run seeds the
filters from device tensors, runs a few ticks, then times each row N times (default 40) after 5 warm-up rounds with a pair of HIP events
on the caller's stream around the whole row -- every row is ordered behind that stream and that stream behind it, as every DeviceIO call
is -- and writes the medians with their p10 - p90 spread as a markdown table to PATH (default profiles/imm.md), stamped with HEAD
(default: `git rev-parse` of the tree the script runs in).

    mix           Imm.mix(): ONE launch of k_imm_mix, with the host work of the call (logc and mixed are allocated, the view is queried)
                  between the events
    mix_kernel    qim_mix alone into buffers allocated beforehand: the launch and the two stream orderings
    fuse_kernel   qbk_fuse alone on the same batch into buffers allocated beforehand, for comparison
    update_kernel qim_update alone
    torch_route   what a caller had before: DeviceIO.state() (16 + 225 dense float64 words per filter), the mixing as torch kernels, and
                  the host-fed set_state (which synchronises)

No ratio is a pass criterion: the numbers are a record.  The cost model to hold them against: one record read and one written per filter
(2 x 136 words), twice the read of k_bank_fuse, and the cross-lane words -- per member of the loop, per lane: the 16 state words in pass 1
and again in each of the six covariance groups (where only the words the group's covariance entries need survive), and the 120 covariance
words once."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def head_of_tree():
    try:
        h = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
        dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True, check=True).stdout.strip()
        return f"the tree of this change on top of `{h}`" if dirty else f"`{h}`"
    except (OSError, subprocess.CalledProcessError):
        return "an unknown head (no git metadata where the script ran)"


def torch_mix(torch, x, P, logmu, Pi, M):
    """The mixing step of every bank in torch (all members valid): the arithmetic of include/qle_imm.h."""
    B, n = x.shape[0], P.shape[1]
    G = B // M
    x, P = x.view(G, M, 16), P.view(G, M, n, n)
    mu = torch.softmax(logmu.view(G, M), dim=1)
    c = mu @ Pi                                                               # [G, j]
    w = Pi[None] * mu[:, :, None] / c[:, None, :]                             # [G, i, j]
    xi, xj = x[:, :, None, :], x[:, None, :, :]

    def qmul(a, b):
        av, aw, bv, bw = a[..., :3], a[..., 3:4], b[..., :3], b[..., 3:4]
        return torch.cat([aw * bv + bw * av + torch.cross(av.expand_as(bv), bv, dim=-1), aw * bw - (av * bv).sum(-1, keepdim=True)], dim=-1)

    def qnorm(a):
        a = a / a.norm(dim=-1, keepdim=True)
        return torch.where(a[..., 3:4] < -0.75, -a, a)

    qc = (xj[..., 6:10] * x.new_tensor([-1.0, -1.0, -1.0, 1.0])).expand(G, M, M, 4)
    dq = qnorm(qmul(qc, xi[..., 6:10].expand(G, M, M, 4)))
    m = dq[..., :3].norm(dim=-1, keepdim=True)
    dth = torch.where(m < 1e-10, 2.0 * dq[..., :3], 2.0 * torch.atan2(m, dq[..., 3:4]) / m.clamp_min(1e-300) * dq[..., :3])
    d = torch.cat([(xi - xj)[..., 0:6], dth, (xi - xj)[..., 10:16]], dim=-1)  # [G, i, j, 15]
    mean = (w[..., None] * d).sum(dim=1)                                      # [G, j, 15]
    a = mean[..., 6:9].norm(dim=-1, keepdim=True)
    qe = torch.cat([mean[..., 6:9] * torch.where(a > 1e-12, torch.sin(a / 2) / a.clamp_min(1e-300), torch.full_like(a, 0.5)), torch.cos(a / 2)], dim=-1)
    x0 = torch.cat([x[..., 0:6] + mean[..., 0:6], qnorm(qmul(x[..., 6:10], qe)), x[..., 10:16] + mean[..., 9:15]], dim=-1)
    cc = (d - mean[:, None])[..., :n]
    P0 = torch.einsum("gij,ginm->gjnm", w, P) + torch.einsum("gij,gijn,gijm->gjnm", w, cc, cc)
    return x0.reshape(B, 16), P0.reshape(B, n, n), torch.log(c).reshape(B)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filters", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--head", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "imm.md"))
    a = ap.parse_args()
    import numpy as np
    import torch

    import quadrotor_landing_amd as qla
    from quadrotor_landing_amd import bank as bk
    from quadrotor_landing_amd import imm as im
    from quadrotor_landing_amd._lib import QleDeviceView

    B, warm = a.filters, 5
    kw = dict(update_freq=400.0, measurement_freq=30.0, direct_orien_method=1, Q_a=[0.0005] * 3, Q_w=[0.00005] * 3,
              R_r=[0.015, 0.015, 0.020], R_ang=[0.0015, 0.0015, 0.04])
    members = (2, 4, 8)
    names = ("mix", "mix_kernel", "fuse_kernel", "update_kernel", "torch_route")
    tables = {}
    for dtype in ("f32", "f64"):
        ekf = qla.BatchedRelativePoseEKF(B, dtype, **kw)
        io = qla.DeviceIO(ekf)
        g = torch.Generator(device="cuda:0"); g.manual_seed(9)
        z = torch.zeros((B, 7), dtype=torch.float32, device="cuda:0")
        z[:, :3] = torch.rand((B, 3), generator=g, device="cuda:0") * 2.0 - 1.0; z[:, 2] += 2.5
        q = torch.randn((B, 4), generator=g, device="cuda:0") * 0.1; q[:, 3] = 1.0
        z[:, 3:] = q / q.norm(dim=1, keepdim=True)
        u = torch.randn((B, 6), generator=g, device="cuda:0") * 0.05; u[:, 2] += 9.8
        io.seed(z)
        for k in range(8):
            io.tick(u, z if k % 4 == 3 else None)
        logmu = torch.randn((B,), generator=g, device="cuda:0", dtype=torch.float64)
        loglik = torch.randn((B,), generator=g, device="cuda:0", dtype=torch.float64) * 3.0
        x_keep, P_keep = (t.cpu().numpy() for t in io.state(dtype="float64"))
        K, Q = bk.bank_lib(), im.imm_lib()
        view = io._view()

        def timed(fn):
            us = []
            for k in range(warm + a.repeats):
                torch.cuda.synchronize(); ekf.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                keep = fn()   # noqa: F841  (the result lives until the events are read)
                e1.record()
                e1.synchronize()
                if k >= warm:
                    us.append(e0.elapsed_time(e1) * 1e3)
            us.sort()
            return statistics.median(us), us[len(us) // 10], us[(9 * len(us)) // 10]

        for M in members:
            Pi_h = np.full((M, M), 0.1 / (M - 1)) + np.eye(M) * (0.9 - 0.1 / (M - 1))
            m = io.imm(M, Pi_h, logmu0=logmu)
            Pi = m.Pi
            nbytes = bk.bcheck(K.qbk_workspace_bytes(C.byref(view), M))
            ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda:0")
            w = torch.empty((B,), dtype=torch.float64, device="cuda:0")
            best = torch.empty((B // M,), dtype=torch.int32, device="cuda:0")
            logc = torch.empty((B,), dtype=torch.float64, device="cuda:0")
            out = torch.empty((B,), dtype=torch.float64, device="cuda:0")
            mixed = torch.empty((B,), dtype=torch.uint8, device="cuda:0")
            fused = QleDeviceView()

            def mix_kernel():
                with io._ordered(view, logmu, Pi):
                    im.icheck(Q.qim_mix(C.byref(view), C.byref(ekf.params), M, logmu.data_ptr(), Pi.data_ptr(), None, logc.data_ptr(), mixed.data_ptr()))

            def fuse_kernel():
                with io._ordered(view, logmu):
                    bk.bcheck(K.qbk_fuse(C.byref(view), M, logmu.data_ptr(), None, ws.data_ptr(), nbytes, C.byref(fused), w.data_ptr(), best.data_ptr()))

            def update_kernel():
                with io._ordered(view, logc, loglik):
                    im.icheck(Q.qim_update(C.byref(view), M, logc.data_ptr(), loglik.data_ptr(), None, m.logmu_min, out.data_ptr()))

            def torch_route():
                x0, P0, lc = torch_mix(torch, *io.state(dtype="float64"), logmu, Pi, M)
                ekf.set_state(x0.cpu().numpy(), P0.cpu().numpy())
                return lc

            # the two routes compute the same thing, from the same state
            ekf.set_state(x_keep, P_keep)
            xt, Pt, lt = torch_mix(torch, *io.state(dtype="float64"), logmu, Pi, M)
            lc, mx = m.mix()
            xm, Pm = io.state(dtype="float64")
            assert bool(mx.all()) and float((lc - lt).abs().max()) < 1e-11
            assert float((xm - xt).abs().max()) < (1e-4 if dtype == "f32" else 1e-9) and float((Pm - Pt).abs().max()) < (1e-4 if dtype == "f32" else 1e-9)
            rows = dict(mix=lambda: m.mix(), mix_kernel=mix_kernel, fuse_kernel=fuse_kernel, update_kernel=update_kernel, torch_route=torch_route)
            tables[dtype, M] = {n: timed(rows[n]) for n in names}
            assert bool(torch.isfinite(io.state()[0]).all())
        io.close(); ekf.close()

    cell = lambda t: f"{t[0]:.1f} ({t[1]:.1f} - {t[2]:.1f})"   # noqa: E731
    lines = ["# IMM: one `mix` against one `fuse` and against the torch route", "",
             f"Measured on an MI355X with `profiles/measure_imm.py` ({B} filters, full 15-state records, {a.repeats} timed rounds after {warm}",
             "warm-up rounds, a pair of HIP events on the caller's stream around each row), on " + (a.head or head_of_tree()) + ".  One run, one",
             "machine; the p10 - p90 spread is given, no box-to-box spread was taken.  Microseconds, median (p10 - p90).", "",
             "Rows: `mix` = `Imm.mix()`, ONE launch of `k_imm_mix` with the host work of the call between the events; `mix_kernel` = `qim_mix`",
             "alone into buffers allocated beforehand; `fuse_kernel` = `qbk_fuse` alone on the same batch; `update_kernel` = `qim_update` alone;",
             "`torch_route` = `DeviceIO.state()`, the mixing as torch kernels and the host-fed `set_state`, what a caller had before.  No ratio is",
             "a pass criterion.", ""]
    for dtype in ("f32", "f64"):
        lines += [f"## {dtype}", "", "| M | " + " | ".join(names) + " | mix_kernel / fuse_kernel | torch_route / mix |", "|---|" + "---|" * (len(names) + 2)]
        for M in members:
            t = tables[dtype, M]
            lines.append(f"| {M} | " + " | ".join(cell(t[n]) for n in names) + f" | {t['mix_kernel'][0] / t['fuse_kernel'][0]:.2f} | {t['torch_route'][0] / t['mix'][0]:.1f} |")
        lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
