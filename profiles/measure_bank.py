#!/usr/bin/env python3
"""Time of one bank fuse by HIP events, next to the two things it can be compared with on the same box (profiles/bank.md).

    python profiles/measure_bank.py [--filters B] [--repeats N] [--head HEAD] [--out PATH]

For fp32 and fp64 handles of B filters (default 65536, full 15-state records) and M = 4 and 64 members per bank the run seeds the filters
from device tensors, runs a few ticks, then times each row N times (default 40) after 5 warm-up rounds with a pair of HIP events on the
caller's stream around the whole row -- every row is ordered behind that stream and that stream behind it, as every DeviceIO call is --
and writes the medians with their p10 - p90 spread as a markdown table to PATH (default profiles/bank.md), stamped with HEAD (default:
`git rev-parse` of the tree the script runs in).

    fuse          Bank.fuse(logw): ONE launch of k_bank_fuse, with the host work of the call (workspace, w and best are allocated, the
                  view is queried) between the events
    fuse_kernel   qbk_fuse alone into buffers allocated beforehand: the launch and the two stream orderings
    nees          DeviceIO.nees(x_true): k_nees and its reduce, a read-only launch with the same record reads, with the host work of the call
    nees_kernel   qcs_nees alone (no summary: one launch) into buffers allocated beforehand
    torch_route   what a caller had before: DeviceIO.state() (16 + 225 dense float64 words per filter), then softmax, quaternion algebra
                  and weighted sums as torch kernels

No ratio is a pass criterion: the numbers are a record.  Algorithmic words per filter: the fuse reads 136 and writes 136 / M; k_nees
reads 136 + 16; the cross-lane work of the fuse is 135 fp64 values x log2 M stages per bank sum."""
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


def torch_route(torch, io, logw, M):
    """The moment-matched mixture of every bank from DeviceIO.state() in torch: the arithmetic of include/qle_bank.h."""
    x, P = io.state(dtype="float64")
    B, n = x.shape[0], P.shape[1]
    G = B // M
    x, P, lw = x.view(G, M, 16), P.view(G, M, n, n), logw.view(G, M)
    w = torch.softmax(lw, dim=1)
    ref = lw.argmax(dim=1)
    xr = x[torch.arange(G, device=x.device), ref][:, None, :]
    qr, q = xr[..., 6:10] * x.new_tensor([-1.0, -1.0, -1.0, 1.0]), x[..., 6:10]

    def qmul(a, b):
        av, aw, bv, bw = a[..., :3], a[..., 3:4], b[..., :3], b[..., 3:4]
        return torch.cat([aw * bv + bw * av + torch.cross(av.expand_as(bv), bv, dim=-1),
                          aw * bw - (av * bv).sum(-1, keepdim=True)], dim=-1)

    def qnorm(a):
        a = a / a.norm(dim=-1, keepdim=True)
        return torch.where(a[..., 3:4] < -0.75, -a, a)

    dq = qnorm(qmul(qr.expand_as(q), q))
    m = dq[..., :3].norm(dim=-1, keepdim=True)
    dth = 2.0 * torch.atan2(m, dq[..., 3:4]) / m.clamp_min(1e-300) * dq[..., :3]
    d = torch.cat([x[..., 0:6] - xr[..., 0:6], dth, x[..., 10:16] - xr[..., 10:16]], dim=-1)
    mean = (w[..., None] * d).sum(dim=1, keepdim=True)
    a = mean[..., 6:9].norm(dim=-1, keepdim=True)
    qe = torch.cat([mean[..., 6:9] * (torch.sin(a / 2) / a.clamp_min(1e-300)), torch.cos(a / 2)], dim=-1)
    xbar = torch.cat([xr[..., 0:6] + mean[..., 0:6], qnorm(qmul(xr[..., 6:10], qe)), xr[..., 10:16] + mean[..., 9:15]], dim=-1)[:, 0]
    c = (d - mean)[..., :n]
    Pbar = (w[..., None, None] * (P + c[..., :, None] * c[..., None, :])).sum(dim=1)
    return xbar, Pbar, w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filters", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--head", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bank.md"))
    a = ap.parse_args()
    import torch

    import quadrotor_landing_amd as qla
    from quadrotor_landing_amd import bank as bk
    from quadrotor_landing_amd import consistency as cs
    from quadrotor_landing_amd import devio as dv
    from quadrotor_landing_amd._lib import QleDeviceView

    B, warm = a.filters, 5
    kw = dict(update_freq=400.0, measurement_freq=30.0, direct_orien_method=1, Q_a=[0.0005] * 3, Q_w=[0.00005] * 3,
              R_r=[0.015, 0.015, 0.020], R_ang=[0.0015, 0.0015, 0.04])
    members = (4, 64)
    names = ("fuse", "fuse_kernel", "nees", "nees_kernel", "torch_route")
    tables = {}
    for dtype in ("f32", "f64"):
        ekf = qla.BatchedRelativePoseEKF(B, dtype, **kw)
        io = qla.DeviceIO(ekf)
        g = torch.Generator(device="cuda:0"); g.manual_seed(8)
        z = torch.zeros((B, 7), dtype=torch.float32, device="cuda:0")
        z[:, :3] = torch.rand((B, 3), generator=g, device="cuda:0") * 2.0 - 1.0; z[:, 2] += 2.5
        q = torch.randn((B, 4), generator=g, device="cuda:0") * 0.1; q[:, 3] = 1.0
        z[:, 3:] = q / q.norm(dim=1, keepdim=True)
        u = torch.randn((B, 6), generator=g, device="cuda:0") * 0.05; u[:, 2] += 9.8
        io.seed(z)
        for k in range(8):
            io.tick(u, z if k % 4 == 3 else None)
        logw = torch.randn((B,), generator=g, device="cuda:0", dtype=torch.float64) * 2.0
        x_true = io.state(dtype="float64")[0].clone()
        K, N = bk.bank_lib(), cs.consistency_lib()
        view = io._view()
        nees_out = torch.empty((B,), dtype=torch.float64, device="cuda:0")

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

        def nees_kernel():
            with io._ordered(view, x_true):
                cs.ccheck(N.qcs_nees(C.byref(view), C.byref(ekf.params), x_true.data_ptr(), dv.QDV_F64, None, 31, float("inf"), nees_out.data_ptr(),
                                     None, None, dv.QDV_F64))

        for M in members:
            b = io.bank(M)
            nbytes = bk.bcheck(K.qbk_workspace_bytes(C.byref(view), M))
            ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda:0")
            w = torch.empty((B,), dtype=torch.float64, device="cuda:0")
            best = torch.empty((B // M,), dtype=torch.int32, device="cuda:0")
            fused = QleDeviceView()

            def fuse_kernel():
                with io._ordered(view, logw):
                    bk.bcheck(K.qbk_fuse(C.byref(view), M, logw.data_ptr(), None, ws.data_ptr(), nbytes, C.byref(fused), w.data_ptr(), best.data_ptr()))

            rows = dict(fuse=lambda: b.fuse(logw), fuse_kernel=fuse_kernel, nees=lambda: io.nees(x_true), nees_kernel=nees_kernel,
                        torch_route=lambda: torch_route(torch, io, logw, M))
            tables[dtype, M] = {n: timed(rows[n]) for n in names}
            # the two routes compute the same thing
            f = b.fuse(logw)
            xt, Pt, wt = torch_route(torch, io, logw, M)
            xf, Pf = f.state(dtype="float64")
            assert float((f.w - wt.reshape(-1)).abs().max()) < 1e-12 and float((Pf - Pt).abs().max()) < (1e-4 if dtype == "f32" else 1e-10)
            assert bool(torch.isfinite(xf).all())
        io.close(); ekf.close()

    cell = lambda t: f"{t[0]:.1f} ({t[1]:.1f} - {t[2]:.1f})"   # noqa: E731
    lines = ["# Filter banks: one `fuse` against the torch route and against `nees`", "",
             f"Measured on an MI355X with `profiles/measure_bank.py` ({B} filters, full 15-state records, {a.repeats} timed rounds after {warm}",
             "warm-up rounds, a pair of HIP events on the caller's stream around each row), on " + (a.head or head_of_tree()) + ".  One run, one",
             "machine; the p10 - p90 spread is given, no box-to-box spread was taken.  Microseconds, median (p10 - p90).", "",
             "Rows: `fuse` = `Bank.fuse(logw)`, ONE launch of `k_bank_fuse` with the host work of the call between the events; `fuse_kernel` =",
             "`qbk_fuse` alone into buffers allocated beforehand; `nees` = `DeviceIO.nees(x_true)` (`k_nees` and its reduce), a read-only launch with",
             "the same record reads; `nees_kernel` = `qcs_nees` alone, no summary (one launch); `torch_route` = `DeviceIO.state()` followed by",
             "softmax, quaternion algebra and weighted sums as torch kernels, what a caller had before.  No ratio is a pass criterion.", ""]
    for dtype in ("f32", "f64"):
        lines += [f"## {dtype}", "", "| M | " + " | ".join(names) + " | fuse_kernel / nees_kernel | torch_route / fuse |", "|---|" + "---|" * (len(names) + 2)]
        for M in members:
            t = tables[dtype, M]
            lines.append(f"| {M} | " + " | ".join(cell(t[n]) for n in names) + f" | {t['fuse_kernel'][0] / t['nees_kernel'][0]:.2f} | {t['torch_route'][0] / t['fuse'][0]:.1f} |")
        lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
