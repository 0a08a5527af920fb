#!/usr/bin/env python3
"""Cost of noise adaptation per tag tick against the route without libqle_adapt.so (profiles/adapt.md).

    python profiles/measure_adapt.py --head REV [--filters 65536] [--out profiles/adapt.md]

For fp32 and fp64, B filters seeded by the synthetic generator and a few ticks in: times, by the wall clock around a synchronisation
(ITER iterations after WARM, every iteration the adaptation work of one tag tick from device tensors, window WINDOW; the tick itself is
in neither route),
    adapt    adapter.observe(u, z), and adapter.apply() on every WINDOW-th iteration          k_adapt_observe, k_adapt_apply amortised
    before   io.innovation(z) with nu and S out, io.state() for the noise Jacobian, the same sample by torch batched solves, sums in
             torch; on every WINDOW-th iteration the mean through the host: get_filter_params, the clamp in numpy, set_filter_params
and writes the table, with REV (the revision the numbers were taken on; the tree the script runs in is not a git checkout everywhere),
to --out.  No pass bound: nobody has measured this before."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ITER, WARM, WINDOW = 5000, 100, 20


def rot(q):
    """[B,4] xyzw -> [B,3,3], as oracle/ekf_np.rot"""
    import torch
    x, y, z, w = q.unbind(1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                        2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                        2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)


def skew(r):
    import torch
    o = torch.zeros_like(r[:, 0])
    return torch.stack([o, -r[:, 2], r[:, 1], r[:, 2], o, -r[:, 0], -r[:, 1], r[:, 0], o], dim=1).reshape(-1, 3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--head", required=True)
    ap.add_argument("--filters", type=int, default=65536)
    ap.add_argument("--out", default="profiles/adapt.md")
    a = ap.parse_args()
    import numpy as np
    import torch

    import quadrotor_landing_amd as qla

    B = a.filters
    kw = dict(update_freq=400.0, measurement_freq=30.0, limit_measurement_freq=1, direct_orien_method=1, Q_a=[0.0005] * 3, Q_w=[0.00005] * 3,
              R_r=[0.015, 0.015, 0.020], R_ang=[0.0015, 0.0015, 0.04])
    rows = []
    for dtype in ("f32", "f64"):
        T = 14
        thm = np.zeros(T, np.uint8); thm[T - 1] = 1
        ekf = qla.BatchedRelativePoseEKF(B, dtype, **kw)
        seq = ekf.make_inputs(T, thm)
        ekf.synth_generate(seq, seed=0xE4F00011)
        ekf.run(seq, 0, T - 1)
        u, z, _ = seq.download_tick(T - 1)
        td = torch.float32 if dtype == "f32" else torch.float64
        u, z = torch.from_numpy(u).to(td).to("cuda:0"), torch.from_numpy(z).to(td).to("cuda:0")
        io = qla.DeviceIO(ekf)
        ad = io.adapter(window=WINDOW)
        pfp0 = ekf.get_filter_params()
        R0 = np.array(list(ekf.derived.R))
        lo, hi = R0 / 100, R0 * 100
        C_vc = torch.tensor(list(ekf.derived.C_vc), dtype=torch.float64, device="cuda:0").reshape(3, 3)
        state = {"k": 0, "R": torch.from_numpy(pfp0[:, 18:24]).to("cuda:0"), "sum": torch.zeros((B, 6), dtype=torch.float64, device="cuda:0"),
                 "n": torch.zeros(B, dtype=torch.float64, device="cuda:0")}

        def adapt():
            ad.observe(u, z)
            state["k"] += 1
            if state["k"] % WINDOW == 0:
                ad.apply()

        def before():
            nu, S, nis = io.innovation(z, dtype=torch.float64)
            x, _ = io.state(dtype=torch.float64)
            N = torch.zeros((B, 6, 6), dtype=torch.float64, device="cuda:0")
            N[:, 0:3, 0:3] = -rot(x[:, 6:10]) @ C_vc
            N[:, 3:6, 3:6] = C_vc
            N[:, 0:3, 3:6] = skew(x[:, 0:3])
            sol = torch.linalg.solve(S, torch.cat([nu[:, :, None], N], dim=2))
            ak = (N * sol[:, :, 0:1]).sum(dim=1)
            ck = (N * sol[:, :, 1:]).sum(dim=1)
            R = state["R"]
            rhat = R + R * R * (ak * ak - ck)
            ok = torch.isfinite(nis) & torch.isfinite(rhat).all(dim=1)
            state["sum"] += torch.where(ok[:, None], rhat, 0.0)
            state["n"] += ok.double()
            state["k"] += 1
            if state["k"] % WINDOW == 0:
                n, s = state["n"].cpu().numpy(), state["sum"].cpu().numpy()
                pfp = ekf.get_filter_params()
                on = n >= WINDOW // 2
                with np.errstate(divide="ignore", invalid="ignore"):
                    pfp[on, 18:24] = np.clip(s[on] / n[on, None], lo, hi)
                ekf.set_filter_params(pfp)
                state["R"] = torch.from_numpy(pfp[:, 18:24]).to("cuda:0")
                state["sum"].zero_(); state["n"].zero_()

        times = {}
        for name, fn in (("adapt", adapt), ("before", before), ("adapt again", adapt)):
            ekf.set_filter_params(pfp0)
            ad.reset()
            state["k"] = 0
            for _ in range(WARM):
                fn()
            torch.cuda.synchronize(); ekf.synchronize()
            t0 = time.perf_counter()
            for _ in range(ITER):
                fn()
            torch.cuda.synchronize(); ekf.synchronize()
            times[name] = (time.perf_counter() - t0) / ITER * 1e6
        rows.append((dtype, times))
        print(dtype, {k: round(v, 1) for k, v in times.items()}, flush=True)
        io.close()
        seq.close()
        ekf.close()
    with open(a.out, "w") as f:
        f.write("# Noise adaptation per tag tick: `k_adapt_observe` + amortised `k_adapt_apply` against the route without them\n\n")
        f.write(f"`profiles/measure_adapt.py --head \"{a.head}\" --filters {B}`: microseconds per tag tick fed from device tensors, wall clock around a\n"
                f"synchronisation, mean of {ITER} iterations after {WARM}, window {WINDOW}; MI355X, one process.  The tick itself is in neither figure; host\n"
                "launch overhead is part of every figure.\n\n")
        f.write("| dtype | adapt: `observe` + `apply` / window | before: `innovation` + `state` + torch solves, the mean through the host once per window | adapt, again |\n"
                "|---|---|---|---|\n")
        for dtype, t in rows:
            f.write(f"| {dtype} | {t['adapt']:.1f} | {t['before']:.1f} | {t['adapt again']:.1f} |\n")
        f.write(f"\nTaken on {a.head}.  The two adapt columns bracket the run-to-run spread of the same call.  The route before evaluates the sample against\n"
                "the stored state (the predicted one is not available outside a kernel) and synchronises once per window.\n")


if __name__ == "__main__":
    main()
