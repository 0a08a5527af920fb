#!/usr/bin/env python3
"""Cost of one error budget against the routes without libqle_budget.so (profiles/budget.md).

    python profiles/measure_budget.py --head REV [--filters 65536 2097152] [--out profiles/budget.md]

For fp32 and fp64 and every batch size, B filters seeded by the synthetic generator and a few ticks in, against the generator's truth:
    budget   io.budget(x_true)                                       k_budget + k_budget_reduce, 256 doubles out
    nees     io.nees(x_true, return_err=True)                        k_nees + k_nees_reduce, for scale: the kernel k_budget is built from
    torch    io.nees(x_true, return_err=True) + io.state() + torch   what a caller had: err [B,n] and P [B,n,n] written out, then
                                                                     err.sum(0), einsum("bi,bj->ij") and P.sum(0) in float64
Timing: HIP events on the caller's stream around ITER calls (the calls are ordered behind and in front of that stream), after WARM calls
of the same route; ROUNDS rounds with the three routes alternating, the median round reported and the spread beside it.  Host launch
overhead is part of every figure where the device is the faster of the two.  No pass bound: nobody has measured this kernel before."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARM, ROUNDS = 10, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--head", required=True)
    ap.add_argument("--filters", type=int, nargs="+", default=[65536, 2097152])
    ap.add_argument("--out", default="profiles/budget.md")
    a = ap.parse_args()
    import numpy as np
    import torch

    import quadrotor_landing_amd as qla

    kw = dict(update_freq=400.0, measurement_freq=30.0, limit_measurement_freq=1, direct_orien_method=1, Q_a=[0.0005] * 3, Q_w=[0.00005] * 3,
              R_r=[0.015, 0.015, 0.020], R_ang=[0.0015, 0.0015, 0.04])
    rows = []
    for B in a.filters:
        iters = max(10, min(400, (1 << 24) // B))
        for dtype in ("f32", "f64"):
            T = 14
            thm = np.zeros(T, np.uint8); thm[T - 1] = 1
            ekf = qla.BatchedRelativePoseEKF(B, dtype, **kw)
            seq = ekf.make_inputs(T, thm)
            ekf.synth_generate(seq, seed=0xE4F00021)
            ekf.run(seq, 0, T)
            td = torch.float32 if dtype == "f32" else torch.float64
            xt = torch.from_numpy(ekf._synth_truth_rows(seq)).to(td).to("cuda:0")
            io = qla.DeviceIO(ekf)

            def budget():
                return io.budget(xt).sums

            def nees():
                return io.nees(xt, return_err=True)

            def route():
                _, err, _ = io.nees(xt, return_err=True)
                _, P = io.state()
                e = err.double()
                return e.sum(0), torch.einsum("bi,bj->ij", e, e), P.double().sum(0)

            routes = (("budget", budget), ("nees", nees), ("torch", route))
            times = {name: [] for name, _ in routes}
            for fn in (budget, nees, route):
                for _ in range(WARM):
                    fn()
            for _ in range(ROUNDS):
                for name, fn in routes:
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize(); ekf.synchronize()
                    t0.record()
                    for _ in range(iters):
                        fn()
                    t1.record()
                    torch.cuda.synchronize()
                    times[name].append(t0.elapsed_time(t1) / iters * 1e3)
            n = float(io.budget(xt).n[0])
            rows.append((B, dtype, iters, n, {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}))
            print(B, dtype, {k: [round(x, 1) for x in v] for k, v in times.items()}, flush=True)
            io.close()
            seq.close()
            ekf.close()
            del xt
            torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        f.write("# One error budget: `k_budget` against `k_nees` and the torch route\n\n")
        f.write(f"`profiles/measure_budget.py --head \"{a.head}\" --filters {' '.join(map(str, a.filters))}`: microseconds per call from device tensors, HIP events\n"
                f"on the caller's stream around a block of calls, after {WARM} warm-up calls of every route; {ROUNDS} rounds with the routes alternating:\n"
                "median (min .. max).  MI355X, one process.\n\n")
        f.write("| filters | dtype | calls per block | counted | `budget` | `nees(return_err=True)` | `nees` err + `state()` + torch sums | budget / nees |\n|---|---|---|---|---|---|---|---|\n")
        for B, dtype, iters, n, t in rows:
            cell = lambda k: f"{t[k][0]:.1f} ({t[k][1]:.1f} .. {t[k][2]:.1f})"   # noqa: E731
            f.write(f"| {B} | {dtype} | {iters} | {n:.0f} | {cell('budget')} | {cell('nees')} | {cell('torch')} | {t['budget'][0] / t['nees'][0]:.2f} |\n")
        f.write(f"\nTaken on {a.head}.\n")


if __name__ == "__main__":
    main()
