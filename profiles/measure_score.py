#!/usr/bin/env python3
"""Cost of one scored tag tick against the route without libqle_score.so (profiles/score.md).

    python profiles/measure_score.py --head REV [--filters 65536] [--out profiles/score.md]

For fp32 and fp64, B filters seeded by the synthetic generator and a few ticks in: times, by the wall clock around a synchronisation
(ITER iterations after WARM, every iteration one tag tick from device tensors),
    plain    io.tick(u, z)                                             the tick alone, for scale
    scored   scorer.observe(u, z) + io.tick(u, z)                      k_score in front of the tick (one more pack, one more launch)
    before   io.tick(u, z, chi2_max=inf, return_nis=True) + torch      what a caller had: the gate's nu and S written out ([B,43] words),
                                                                      torch.linalg.slogdet and the elementwise accumulation of the same
                                                                      36 words per filter -- and a run whose mask words the gate wrote
and writes the table, with REV (the revision the numbers were taken on; the tree the script runs in is not a git checkout everywhere),
to --out.  No pass bound: nobody has measured this before."""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ITER, WARM = 2000, 50


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--head", required=True)
    ap.add_argument("--filters", type=int, default=65536)
    ap.add_argument("--out", default="profiles/score.md")
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
        x0, P0 = ekf.get_state()
        io = qla.DeviceIO(ekf)
        sc = io.scorer()
        A = torch.zeros((36, B), dtype=torch.float64, device="cuda:0")

        def plain():
            io.tick(u, z)

        def scored():
            sc.observe(u, z)
            io.tick(u, z)

        def before():
            acc, nis, nu, S = io.tick(u, z, chi2_max=math.inf, return_nis=True)
            ok = acc.bool() & torch.isfinite(nis)
            okd = ok.double()
            nud, nisd = nu.double().T, nis.double()
            pair = okd * (A[0] >= 1).double()
            A[0] += okd
            A[1] += torch.where(ok, nisd, 0.0)
            A[2] += torch.where(ok, nisd * nisd, 0.0)
            A[3] += torch.where(ok, torch.linalg.slogdet(S.double())[1], 0.0)
            A[4] += (acc == 0).double()
            A[5] += pair
            A[6:12] += torch.where(ok, nud, 0.0)
            A[12:18] += torch.where(ok, nud * nud, 0.0)
            A[18:24] += torch.where(ok, torch.diagonal(S, dim1=1, dim2=2).double().T, 0.0)
            A[24:30] += pair * nud * A[30:36]
            A[30:36] = torch.where(ok, nud, A[30:36])

        times = {}
        for name, fn in (("plain", plain), ("scored", scored), ("before", before), ("plain again", plain)):
            ekf.set_state(x0, P0)   # every route starts from the same state; the tag pose stays near it for a few hundred ticks' worth of cost
            for _ in range(WARM):
                fn()
            torch.cuda.synchronize(); ekf.synchronize()
            t0 = time.perf_counter()
            for _ in range(ITER):
                fn()
            torch.cuda.synchronize(); ekf.synchronize()
            times[name] = (time.perf_counter() - t0) / ITER * 1e6
        rows.append((dtype, times))
        print(dtype, {k: round(v, 1) for k, v in times.items()})
        io.close()
        seq.close()
        ekf.close()
    with open(a.out, "w") as f:
        f.write("# One scored tag tick: `k_score` against the route without it\n\n")
        f.write(f"`profiles/measure_score.py --head \"{a.head}\" --filters {B}`: microseconds per tag tick fed from device tensors, wall clock around a\n"
                f"synchronisation, mean of {ITER} iterations after {WARM}; MI355X, one process.  Host launch overhead is part of every figure.\n\n")
        f.write("| dtype | plain tick | scored: `observe` + `tick` | before: gated tick with `nu`, `S` + torch accumulation | plain tick, again |\n|---|---|---|---|---|\n")
        for dtype, t in rows:
            f.write(f"| {dtype} | {t['plain']:.1f} | {t['scored']:.1f} | {t['before']:.1f} | {t['plain again']:.1f} |\n")
        f.write(f"\nTaken on {a.head}.  The two plain columns bracket the run-to-run spread of the same call.  The route before also leaves the\n"
                "mask words the gate wrote in the slot; the scored tick is the plain tick.\n")


if __name__ == "__main__":
    main()
