#!/usr/bin/env python3
"""Cost of the consistency diagnostics against the two routes without them (profiles/r07_consistency.md).

    rocprofv3 --kernel-trace --stats -f csv -d DIR -o NAME -- python profiles/measure_consistency.py DTYPE B [routes]
    python profiles/measure_consistency.py --summarize DIR [DIR ...]

DTYPE is f32 or f64, B the number of filters (65536, 1048576).  The run seeds B filters from the synthetic generator, runs 56 matched-noise
ticks (cfg 3), then calls DeviceIO.nees 50 times (k_nees and k_nees_reduce: their times are the profiler's) and prints one JSON line
with the batch mean NEES of the run -- a finding about the filter, not a pass criterion -- and the algorithmic bytes per filter.
With `routes` it also times, by the wall clock around a synchronisation, what a caller had without the library:
    host    get_state (241 doubles per filter over PCIe) + np.linalg.solve per filter
    torch   DeviceIO.state (AoS tensors) + torch.linalg.solve on the n x n matrices (the error vector taken as given: a lower bound)
--summarize prints launches and mean / median / min duration of k_nees and k_nees_reduce after the first 10 launches."""
import collections
import csv
import glob
import json
import os
import statistics
import sys
import time

N, SKIP = 50, 10


def summarize(dirs):
    for d in dirs:
        dur = collections.defaultdict(list)
        for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)):
            for r in csv.DictReader(open(f)):
                for fam in ("k_nees_reduce", "k_nees<"):
                    if fam in r["Kernel_Name"]:
                        dur[fam.rstrip("<")].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
                        break
        print(f"## {d}")
        print("| kernel | launches | mean us | median us | min us |")
        print("|---|---|---|---|---|")
        for fam, v in dur.items():
            w = v[SKIP:] if len(v) > SKIP else v
            print(f"| `{fam}` | {len(v)} | {statistics.mean(w) / 1e3:.2f} | {statistics.median(w) / 1e3:.2f} | {min(w) / 1e3:.2f} |")
        print()


def main():
    if sys.argv[1:2] == ["--summarize"]:
        return summarize(sys.argv[2:])
    import numpy as np
    import torch

    import quadrotor_landing_amd as qla

    dtype, B = sys.argv[1], int(sys.argv[2])
    routes = sys.argv[3:4] == ["routes"]
    kw = dict(update_freq=400.0, measurement_freq=30.0, limit_measurement_freq=1, direct_orien_method=1, Q_a=[0.0005] * 3, Q_w=[0.00005] * 3,
              R_r=[0.015, 0.015, 0.020], R_ang=[0.0015, 0.0015, 0.04])
    T = 56
    thm = np.zeros(T, np.uint8); thm[13::14] = 1
    ekf = qla.BatchedRelativePoseEKF(B, dtype, **kw)
    seq = ekf.make_inputs(T, thm)
    ekf.synth_generate(seq, seed=0xE4F00007)
    ekf.run(seq, 0, T)
    n = ekf.num_states
    s = ekf.synth_nees(seq, chi2_hi=30.0)
    pose, bias = ekf.synth_truth(seq)
    xt = np.zeros((B, 16)); xt[:, 0:3] = pose[:, 0:3]; xt[:, 6:10] = pose[:, 3:7]
    xt[:, 10:16] = bias + np.array(list(ekf.params.ab_static) + list(ekf.params.wb_static))
    td = torch.float32 if dtype == "f32" else torch.float64
    xtt = torch.from_numpy(xt).to(td).to("cuda:0")
    io = qla.DeviceIO(ekf)
    blocks = "r+theta+ab+wb" if n == 15 else "r+theta"
    for _ in range(N):
        io.nees(xtt, blocks=blocks)
    ekf.synchronize()
    w = 4 if dtype == "f32" else 8
    out = dict(dtype=dtype, filters=B, n=n, blocks=blocks, calls=N, mean_nees=s["mean_nees"], dof=s["dof"], count=s["count"], n_above_30=s["n_above"],
               n_not_pd=s["n_not_pd"], bytes_per_filter=(16 + 120 + 16 + 1) * w)
    if routes:
        torch.cuda.synchronize(); t0 = time.perf_counter()
        x, P = ekf.get_state()
        e = np.zeros((B, n)); e[:, 0:3] = xt[:, 0:3] - x[:, 0:3]
        np.einsum("bi,bi->b", e, np.linalg.solve(P, e[:, :, None])[:, :, 0])
        out["host_route_s"] = time.perf_counter() - t0
        torch.cuda.synchronize(); t0 = time.perf_counter()
        xs, Ps = io.state()
        et = torch.zeros((B, n, 1), dtype=td, device="cuda:0")
        (et * torch.linalg.solve(Ps, et)).sum()
        torch.cuda.synchronize()
        out["torch_route_s"] = time.perf_counter() - t0
    print(json.dumps(out))
    io.close()
    ekf.close()


if __name__ == "__main__":
    main()
