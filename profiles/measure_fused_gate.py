#!/usr/bin/env python3
"""Kernel-time comparison of the two gated ticks at 65 536 filters (profiles/r06_fused_gate.md section 3).

    rocprofv3 --kernel-trace --stats -f csv -d DIR -o NAME -- python profiles/measure_fused_gate.py DTYPE [KIND ...]
    python profiles/measure_fused_gate.py --summarize DIR [DIR ...]

DTYPE is f32 or f64; KIND is any of
    three   the host-array qle_step_gated: k_predict + k_innov<..., true> + k_update, three launches
    gate    the gate in front of the fused tick: k_pregate + k_step, DeviceIO.tick(chi2_max=...)
    plain   the ungated tick: k_step alone, DeviceIO.tick()
(default: all three; a commit without the gate library runs `three plain`).  200 ticks of each kind, direct orientation method, every
filter carries a tag pose, chi2_max = inf so that every correction is applied.  The run prints the launch counts only; the kernel times
are the profiler's.  --summarize reads the *kernel_trace.csv of each profiler directory and prints, per kernel family, the launches and
the mean / median / min duration after the first 10 launches of the family; k_step is listed apart for the ticks whose previous kernel
was k_pregate and for the others."""
import collections
import csv
import glob
import os
import statistics
import sys

B, N, SKIP = 65536, 200, 10
FAMILIES = ("k_predict", "k_innov", "k_update", "k_pregate", "k_step")


def family(name):
    for f in FAMILIES:
        if f"qle::{f}<" in name or name.startswith(f + "<") or f" {f}<" in name:
            return f
    return None


def summarize(dirs):
    for d in dirs:
        rows = []
        for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)):
            rows += list(csv.DictReader(open(f)))
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        dur, names, prev = collections.defaultdict(list), collections.defaultdict(set), None
        for r in rows:
            fam = family(r["Kernel_Name"])
            if fam == "k_step":
                fam = "k_step behind k_pregate" if prev == "k_pregate" else "k_step alone"
            if fam:
                dur[fam].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
                names[fam].add(r["Kernel_Name"])
            prev = family(r["Kernel_Name"])
        print(f"## {d}")
        print("| kernel | launches | mean us | median us | min us |")
        print("|---|---|---|---|---|")
        for fam, v in dur.items():
            w = v[SKIP:] if len(v) > SKIP else v
            print(f"| `{fam}` | {len(v)} | {statistics.mean(w) / 1e3:.2f} | {statistics.median(w) / 1e3:.2f} | {min(w) / 1e3:.2f} |")
        for fam, s in names.items():
            for n in sorted(s):
                print(f"{fam}: {n[:160]}")
        print()


def main():
    if sys.argv[1:2] == ["--summarize"]:
        return summarize(sys.argv[2:])
    import numpy as np
    import torch

    import quadrotor_landing_amd as qla

    dtype = sys.argv[1] if len(sys.argv) > 1 else "f32"
    kinds = sys.argv[2:] or ["three", "gate", "plain"]
    kw = dict(update_freq=400.0, measurement_freq=30.0, direct_orien_method=1, Q_a=[0.0005] * 3, Q_w=[0.00005] * 3,
              R_r=[0.015, 0.015, 0.020], R_ang=[0.0015, 0.0015, 0.04])
    ekf = qla.BatchedRelativePoseEKF(B, dtype, **kw)
    seq = ekf.make_inputs(4, [0, 0, 0, 1])
    ekf.synth_generate(seq, seed=0xE4F00006)
    x0, P0 = ekf.get_state()
    u, z, _ = seq.download_tick(3)
    td = torch.float32 if dtype == "f32" else torch.float64
    ut, zt = torch.from_numpy(u).to(td).to("cuda:0"), torch.from_numpy(z).to(td).to("cuda:0")
    io = qla.DeviceIO(ekf)
    for kind in kinds:
        ekf.set_state(x0, P0)
        for _ in range(N):
            if kind == "three":
                ekf.step_gated(u, z, np.inf)
            elif kind == "gate":
                io.tick(ut, zt, chi2_max=np.inf)
            elif kind == "plain":
                io.tick(ut, zt)
            else:
                sys.exit(f"unknown kind {kind}")
        ekf.synchronize()
        print(f"{kind}: non-finite filters after {N} ticks: {ekf.count_nonfinite()}")
    gl = qla.gate.gate_lib().qgt_launch_count() if "gate" in kinds else 0
    print(f"{dtype}: {N} ticks of each of {kinds} at {B} filters; gate launches {gl}")
    io.close()
    ekf.close()


if __name__ == "__main__":
    main()
