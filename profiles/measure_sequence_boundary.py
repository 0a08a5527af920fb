#!/usr/bin/env python3
"""The sequence boundary (DeviceIO.sequence / run, libqle_sequence.so) next to the per-tick device-tensor boundary and the resident
ceiling.

In one process on one MI355X at 65 536 filters on the cfg 3 schedule (140 ticks, tag poses every 14th), fp32 and fp64, float32
tensors, wall clock around the 140 ticks synchronised at both ends, median over repeats after a warm-up, in us per tick:
  (b) the DeviceIO.tick loop, with and without DeviceIO.report every tick: the path as it was, measured in the same run;
  (s) the pack of the whole sequence (DeviceSequence.pack into an existing sequence) + ONE DeviceIO.run, with and without a report
      trace on every tick; and DeviceIO.sequence + run, which also creates the sequence (allocation and a synchronous copy of the
      slot table) inside the timed region;
  (c) ekf.run over the same resident sequence: the ceiling;
  (p) the pack alone: HIP events on the handle's stream over back-to-back qsq_pack calls of the whole sequence, bytes moved / time.
The box and the commit are stamped into the output (one JSON line on stdout; --out writes the JSON and a markdown table beside it).
usage: measure_sequence_boundary.py [--out FILE.json] [--quick] [--commit ID]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import quadrotor_landing_amd as qla  # noqa: E402
from bench import CFG3  # noqa: E402
from quadrotor_landing_amd import sequence  # noqa: E402

T = 140
THM = np.zeros(T, np.uint8); THM[13::14] = 1
TAGS = [int(t) for t in np.flatnonzero(THM)]


def median_of(fn, reps):
    return statistics.median(fn() for _ in range(reps))


def measure(B, dtype, reps):
    ekf = qla.BatchedRelativePoseEKF(B, dtype, **CFG3)
    seq = ekf.make_inputs(T, THM)
    ekf.synth_generate(seq, seed=0xE4F00003)
    U = np.empty((T, B, 6), np.float32); Z = np.empty((len(TAGS), B, 7), np.float32)
    for t in range(T):
        u, z, _ = seq.download_tick(t)
        U[t] = u
        if THM[t]:
            Z[TAGS.index(t)] = z
    io = qla.DeviceIO(ekf)
    Us, Zs = torch.from_numpy(U).cuda(), torch.from_numpy(Z).cuda()
    Ud = [Us[t] for t in range(T)]                                    # B = 65536: every slab starts on a 16-byte boundary
    Zd = [Zs[TAGS.index(t)] if THM[t] else None for t in range(T)]
    out = {k: torch.empty((B,) + s, dtype=torch.float32, device="cuda:0") for k, s in io._REPORT}
    dseq = io.sequence(Us, Zs, TAGS)
    made = []

    def wall(body):
        torch.cuda.synchronize(); ekf.synchronize()
        t0 = time.perf_counter()
        body()
        torch.cuda.synchronize(); ekf.synchronize()
        return (time.perf_counter() - t0) / T

    def b_tick_report():
        for t in range(T):
            io.tick(Ud[t], Zd[t])
            io.report(out=out)

    def b_tick():
        for t in range(T):
            io.tick(Ud[t], Zd[t])

    def s_pack_run():
        dseq.pack(Us, Zs)
        io.run(dseq)

    def s_pack_run_report():
        dseq.pack(Us, Zs)
        io.run(dseq, trace_every=1, dtype=torch.float32)

    def s_sequence_run():
        made.append(io.sequence(Us, Zs, TAGS))
        io.run(made[-1])

    def c_resident():
        ekf.run(seq, 0, T)

    res = {}
    for name, body in (("b_tick_loop_with_report", b_tick_report), ("b_tick_loop", b_tick), ("s_pack_run", s_pack_run),
                       ("s_pack_run_report_trace", s_pack_run_report), ("s_sequence_run", s_sequence_run), ("c_resident_sequence", c_resident)):
        wall(body)   # warm-up
        s = median_of(lambda: wall(body), reps)
        res[name] = {"us_per_tick": s * 1e6, "ticks_per_s": B / s}
        for d in made:
            d.close()
        made.clear()
        torch.cuda.empty_cache()
    us = {k: v["us_per_tick"] for k, v in res.items()}
    # (p) the pack alone, HIP events on the handle's stream
    S = sequence.sequence_lib()
    view = io._view()
    w = 4 if dtype == "f32" else 8
    nbytes = T * B * 6 * (4 + w) + len(TAGS) * B * (7 * 4 + 8 * w)
    calls = 20

    def packs():
        ekf.timer_begin()
        for _ in range(calls):
            rc = S.qsq_pack(C.byref(view), dseq.inputs._h, 0, T, Us.data_ptr(), Zs.data_ptr(), None, 0)
            assert not rc, S.qsq_last_error()
        return ekf.timer_end() / calls * 1e3   # us per pack of the whole sequence
    packs()
    pus = median_of(packs, reps)
    res["p_pack_alone"] = {"us_per_sequence": pus, "us_per_tick": pus / T, "launches": -(-T // sequence.CHUNK), "bytes": int(nbytes),
                           "GB_per_s": nbytes / pus * 1e-3}
    res["ratios"] = {
        "s_over_c": us["s_pack_run"] / us["c_resident_sequence"],
        "b_over_s": us["b_tick_loop"] / us["s_pack_run"],
        "b_over_s_with_report": us["b_tick_loop_with_report"] / us["s_pack_run_report_trace"],
        "c_plus_pack_share_us": us["c_resident_sequence"] + pus / T,
        "s_minus_c_plus_pack_us": us["s_pack_run"] - (us["c_resident_sequence"] + pus / T),
    }
    res["policy"] = ekf.policy()
    dseq.close(); ekf.close()
    return res


def markdown(doc):
    rows = ["# Sequence boundary at 65 536 filters, cfg 3 schedule", "",
            f"{doc['device']} ({doc['cus']} CUs), host {doc['host']}, commit {doc['commit_parent']} + this change, torch {doc['torch']}; "
            f"{doc['schedule']}; median of {doc['repeats']} after a warm-up; us per tick.", "",
            "| path | fp32 | fp64 |", "|---|---|---|"]
    names = (("b_tick_loop_with_report", "(b) `io.tick` + `io.report` per tick"), ("b_tick_loop", "(b) `io.tick` loop"),
             ("s_pack_run_report_trace", "(s) pack + `io.run`, report trace every tick"), ("s_pack_run", "(s) pack + `io.run`"),
             ("s_sequence_run", "(s) `io.sequence` + `io.run` (creates the sequence)"), ("c_resident_sequence", "(c) `ekf.run`, resident"))
    r = doc["runs"]
    for key, label in names:
        rows.append(f"| {label} | {r['65536 f32'][key]['us_per_tick']:.2f} | {r['65536 f64'][key]['us_per_tick']:.2f} |")
    p = [r[k]["p_pack_alone"] for k in ("65536 f32", "65536 f64")]
    rows.append(f"| (p) pack alone, per tick ({p[0]['launches']} launches per sequence) | {p[0]['us_per_tick']:.2f} | {p[1]['us_per_tick']:.2f} |")
    rows.append(f"| (p) pack alone, GB/s | {p[0]['GB_per_s']:.0f} | {p[1]['GB_per_s']:.0f} |")
    for key, label in (("s_over_c", "(s) / (c)"), ("b_over_s", "(b) / (s)"), ("b_over_s_with_report", "(b) / (s), both with the report"),
                       ("s_minus_c_plus_pack_us", "(s) - ((c) + pack share), us")):
        rows.append(f"| {label} | {r['65536 f32']['ratios'][key]:.3f} | {r['65536 f64']['ratios'][key]:.3f} |")
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer repeats (a smoke run of the script)")
    ap.add_argument("--commit", default=None, help="the commit this tree was made from, where the tree carries no history")
    a = ap.parse_args()
    reps = 3 if a.quick else 7
    commit = a.commit
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
        except OSError:
            commit = "unknown"
    prop = torch.cuda.get_device_properties(0)
    doc = {"device": prop.name, "cus": prop.multi_processor_count, "host": os.uname().nodename, "commit_parent": commit,
           "torch": torch.__version__, "schedule": "cfg 3: 140 ticks, tag poses every 14th, float32 tensors", "repeats": reps, "runs": {}}
    for label, B, dtype in (("65536 f32", 65536, "f32"), ("65536 f64", 65536, "f64")):
        doc["runs"][label] = measure(B, dtype, reps)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
        with open(os.path.splitext(a.out)[0] + ".md", "w") as f:
            f.write(markdown(doc))
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
