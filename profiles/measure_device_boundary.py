#!/usr/bin/env python3
"""The device-tensor boundary (quadrotor_landing_amd/devio.py) next to the host-buffer boundary and the resident ceiling.

In one process on one MI355X, on the cfg 3 schedule (tag poses every 14th tick):
  (a) the host-buffer boundary: qle_step from host fp64 arrays per tick (DESIGN.md section 5's PCIe-inclusive row), re-measured here;
  (b) the new path: DeviceIO.tick from float32 torch tensors plus report(float32) every tick;
  (c) qle_run over a device-resident sequence: the ceiling (b) cannot exceed;
  (d) the three boundary kernels alone, HIP events on the handle's stream over back-to-back launches: us per launch and achieved
      GB/s = (bytes read + bytes written) / time, beside k_predict's own rate at the same batch.
Medians over repeats after a warm-up; the box and the commit are stamped into the output (one JSON line on stdout).
usage: measure_device_boundary.py [--out FILE] [--quick]"""
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
from quadrotor_landing_amd import devio  # noqa: E402

T = 140
THM = np.zeros(T, np.uint8); THM[13::14] = 1


def median_of(fn, reps):
    return statistics.median(fn() for _ in range(reps))


def schedule(B, dtype, reps, host_path):
    """ticks/s of (a), (b), (c) for B filters; wall clock around T ticks, synchronised at both ends."""
    ekf = qla.BatchedRelativePoseEKF(B, dtype, **CFG3)
    seq = ekf.make_inputs(T, THM)
    ekf.synth_generate(seq, seed=0xE4F00003)
    U, Z = [], []
    for t in range(T):
        u, z, _ = seq.download_tick(t)
        U.append(u); Z.append(z if THM[t] else None)
    io = qla.DeviceIO(ekf)
    Ud = [torch.from_numpy(u.astype(np.float32)).cuda() for u in U]
    Zd = [None if z is None else torch.from_numpy(z.astype(np.float32)).cuda() for z in Z]
    out = {k: torch.empty((B,) + s, dtype=torch.float32, device="cuda:0") for k, s in io._REPORT}

    def wall(body):
        torch.cuda.synchronize(); ekf.synchronize()
        t0 = time.perf_counter()
        body()
        torch.cuda.synchronize(); ekf.synchronize()
        return (time.perf_counter() - t0) / T

    def host():
        for t in range(T):
            ekf.step(U[t], Z[t])

    def tensors():
        for t in range(T):
            io.tick(Ud[t], Zd[t])
            io.report(out=out)

    def tensors_no_report():
        for t in range(T):
            io.tick(Ud[t], Zd[t])

    def resident():
        ekf.run(seq, 0, T)

    res = {}
    for name, body in (("a_host_buffer", host), ("b_device_tensors_with_report", tensors), ("b_device_tensors_tick_only", tensors_no_report),
                       ("c_resident_sequence", resident)):
        if name == "a_host_buffer" and not host_path:
            continue
        wall(body)   # warm-up
        s = median_of(lambda: wall(body), reps)
        res[name] = {"us_per_tick": s * 1e6, "ticks_per_s": B / s}
    if "a_host_buffer" in res:
        res["b_over_a"] = res["b_device_tensors_with_report"]["ticks_per_s"] / res["a_host_buffer"]["ticks_per_s"]
    res["b_over_c"] = res["b_device_tensors_with_report"]["ticks_per_s"] / res["c_resident_sequence"]["ticks_per_s"]
    res["policy"] = ekf.policy()
    ekf.close()
    return res


def kernels(B, dtype, reps, launches=200):
    """(d): the boundary kernels alone, float32 tensors, HIP events on the handle's stream."""
    ekf = qla.BatchedRelativePoseEKF(B, dtype, **CFG3)
    pred = np.zeros(16, np.uint8)
    seq = ekf.make_inputs(16, pred)
    ekf.synth_generate(seq, seed=0xE4F00003)
    io = qla.DeviceIO(ekf)
    D = devio.devio_lib()
    w = 4 if dtype == "f32" else 8
    n = ekf.num_states
    u = torch.randn((B, 6), dtype=torch.float32, device="cuda:0"); z = torch.randn((B, 7), dtype=torch.float32, device="cuda:0")
    x = torch.empty((B, 16), dtype=torch.float32, device="cuda:0"); P = torch.empty((B, n, n), dtype=torch.float32, device="cuda:0")
    rep = {k: torch.empty((B,) + s, dtype=torch.float32, device="cuda:0") for k, s in io._REPORT}
    io.tick(u, z); io.tick(u)
    torch.cuda.synchronize(); ekf.synchronize()
    view = io._view(); iv0 = io._inputs_view(0); iv1 = io._inputs_view(1)
    vb = C.byref(view)
    rp = [rep[k].data_ptr() for k, _ in io._REPORT]
    rec = view.record_words
    cases = {
        "k_dv_pack (u)": (lambda: D.qdv_pack_inputs(vb, C.byref(iv0), u.data_ptr(), None, None, 0), B * 6 * (4 + w)),
        "k_dv_pack (u, z)": (lambda: D.qdv_pack_inputs(vb, C.byref(iv1), u.data_ptr(), z.data_ptr(), None, 0), B * (13 * 4 + 14 * w)),
        "k_dv_state (x, P)": (lambda: D.qdv_unpack_state(vb, x.data_ptr(), P.data_ptr(), 0), B * (rec * w + (16 + n * n) * 4)),
        "k_dv_state (x)": (lambda: D.qdv_unpack_state(vb, x.data_ptr(), None, 0), B * 16 * (w + 4)),
        "k_dv_report": (lambda: D.qdv_unpack_report(vb, rp[0], rp[1], rp[2], rp[3], 0), B * ((16 + 21) * w + 52 * 4)),
        "k_predict (qle_run, predict-only ticks)": (lambda: qla._lib.check(qla.lib().qle_run(ekf._h, seq._h, 0, 1)), ekf.algorithmic_bytes(0)),
    }
    res = {}
    for name, (call, nbytes) in cases.items():
        def timed():
            ekf.timer_begin()
            for _ in range(launches):
                rc = call()
                assert not rc, rc
            return ekf.timer_end() / launches * 1e3   # us per launch
        timed()   # warm-up
        us = median_of(timed, reps)
        res[name] = {"us_per_launch": us, "bytes": int(nbytes), "GB_per_s": nbytes / us * 1e-3}
    ekf.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer repeats (a smoke run of the script)")
    a = ap.parse_args()
    reps = 3 if a.quick else 7
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    prop = torch.cuda.get_device_properties(0)
    doc = {"device": prop.name, "cus": prop.multi_processor_count, "host": os.uname().nodename, "commit_parent": commit,
           "torch": torch.__version__, "schedule": "cfg 3: 140 ticks, tag poses every 14th", "repeats": reps, "runs": {}}
    for label, B, dtype, host_path in (("65536 f32", 65536, "f32", True), ("65536 f64", 65536, "f64", True), ("2097152 f32", 2097152, "f32", False)):
        doc["runs"][label] = {"schedule": schedule(B, dtype, reps, host_path), "kernels": kernels(B, dtype, reps)}
    line = json.dumps(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
