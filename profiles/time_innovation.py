#!/usr/bin/env python3
"""Cost of the innovation diagnostics and of the gated tick next to the fused tick (HIP events on the handle's stream).

    python profiles/time_innovation.py <batch> <f32|f64> [n]

Per call, host-buffer entry points (each includes the upload of its tag poses / IMU samples through the staging buffer):
  innovation_us   qle_innovation, every output left on the device (one k_innov launch in diagnostics mode)
  step_gated_us   qle_step_gated at chi2_max = 16.81, outputs left on the device (predict, k_innov as the gate, k_update)
  step_us         qle_step with the same inputs (one fused launch)
and, for scale, run_us: the benchmarked fused tick (qle_run on device-resident inputs, every tick with tag poses).
The kernel times alone come from a `rocprofv3 --kernel-trace --stats` run of this script.  cfg 3 parameters (bench.py).
"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quadrotor_landing_amd as qla  # noqa: E402
from bench import CFG3  # noqa: E402
from quadrotor_landing_amd._lib import check, lib  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
dtype = sys.argv[2] if len(sys.argv) > 2 else "f32"
N = int(sys.argv[3]) if len(sys.argv) > 3 else 50
pd = C.POINTER(C.c_double)

ekf = qla.BatchedRelativePoseEKF(B, dtype, **CFG3)
seq = ekf.make_inputs(14, np.ones(14, np.uint8))
ekf.synth_generate(seq, seed=3)
x0, P0 = ekf.get_state()
u, z, _ = seq.download_tick(0)
up, zp = u.ctypes.data_as(pd), z.ctypes.data_as(pd)
out = {"batch": B, "dtype": dtype, "n": N}


def timed(name, call):
    ekf.set_state(x0, P0)
    call(); call()
    ekf.synchronize()
    ekf.timer_begin()
    for _ in range(N):
        call()
    out[name] = round(ekf.timer_end() / N * 1e3, 2)


timed("innovation_us", lambda: check(lib().qle_innovation(ekf._h, zp, None, None, None, None)))
timed("step_gated_us", lambda: check(lib().qle_step_gated(ekf._h, up, zp, None, C.c_double(16.81), None, None)))
timed("step_us", lambda: check(lib().qle_step(ekf._h, up, zp, None)))
ekf.set_state(x0, P0)
ekf.run(seq, 0, 28); ekf.synchronize()
ekf.timer_begin(); ekf.run(seq, 0, N); out["run_us"] = round(ekf.timer_end() / N * 1e3, 2)
ekf.set_state(x0, P0)
acc, nis = ekf.update_gated(z, 16.81)
out["accepted_share"] = round(float(acc.mean()), 4)
out["nis_mean"] = round(float(np.nanmean(nis)), 3)
out["policy"] = ekf.policy()
out["bad"] = ekf.count_nonfinite()
print(json.dumps(out), flush=True)
ekf.close()
