#!/usr/bin/env python3
"""Time of the lifecycle kernels by HIP events (profiles/r08_health.md).

    python profiles/measure_health.py DTYPE B [LAUNCHES]

DTYPE is f32 or f64, B the number of filters (65536, 2097152).  The run seeds B filters from device tensors, runs a few ticks, then
times, each with qle_timer_begin / qle_timer_end (HIP events on the handle's stream) around ONE call, LAUNCHES (default 120) calls after
20 warm-up calls, and prints one JSON line with the median, the minimum and the 10 % / 90 % quantiles in microseconds:
    health          DeviceIO.health without a summary: k_health alone
    health_summary  with the summary: k_health + k_health_reduce
    seed_slot       qle_initialize_state_slot alone (k_seed reading the tag slot; the pack is outside the timed region)
    nees            DeviceIO.nees with a summary (k_nees + k_nees_reduce): the comparison -- it reads the same record and runs the same
                    factorisation
    nees_alone      qcs_nees without a summary (k_nees alone)
An event pair around a single launch includes the launch's own dispatch latency (a few microseconds); it is the same for every row.
Algorithmic bytes per filter: health reads 136 words (64 compact) and writes 2 bytes; seed reads 8 + 16 words and writes 136."""
import ctypes as C
import json
import statistics
import sys


def main():
    import numpy as np
    import torch

    import quadrotor_landing_amd as qla
    from quadrotor_landing_amd import consistency as cs
    from quadrotor_landing_amd._lib import check, lib

    dtype, B = sys.argv[1], int(sys.argv[2])
    n_timed = int(sys.argv[3]) if len(sys.argv) > 3 else 120
    warm = 20
    kw = dict(update_freq=400.0, measurement_freq=30.0, direct_orien_method=1, Q_a=[0.0005] * 3, Q_w=[0.00005] * 3,
              R_r=[0.015, 0.015, 0.020], R_ang=[0.0015, 0.0015, 0.04])
    ekf = qla.BatchedRelativePoseEKF(B, dtype, **kw)
    io = qla.DeviceIO(ekf)
    g = torch.Generator(device="cuda:0"); g.manual_seed(8)
    z = torch.zeros((B, 7), dtype=torch.float32, device="cuda:0")
    z[:, :3] = torch.rand((B, 3), generator=g, device="cuda:0") * 2.0 - 1.0; z[:, 2] += 2.5
    q = torch.randn((B, 4), generator=g, device="cuda:0") * 0.1; q[:, 3] = 1.0
    z[:, 3:] = q / q.norm(dim=1, keepdim=True)
    u = torch.randn((B, 6), generator=g, device="cuda:0") * 0.05; u[:, 2] += 9.8
    mask = torch.ones(B, dtype=torch.uint8, device="cuda:0")
    io.seed(z, mask)
    for k in range(8):
        io.tick(u, z if k % 4 == 3 else None)
    x, _ = io.state()
    xt = x.clone()
    torch.cuda.synchronize(); ekf.synchronize()
    view = io._view()
    K = cs.consistency_lib()
    nees_out = torch.empty(B, dtype=x.dtype, device="cuda:0")

    def nees_alone():
        cs.ccheck(K.qcs_nees(C.byref(view), C.byref(ekf.params), xt.data_ptr(), 0 if x.dtype == torch.float32 else 1, None,
                             31 if ekf.num_states == 15 else 7, float("inf"), nees_out.data_ptr(), None, None, 0 if x.dtype == torch.float32 else 1))

    rows = {
        "health": lambda: io.health(),
        "health_summary": lambda: io.health(return_summary=True),
        "seed_slot": lambda: check(lib().qle_initialize_state_slot(ekf._h, io._seq._h, 1, 0)),
        "nees": lambda: io.nees(xt),
        "nees_alone": nees_alone,
    }
    out = dict(dtype=dtype, filters=B, n=ekf.num_states, record_words=ekf.policy()["record_words"], timed=n_timed, warmup=warm)
    for name, fn in rows.items():
        for _ in range(warm):
            fn()
        ekf.synchronize(); torch.cuda.synchronize()
        us = []
        for _ in range(n_timed):
            ekf.timer_begin()
            fn()
            us.append(ekf.timer_end() * 1e3)
        us.sort()
        out[name] = dict(median_us=round(statistics.median(us), 2), min_us=round(us[0], 2), p10_us=round(us[len(us) // 10], 2),
                         p90_us=round(us[(9 * len(us)) // 10], 2))
    _, flagged, summ = io.health(return_summary=True)
    torch.cuda.synchronize()
    out["summary"] = [float(v) for v in summ.cpu().numpy()]
    assert np.isfinite(out["summary"]).all()
    print(json.dumps(out))
    io.close()
    ekf.close()


if __name__ == "__main__":
    main()
