#!/usr/bin/env python3
"""Time of the device state I/O by HIP events (profiles/stateio.md).

    python profiles/measure_stateio.py DTYPE [B] [REPEATS] [INNER]

DTYPE is f32 or f64, B the number of filters (default 65536).  The run seeds B filters from device tensors, runs a few ticks, then times
each row REPEATS (default 20) times after 3 warm-up rounds, with qle_timer_begin / qle_timer_end (HIP events on the handle's stream)
around INNER (default 10) calls of the row back to back, and prints one JSON line with the median, the minimum and the 10 % / 90 %
quantiles of the time PER CALL in microseconds:
    predict         qle_run over one predict-only tick of a device-resident sequence: ONE launch of the predict kernel, which reads and
                    writes every record word once -- the bytes of an identity copy in each direction: the first yardstick
    snapshot        a snapshot into a workspace that exists (what `gather` does first): ONE launch of k_si_copy, identity index
    snapshot_alloc  DeviceIO.snapshot(): the same with a fresh workspace tensor per call (host work outside the stream)
    restore         DeviceIO.restore(snap): ONE launch of k_si_copy, identity index
    set_state       DeviceIO.set_state(x, P) from tensors of the compute dtype: ONE launch of k_si_pack
    gather_perm     DeviceIO.gather(index) with a random permutation: two launches, the second with one 16-byte access per lane and row
    fork4           DeviceIO.fork(4): two launches, the second reading every fourth record four times
    host_route      the only route without this library: DeviceIO.state() -> host -> BatchedRelativePoseEKF.set_state, by the host
                    clock around the whole of it, ending in a synchronise (HOST_REPEATS rounds; 241 doubles per filter each way)
Every row includes the host work of its Python call (view query, two stream orderings, the mark of the tick library); with INNER calls
per event pair the launches queue behind one another, so a row approaches the device time per call from above.
Algorithmic bytes per filter: predict, snapshot and restore read and write record_words words of the compute dtype; gather and fork twice
that; set_state reads 16 + n * n words and writes record_words."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch

    import quadrotor_landing_amd as qla
    from quadrotor_landing_amd import stateio

    dtype = sys.argv[1]
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
    n_timed = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    inner = int(sys.argv[4]) if len(sys.argv) > 4 else 10
    warm = 3
    host_repeats = 5 if B <= 262144 else 2
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
    io.seed(z)
    for k in range(8):
        io.tick(u, z if k % 4 == 3 else None)
    seq = ekf.make_inputs(1)
    seq.upload_tick(0, u.double().cpu().numpy())
    x, P = io.state()
    snap = io.snapshot()
    kept = io.snapshot()
    perm = torch.randperm(B, generator=g, device="cuda:0").to(torch.int32)
    torch.cuda.synchronize(); ekf.synchronize()

    def timed(fn):
        us = []
        for k in range(warm + n_timed):
            ekf.synchronize(); torch.cuda.synchronize()
            ekf.timer_begin()
            for _ in range(inner):
                fn()
            ms = ekf.timer_end()
            if k >= warm:
                us.append(ms * 1e3 / inner)
        return quantiles(us)

    def quantiles(us):
        us = sorted(us)
        return dict(median_us=round(statistics.median(us), 2), min_us=round(us[0], 2), p10_us=round(us[len(us) // 10], 2),
                    p90_us=round(us[(9 * len(us)) // 10], 2))

    def host_route():
        us = []
        for _ in range(host_repeats):
            ekf.synchronize(); torch.cuda.synchronize()
            t0 = time.perf_counter()
            xs, Ps = io.state(dtype="float64")
            ekf.set_state(xs.cpu().numpy(), Ps.cpu().numpy())
            ekf.synchronize()
            us.append((time.perf_counter() - t0) * 1e6)
        return quantiles(us)

    rows = {
        "predict": lambda: ekf.run(seq, 0, 1),
        "snapshot": lambda: stateio.snapshot(io, into=kept),
        "snapshot_alloc": io.snapshot,
        "restore": lambda: io.restore(snap),
        "set_state": lambda: io.set_state(x, P),
        "gather_perm": lambda: io.gather(perm),
        "fork4": lambda: io.fork(4),
    }
    policy = ekf.policy()
    out = dict(dtype=dtype, filters=B, n=ekf.num_states, record_words=policy["record_words"], state_policy=policy["state_policy"],
               timed=n_timed, inner=inner, warmup=warm, host_repeats=host_repeats, rows={})
    for name, fn in rows.items():
        io.restore(snap)   # every row starts from the same records
        out["rows"][name] = timed(fn)
    io.restore(snap)
    out["rows"]["host_route"] = host_route()
    xf, _ = io.state()
    assert bool(torch.isfinite(xf).all())
    print(json.dumps(out))
    io.close(); ekf.close()


if __name__ == "__main__":
    main()
