#!/usr/bin/env python3
"""Time of the look-ahead kernel by HIP events (profiles/lookahead.md).

    python profiles/measure_lookahead.py DTYPE [B] [REPEATS]

DTYPE is f32 or f64, B the number of filters (default 65536).  The run seeds B filters from device tensors, runs a few ticks, then times,
each with qle_timer_begin / qle_timer_end (HIP events on the handle's stream) around the whole row, REPEATS (default 40) times after 5
warm-up rounds, for h = 1, 8, 32, and prints one JSON line with the median, the minimum and the 10 % / 90 % quantiles in microseconds:
    lookahead       DeviceIO.lookahead(u, h): ONE launch of k_lookahead (the workspace allocation is host work outside the stream)
    lookahead_coast the same with both sigma limits given (ticks_to_limit written)
    predict_host    h launches of qle_predict on a scratch handle with the same state: what a caller has today (each call uploads u)
    run_sequence    qle_run over h predict-only ticks of a device-resident sequence on that scratch handle: h launches of k_predict and
                    nothing else -- the yardstick without the upload
The one-off cost of today's route that no row contains: qle_set_state on the scratch handle (241 doubles per filter over the host).
An event pair includes the dispatch latency of the first launch (a few microseconds); it is the same for every row.
Algorithmic bytes per filter and call: lookahead reads 136 words (64 compact) and 6 of u and writes 136 (64); every predict launch reads
and writes 136 (64) and reads 6."""
import json
import statistics
import sys


def main():
    import torch

    import quadrotor_landing_amd as qla

    dtype = sys.argv[1]
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
    n_timed = int(sys.argv[3]) if len(sys.argv) > 3 else 40
    warm = 5
    horizons = (1, 8, 32)
    kw = dict(update_freq=400.0, measurement_freq=30.0, direct_orien_method=1, Q_a=[0.0005] * 3, Q_w=[0.00005] * 3,
              R_r=[0.015, 0.015, 0.020], R_ang=[0.0015, 0.0015, 0.04])
    ekf = qla.BatchedRelativePoseEKF(B, dtype, **kw)
    scratch = qla.BatchedRelativePoseEKF(B, dtype, **kw)
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
    torch.cuda.synchronize(); ekf.synchronize()
    x0, P0 = ekf.get_state()
    u_host = u.double().cpu().numpy()
    seq = scratch.make_inputs(max(horizons))
    for t in range(max(horizons)):
        seq.upload_tick(t, u_host)

    def timed(handle, fn, reset=None):
        us = []
        for k in range(warm + n_timed):
            if reset is not None:
                reset()
            handle.synchronize(); torch.cuda.synchronize()
            handle.timer_begin()
            fn()
            ms = handle.timer_end()
            if k >= warm:
                us.append(ms * 1e3)
        us.sort()
        return dict(median_us=round(statistics.median(us), 2), min_us=round(us[0], 2), p10_us=round(us[len(us) // 10], 2),
                    p90_us=round(us[(9 * len(us)) // 10], 2))

    out = dict(dtype=dtype, filters=B, n=ekf.num_states, record_words=ekf.policy()["record_words"], timed=n_timed, warmup=warm, rows={})
    for h in horizons:
        def predict_host():
            for _ in range(h):
                scratch.predict(u_host)
        rows = {
            "lookahead": (ekf, lambda: io.lookahead(u, h), None),
            "lookahead_coast": (ekf, lambda: io.lookahead(u, h, sigma_r_max=0.5, sigma_theta_max=0.3), None),
            "predict_host": (scratch, predict_host, lambda: scratch.set_state(x0, P0)),
            "run_sequence": (scratch, lambda: scratch.run(seq, 0, h), lambda: scratch.set_state(x0, P0)),
        }
        out["rows"][f"h={h}"] = {name: timed(*row) for name, row in rows.items()}
    xf, _ = io.lookahead(u, 32).state()
    assert bool(torch.isfinite(xf).all())
    print(json.dumps(out))
    io.close(); scratch.close(); ekf.close()


if __name__ == "__main__":
    main()
