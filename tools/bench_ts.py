#!/usr/bin/env python3
"""Cost of the transport-stream mux on the C2 workload (easydarwin_amd/workload.py: 1024 sessions x
16 UDP subscribers) with every video track tapped: per step one drain into a device buffer and one
mux of it into another device buffer, per tick length.

  python tools/bench_ts.py [--sessions 1024] [--subs 16] [--ticks 1000,100,20] [--steps 10]

Reports the step time with drain + mux and with the drain alone, the mux's device time by event
pairs (edgpu_kernel_times(6): plan + place + pack, not timed apart) beside the drain's
(edgpu_kernel_times(5)) from the same run, and (ES bytes read + TS bytes written) / mux time as a
fraction of the 8 TB/s the README uses.  One JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from easydarwin_amd import edgpu  # noqa: E402
from easydarwin_amd.workload import H264Fleet  # noqa: E402

PEAK = 8e12


def measure(tick_ms: int, sessions: int, subs: int, steps: int, warm: int) -> dict:
    dev = torch.device("cuda", 0)
    fleet = H264Fleet(np.arange(sessions), tick_ms=tick_ms)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0xEA5D)
    need = warm + steps
    host = [fleet.next_batch() for _ in range(need)]
    base = [bench.make_batch_on_device(b, dev, gen) for b in host]
    del host
    torch.cuda.synchronize(dev)
    max_pk = max(b["n"] for b in base)
    max_by = max(b["bytes"] for b in base)
    ctx = edgpu.Context(device=0, video_ring_packets=8192, video_ring_bytes=16 << 20, other_ring_packets=256,
                        other_ring_bytes=64 << 10, max_batch_packets=max_pk + 1, max_batch_bytes=1 << 20,
                        out_arena_bytes=int(max_by * subs * 1.05) // 16 * 16 + (1 << 20),
                        max_out_packets=int(max_pk * subs * 1.05) + 1024)
    sess = []
    for _ in range(sessions):
        s = ctx.session_add(fleet.sdp())
        sess.append(s)
        for _k in range(subs):
            ctx.subscriber_add(s, edgpu.TRANSPORT_UDP)
    es = ctx.device_alloc(4 * max_by + (sessions << 8) + (1 << 20))
    ts = ctx.device_alloc(6 * max_by + (sessions << 12) + (1 << 20))
    states = np.zeros(sessions, dtype=edgpu.TS_STATE_DTYPE)
    span = need * tick_ms
    epoch = [0]

    def run(mux: bool, timing: int):
        bts = [bench.later_batch(ctx, b, epoch[0] * span) if epoch[0] else b for b in base]
        epoch[0] += 1
        ctx.set_timing(timing)
        done = []

        def step(i):
            bench.run_step(ctx, bts[i])
            n, units, streams = ctx.tap_drain(out=es)
            if mux:
                rows = np.zeros(len(units), dtype=edgpu.TS_UNIT_DTYPE)
                rc, res = ctx.ts_mux_raw(None, es.ptr, n, edgpu.PTR_DEVICE, units, streams, states[:len(streams)],
                                         ts.ptr, ts.nbytes, edgpu.PTR_DEVICE, rows)
                if rc:
                    raise SystemExit(f"edgpu_ts_mux: {rc}")
                done.append((int(streams["bytes"].sum()), int(res.bytes), len(units)))

        for i in range(warm):
            step(i)
        ctx.sync()
        ctx.kernel_times(5)
        ctx.kernel_times(6)
        t0 = time.perf_counter()
        for i in range(warm, need):
            step(i)
        ctx.sync()
        dt = (time.perf_counter() - t0) / steps
        if ctx.stats().status != 0:
            raise SystemExit(f"engine status {ctx.stats().status}")
        return dt, done

    for s in sess:
        ctx.tap_enable(s, 0)
    run(False, ctx.TIMING_FANOUT)                   # first pass: rings and tables settle
    off, _ = run(False, ctx.TIMING_FANOUT)
    on, _ = run(True, ctx.TIMING_FANOUT)
    _, done = run(True, ctx.TIMING_ALL)
    k5, k6 = ctx.kernel_times(5), ctx.kernel_times(6)
    es.free()
    ts.free()
    ctx.close()
    read = float(np.mean([d[0] for d in done])) if done else 0.0
    written = float(np.mean([d[1] for d in done])) if done else 0.0
    m6 = float(np.mean(k6)) if k6 else None
    return {"tick_ms": tick_ms, "packets_per_step": int(np.mean([b["n"] for b in base])),
            "step_ms_drain_only": round(1e3 * off, 4), "step_ms_drain_and_mux": round(1e3 * on, 4),
            "mux_us": [round(1e3 * v, 2) for v in k6], "mux_us_mean": round(1e3 * m6, 2) if k6 else None,
            "mux_us_min": round(1e3 * float(np.min(k6)), 2) if k6 else None,
            "drain_us_mean": round(1e3 * float(np.mean(k5)), 2) if k5 else None,
            "es_bytes_read_per_step": int(read), "ts_bytes_written_per_step": int(written),
            "units_per_step": int(np.mean([d[2] for d in done])) if done else 0,
            "fraction_of_peak": round((read + written) / (m6 * 1e-3) / PEAK, 4) if k6 else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=1024)
    ap.add_argument("--subs", type=int, default=16)
    ap.add_argument("--ticks", default="1000,100,20")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    edgpu.load()
    res = [measure(int(t), args.sessions, args.subs, args.steps, args.warmup) for t in args.ticks.split(",")]
    print(json.dumps({"bench": "ts", "sessions": args.sessions, "subs": args.subs, "results": res}))


if __name__ == "__main__":
    main()
