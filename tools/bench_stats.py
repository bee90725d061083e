#!/usr/bin/env python3
"""Cost of the per-stream statistics on the C2 workload (easydarwin_amd/workload.py: 1024
sessions x 16 UDP subscribers): step time with statistics off and on in one process, and the
stats kernel's mean duration (edgpu_kernel_times(4)), per tick length.

  python tools/bench_stats.py [--sessions 1024] [--subs 16] [--ticks 1000,100,20] [--steps 10]

With statistics on, every session is enabled and each step makes a sample call before its
fan-out.  The step times are taken with the fan-out's event pair only (as bench.py's timed
region); the kernel durations come from extra steps that record every event.  One JSON line.
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


def measure(tick_ms: int, sessions: int, subs: int, steps: int, warm: int, repeats: int) -> dict:
    dev = torch.device("cuda", 0)
    fleet = H264Fleet(np.arange(sessions), tick_ms=tick_ms)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0xEA5D)
    need = warm + steps
    host = [fleet.next_batch() for _ in range(need)]
    per_stream = np.concatenate([np.diff(b["seg_off"].astype(np.int64)) for b in host[warm:]])
    base = [bench.make_batch_on_device(b, dev, gen) for b in host]
    del host
    torch.cuda.synchronize(dev)
    max_pk = max(b["n"] for b in base)
    ctx = edgpu.Context(device=0, video_ring_packets=8192, video_ring_bytes=16 << 20, other_ring_packets=256,
                        other_ring_bytes=64 << 10, max_batch_packets=max_pk + 1, max_batch_bytes=1 << 20,
                        out_arena_bytes=int(max(b["bytes"] for b in base) * subs * 1.05) // 16 * 16 + (1 << 20),
                        max_out_packets=int(max_pk * subs * 1.05) + 1024)
    sess = []
    for _ in range(sessions):
        s = ctx.session_add(fleet.sdp())
        sess.append(s)
        for _k in range(subs):
            ctx.subscriber_add(s, edgpu.TRANSPORT_UDP)
    span = need * tick_ms
    epoch = [0]

    def run(on: bool, timing: int):
        """One pass over the resident batches, a whole span later than the last one."""
        bts = [bench.later_batch(ctx, b, epoch[0] * span) if epoch[0] else b for b in base]
        epoch[0] += 1
        ctx.set_timing(timing)
        for i in range(warm):
            if on:
                ctx.stream_stats_sample(bts[i]["t"])
            bench.run_step(ctx, bts[i])
        ctx.sync()
        ctx.kernel_times(4)
        t0 = time.perf_counter()
        for i in range(warm, need):
            if on:
                ctx.stream_stats_sample(bts[i]["t"])
            bench.run_step(ctx, bts[i])
        ctx.sync()
        dt = (time.perf_counter() - t0) / steps
        if ctx.stats().status != 0:
            raise SystemExit(f"engine status {ctx.stats().status}")
        return dt

    off, on = [], []
    run(False, ctx.TIMING_FANOUT)                   # first pass: rings and tables settle
    for _ in range(repeats):
        off.append(run(False, ctx.TIMING_FANOUT))
        for s in sess:
            ctx.stream_stats_enable(s, base[0]["t"] + epoch[0] * span)
        on.append(run(True, ctx.TIMING_FANOUT))
        for s in sess:
            ctx.stream_stats_disable(s)
    for s in sess:
        ctx.stream_stats_enable(s, base[0]["t"] + epoch[0] * span)
    run(True, ctx.TIMING_ALL)
    k = ctx.kernel_times(4)
    received = int(sum(int(r["received"]) for s in sess[:8] for r in ctx.stream_stats(s)))
    ctx.close()
    return {"tick_ms": tick_ms, "packets_per_step": int(np.mean([b["n"] for b in base])),
            "step_ms_off": [round(1e3 * v, 4) for v in off], "step_ms_on": [round(1e3 * v, 4) for v in on],
            "packets_per_stream_step": {"min": int(per_stream.min()), "mean": round(float(per_stream.mean()), 1),
                                        "max": int(per_stream.max())},
            "stats_kernel_us": [round(1e3 * v, 2) for v in k],
            "stats_kernel_us_mean": round(1e3 * float(np.mean(k)), 2) if k else None,
            "stats_kernel_us_min": round(1e3 * float(np.min(k)), 2) if k else None, "stats_kernel_launches": len(k),
            "received_first8": received}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=1024)
    ap.add_argument("--subs", type=int, default=16)
    ap.add_argument("--ticks", default="1000,100,20")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    edgpu.load()
    out = [measure(int(t), args.sessions, args.subs, args.steps, args.warmup, args.repeats) for t in args.ticks.split(",")]
    print(json.dumps({"bench": "stream_stats", "sessions": args.sessions, "subs": args.subs, "results": out}))


if __name__ == "__main__":
    main()
