#!/usr/bin/env python3
"""Cost of the H.264 elementary-stream tap on the C2 workload (easydarwin_amd/workload.py: 1024
sessions x 16 UDP subscribers) with every video track tapped: one drain into a device buffer per
step, per tick length.

  python tools/bench_tap.py [--sessions 1024] [--subs 16] [--ticks 1000,100,20] [--steps 10]

Reports the drain's device time by event pairs (edgpu_kernel_times(5): scan + place + copy), the
step time with the drain and without it, and (ring bytes read + Annex-B bytes written) / drain
time as a fraction of the 8 TB/s the README uses.  The ring bytes read are taken as the slot
bytes of the packets the step enqueued.  One JSON line.
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
    out = ctx.device_alloc(4 * max_by + (sessions << 8) + (1 << 20))
    span = need * tick_ms
    epoch = [0]

    def run(tap: bool, timing: int):
        bts = [bench.later_batch(ctx, b, epoch[0] * span) if epoch[0] else b for b in base]
        epoch[0] += 1
        ctx.set_timing(timing)
        drained = []
        for i in range(warm):
            bench.run_step(ctx, bts[i])
            if tap:
                ctx.tap_drain(out=out)
        ctx.sync()
        ctx.kernel_times(5)
        t0 = time.perf_counter()
        for i in range(warm, need):
            bench.run_step(ctx, bts[i])
            if tap:
                n, units, streams = ctx.tap_drain(out=out)
                drained.append((n, len(units), int(streams["bytes"].sum())))
        ctx.sync()
        dt = (time.perf_counter() - t0) / steps
        if ctx.stats().status != 0:
            raise SystemExit(f"engine status {ctx.stats().status}")
        return dt, drained

    run(False, ctx.TIMING_FANOUT)                   # first pass: rings and tables settle
    off, _ = run(False, ctx.TIMING_FANOUT)
    for s in sess:
        ctx.tap_enable(s, 0)
    on, _ = run(True, ctx.TIMING_FANOUT)
    _, drained = run(True, ctx.TIMING_ALL)
    k = ctx.kernel_times(5)
    st = ctx.tap_drain(flush=True, out=out)[2]
    counters = {c: int(st[c].sum()) for c in ("packets", "skipped", "malformed", "orphans", "unsupported", "missed", "units", "damaged_units")}
    out.free()
    ctx.close()
    read = float(np.mean([b["bytes"] for b in base[warm:]]))
    written = float(np.mean([d[2] for d in drained])) if drained else 0.0
    kmean = float(np.mean(k)) if k else None
    return {"tick_ms": tick_ms, "packets_per_step": int(np.mean([b["n"] for b in base])),
            "step_ms_off": round(1e3 * off, 4), "step_ms_on": round(1e3 * on, 4),
            "drain_us": [round(1e3 * v, 2) for v in k], "drain_us_mean": round(1e3 * kmean, 2) if k else None,
            "drain_us_min": round(1e3 * float(np.min(k)), 2) if k else None,
            "ring_bytes_read_per_step": int(read), "annexb_bytes_per_step": int(written),
            "units_per_step": int(np.mean([d[1] for d in drained])) if drained else 0,
            "fraction_of_peak": round((read + written) / (kmean * 1e-3) / PEAK, 4) if k else None,
            "counters": counters}


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
    print(json.dumps({"bench": "tap", "sessions": args.sessions, "subs": args.subs, "results": res}))


if __name__ == "__main__":
    main()
