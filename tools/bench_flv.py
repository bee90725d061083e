#!/usr/bin/env python3
"""Cost of the FLV mux on the C2 workload (easydarwin_amd/workload.py: 1024 sessions x 16 UDP
subscribers) with every video track tapped: per step one drain into a device buffer, one
fragmented-MP4 mux and one FLV mux of it, each into a device buffer of its own, per tick length.

  python tools/bench_flv.py [--sessions 1024] [--subs 16] [--ticks 1000,100,20] [--steps 10]

Reports, from the same run, the device times by event pairs of the drain (edgpu_kernel_times(5)), the
fragmented-MP4 mux (7: the yardstick) and the FLV mux (8: its five kernels, not timed apart) as
median, minimum and maximum, the step time with the drain alone and with both muxes, and (ES bytes
read twice + bytes written) / mux time as a fraction of the 8 TB/s the README uses.  One JSON line.
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


def spread(ms):
    if not ms:
        return None
    us = 1e3 * np.asarray(ms, dtype=np.float64)
    return {"median": round(float(np.median(us)), 2), "min": round(float(us.min()), 2), "max": round(float(us.max()), 2), "n": len(ms)}


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
    flv = ctx.device_alloc(6 * max_by + (sessions << 12) + (1 << 20))
    mp4 = ctx.device_alloc(6 * max_by + (sessions << 12) + (1 << 20))
    flv_states = np.zeros(sessions, dtype=edgpu.FLV_STATE_DTYPE)
    mp4_states = np.zeros(sessions, dtype=edgpu.MP4_STATE_DTYPE)
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
                samples = np.zeros(len(units), dtype=edgpu.MP4_SAMPLE_DTYPE)
                frags = np.zeros(max(len(units), 1), dtype=edgpu.MP4_FRAG_DTYPE)
                rc, mres = ctx.mp4_mux_raw(None, es.ptr, n, edgpu.PTR_DEVICE, units, streams, mp4_states[:len(streams)],
                                           mp4.ptr, mp4.nbytes, edgpu.PTR_DEVICE, samples, frags)
                if rc:
                    raise SystemExit(f"edgpu_mp4_mux: {rc}")
                tags = np.zeros(len(units), dtype=edgpu.FLV_TAG_DTYPE)
                rc, fres = ctx.flv_mux_raw(None, es.ptr, n, edgpu.PTR_DEVICE, units, streams, flv_states[:len(streams)],
                                           flv.ptr, flv.nbytes, edgpu.PTR_DEVICE, tags)
                if rc:
                    raise SystemExit(f"edgpu_flv_mux: {rc}")
                done.append((int(streams["bytes"].sum()), int(fres.bytes), int(mres.bytes), len(units), int(mres.frags)))

        for i in range(warm):
            step(i)
        ctx.sync()
        for w in (5, 7, 8):
            ctx.kernel_times(w)
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
    k5, k7, k8 = ctx.kernel_times(5), ctx.kernel_times(7), ctx.kernel_times(8)
    es.free()
    flv.free()
    mp4.free()
    ctx.close()
    mean = lambda k: float(np.mean([d[k] for d in done])) if done else 0.0      # noqa: E731
    read, flv_written, mp4_written = mean(0), mean(1), mean(2)
    m7 = float(np.median(k7)) if k7 else None
    m8 = float(np.median(k8)) if k8 else None
    return {"tick_ms": tick_ms, "packets_per_step": int(np.mean([b["n"] for b in base])),
            "step_ms_drain_only": round(1e3 * off, 4), "step_ms_drain_and_both_muxes": round(1e3 * on, 4),
            "drain_us": spread(k5), "mp4_mux_us": spread(k7), "flv_mux_us": spread(k8),
            "es_bytes_per_step": int(read), "flv_bytes_written_per_step": int(flv_written),
            "mp4_bytes_written_per_step": int(mp4_written),
            "units_per_step": int(mean(3)), "fragments_per_step": int(mean(4)),
            "mp4_fraction_of_peak": round((2 * read + mp4_written) / (m7 * 1e-3) / PEAK, 4) if k7 else None,
            "flv_fraction_of_peak": round((2 * read + flv_written) / (m8 * 1e-3) / PEAK, 4) if k8 else None}


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
    print(json.dumps({"bench": "flv", "sessions": args.sessions, "subs": args.subs, "results": res}))


if __name__ == "__main__":
    main()
