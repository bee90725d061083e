#!/usr/bin/env python3
"""Cost of the AAC audio tap on the audio half of the C5 workload (tools/bench_c5.py: mixed video with
AAC / PCMA / PCMU audio, one session in three AAC): every MPEG4-GENERIC track is tapped and drained
into a device buffer once per step, per tick length.

  python tools/bench_aac.py [--sessions 1024] [--ticks 1000,100,20] [--steps 10]

The AAC tracks carry RFC 3640 AAC-hbr packets (synth.py's opt-in rfc3640 flag: one 200..400-byte AU
per packet, 46.9 packets/s); only the audio tracks are pushed, since a drain reads nothing else.
Reports the drain's device time by event pairs (edgpu_kernel_times(9): scan + place + copy), the
bytes read (the slot bytes of the tapped packets a step enqueued) and written (ADTS bytes), and
(read + written) / drain time as a fraction of the 8 TB/s the README uses.  One JSON line.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from easydarwin_amd import edgpu  # noqa: E402
from easydarwin_amd.synth import SEED_BASE, TrackSpec, make_sdp, session_packets  # noqa: E402

PEAK = 8e12
AUDIO = [("MPEG4-GENERIC/48000/2", 98), ("PCMA/8000", 8), ("PCMU/8000", 0)]


def tracks_of(g: int):
    a = AUDIO[(g // 3) % 3]
    return [TrackSpec("video", "H264/90000", 96),
            TrackSpec("audio", a[0], a[1], extra={"rfc3640": True} if a[1] == 98 else {})]


def measure(tick_ms: int, sessions: int, steps: int, warm: int) -> dict:
    need = warm + steps
    per_step = [[] for _ in range(need)]
    sdps = []
    for g in range(sessions):
        tr = tracks_of(g)
        sdps.append(make_sdp(tr))
        for t, ch, data in session_packets(tr[1:], need * tick_ms, SEED_BASE + 5000 + g, t0=(g * 7) % 33):
            per_step[min(int(t) // tick_ms, need - 1)].append((g, 2 + ch, int(t), data))     # track 1's channels
    batches = [edgpu.build_batch(pk) for pk in per_step]
    with edgpu.Context(device=0, other_ring_packets=2048, other_ring_bytes=1 << 20,
                       max_batch_packets=max(len(b[0]) for b in batches) + 1, max_batch_bytes=32 << 20) as ctx:
        tapped = []
        for g in range(sessions):
            s = ctx.session_add(sdps[g])
            try:
                ctx.aac_tap_enable(s, 1, edgpu.aac_config_parse(sdps[g], 1))
                tapped.append(g)
            except edgpu.EdgpuError as e:
                if e.code != edgpu.BAD_ARGUMENT:
                    raise                                               # (PCMA / PCMU)
        out = ctx.device_alloc(max(b[3].nbytes for b in batches) * 2 + (sessions << 8) + (1 << 20))
        read, written, frames = [], [], []
        for i, b in enumerate(batches):
            ctx.ingest_host(*b)
            ctx.keyframe_index()
            if i == warm:
                ctx.sync()
                ctx.kernel_times(9)
            n, rows, streams = ctx.aac_tap_drain(out=out)
            if i >= warm:
                written.append(int(streams["bytes"].sum()))
                frames.append(len(rows))
                read.append(sum((4 + len(p[3]) + 15) // 16 * 16 for p in per_step[i] if p[1] == 2 and p[0] in set(tapped)))
        k = ctx.kernel_times(9)
        st = ctx.aac_tap_drain(flush=True, out=out)[2]
        counters = {c: int(st[c].sum()) for c in ("packets", "skipped", "malformed", "orphans", "unsupported", "missed",
                                                  "frames", "discontinuities")}
        out.free()
    kmean = float(np.mean(k)) if k else None
    rd, wr = float(np.mean(read)), float(np.mean(written))
    return {"tick_ms": tick_ms, "taps": len(tapped), "frames_per_step": int(np.mean(frames)),
            "drain_us": [round(1e3 * v, 2) for v in k], "drain_us_mean": round(1e3 * kmean, 2) if k else None,
            "drain_us_min": round(1e3 * float(np.min(k)), 2) if k else None,
            "ring_bytes_read_per_step": int(rd), "adts_bytes_per_step": int(wr),
            "fraction_of_peak": round((rd + wr) / (kmean * 1e-3) / PEAK, 6) if k else None, "counters": counters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=1024)
    ap.add_argument("--ticks", default="1000,100,20")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    edgpu.load()
    res = [measure(int(t), args.sessions, args.steps, args.warmup) for t in args.ticks.split(",")]
    print(json.dumps({"bench": "aac", "sessions": args.sessions, "results": res}))


if __name__ == "__main__":
    main()
