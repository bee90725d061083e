#!/usr/bin/env python3
"""HLS from the engine's taps: H.264 tracks -> MPEG-2 transport stream on the GPU -> .ts segments and
.m3u8 playlists (edgpu_tap_*, edgpu_ts_mux, easydarwin_amd/hls.py).

Replays a trace file (--trace) or a small synthetic push (--sessions, --seconds) as
tools/tap_record.py does, taps every H.264 track, drains and muxes every tick (Context.tap_drain_ts)
and writes <session>_<track>/seg<n>.ts with index.m3u8 under --out.  A segment is cut at the first
KEY unit --segment seconds after it began; --window bounds the playlist (0 keeps every segment).

--fmp4 writes fragmented-MP4 segments instead (Context.tap_drain_mp4, hls.Fmp4Segmenter):
<session>_<track>/init.mp4, seg<n>.m4s and a version-7 playlist with #EXT-X-MAP.  Streams whose SPS
does not parse get a stand-in initialisation segment, as in tools/tap_record.py --mp4.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from easydarwin_amd import edgpu, hls  # noqa: E402
from tap_record import StandInInit, from_trace, synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--trace")
    ap.add_argument("--sessions", type=int, default=2)
    ap.add_argument("--seconds", type=int, default=3)
    ap.add_argument("--tick-ms", type=int, default=100)
    ap.add_argument("--segment", type=float, default=2.0, help="seconds per segment")
    ap.add_argument("--window", type=int, default=0, help="segments the playlist lists (0: all)")
    ap.add_argument("--out", required=True)
    ap.add_argument("--fmp4", action="store_true", help="fragmented-MP4 segments instead of transport-stream ones")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    sdps, pushes = from_trace(a.trace) if a.trace else synthetic(a.sessions, a.seconds)
    init = StandInInit()
    seg = hls.Fmp4Segmenter(a.out, a.segment, a.window, init) if a.fmp4 else hls.Segmenter(a.out, a.segment, a.window)
    units = 0
    with edgpu.Context(max_batch_packets=1 << 15, max_batch_bytes=32 << 20, out_arena_bytes=32 << 20,
                       max_out_packets=1 << 16) as ctx:
        sess = []
        for sdp in sdps:
            s = ctx.session_add(sdp)
            sess.append(s)
            for t in range(ctx.session_tracks(s)):
                try:
                    ctx.tap_enable(s, t)
                except edgpu.EdgpuError as e:
                    if e.code != edgpu.BAD_ARGUMENT:
                        raise                                       # (not an H.264 track)
        merged = sorted(((t, i, ch, d) for i, pk in enumerate(pushes) for t, ch, d in pk), key=lambda x: x[0])
        end = merged[-1][0] + 1 if merged else 0
        k = 0
        for tick in range(0, end + a.tick_ms, a.tick_ms):
            batch = []
            while k < len(merged) and merged[k][0] < tick + a.tick_ms:
                t, i, ch, d = merged[k]
                batch.append((sess[i], ch, t, d))
                k += 1
            if batch:
                ctx.ingest_host(*edgpu.build_batch(batch))
                ctx.keyframe_index()
            if a.fmp4:
                data, samples, frags, rows, streams = ctx.tap_drain_mp4(flush=tick + a.tick_ms > end)
                units += len(rows)
                seg.push(data, samples, frags, streams)
                continue
            data, rows, streams = ctx.tap_drain_ts(flush=tick + a.tick_ms > end)
            units += len(rows)
            seg.push(data, rows, streams)
    seg.close()
    report = {"units": units, "streams": seg.summary()}
    if a.fmp4:
        report["stand_in_init"] = init.count
    print(json.dumps(report))


if __name__ == "__main__":
    main()
