#!/usr/bin/env python3
"""Records H.264 elementary streams from the engine's taps (edgpu_tap_*).

Replays a trace file (--trace, the pushes of an .edtr trace) or a small synthetic push (--sessions
sessions of one H.264 track plus audio, --seconds long), taps every H.264 track, drains every
tick and writes <session>_<track>_<n>.h264 (Annex-B) under --out with index.json, the units of
every file.  A file starts at the first KEY unit and a new file is cut at the first KEY unit
--segment seconds after the file began: the reference recorder's rule (its segment is 300 s).

--mp4 records fragmented MP4 instead (Context.tap_drain_mp4, easydarwin_amd/mp4.py): the units are
muxed into moof + mdat fragments on the GPU and <session>_<track>_<n>.mp4 holds the initialisation
segment and then the fragments, cut by the same rule.  A stream whose SPS does not parse (the
synthetic push and the test traces carry random bytes in their parameter sets) gets the
initialisation segment of a stand-in 640x480 Baseline SPS, so that its file still opens; the report
counts them in "stand_in_init".

--flv records FLV (Context.tap_drain_flv, easydarwin_amd/flv.py): one video tag per access unit,
muxed on the GPU, in <session>_<track>_<n>.flv behind the file header, onMetaData and the AVC sequence
header, cut by the same rule; the stand-in parameter sets serve its headers in the same way.

--audio also taps every MPEG4-GENERIC track (edgpu_aac_tap_*), with the config taken from its fmtp line,
and records <session>_<track>_<n>.aac (ADTS) through easydarwin_amd/aac.py, listed in audio_index.json.
The audio taps are flushed whenever --segment seconds have passed since the last flush, and at the end,
so that aac.Recorder, which cuts a file only after a flush, cuts by the same period.
The synthetic push then carries an RFC 3640 AAC-hbr track instead of PCMA.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from easydarwin_amd import edgpu  # noqa: E402
from easydarwin_amd.synth import SEED_BASE, TrackSpec, make_sdp, session_packets  # noqa: E402


class Recorder:
    def __init__(self, out_dir, segment_ms):
        self.out_dir, self.segment_ms = out_dir, segment_ms
        self.open = {}              # (session, track) -> [file object, entry, start arrival]
        self.files = []
        self.drained_units = 0

    def take(self, data, units, streams):
        self.drained_units += len(units)
        for st in streams:
            key = (int(st["session"]), int(st["track"]))
            for u in units[int(st["unit_first"]):int(st["unit_first"]) + int(st["unit_count"])]:
                cur = self.open.get(key)
                is_key = bool(int(u["flags"]) & edgpu.TAP_KEY)
                if is_key and (cur is None or int(u["arrival_ms"]) - cur[2] >= self.segment_ms):
                    if cur:
                        cur[0].close()
                    name = "%d_%d_%d.h264" % (key[0], key[1], sum(1 for f in self.files if f["stream"] == list(key)))
                    entry = {"file": name, "stream": list(key), "units": []}
                    self.files.append(entry)
                    cur = self.open[key] = [open(os.path.join(self.out_dir, name), "wb"), entry, int(u["arrival_ms"])]
                if cur is None:
                    continue                                        # nothing before the first key frame
                off, n = int(u["offset"]), int(u["bytes"])
                cur[1]["units"].append({"offset": cur[0].tell(), "bytes": n, "rtp_ts": int(u["rtp_ts"]),
                                        "arrival_ms": int(u["arrival_ms"]), "flags": int(u["flags"])})
                cur[0].write(data[off:off + n].tobytes())

    def close(self):
        for cur in self.open.values():
            cur[0].close()
        with open(os.path.join(self.out_dir, "index.json"), "w") as f:
            json.dump({"files": self.files, "drained_units": self.drained_units}, f)


# 640x480 Baseline, level 3.0, and a PPS: what StandInInit uses where a stream's own SPS does not parse
STAND_IN_SPS = bytes([0x67, 0x42, 0x00, 0x1E, 0xF4, 0x05, 0x01, 0xEC, 0x80])
STAND_IN_PPS = bytes([0x68, 0xCE, 0x3C, 0x80])


class StandInInit:
    """The `init` callable of mp4.Recorder / hls.Fmp4Segmenter: edgpu.mp4_init, with the stand-in
    parameter sets where it refuses the stream's own."""

    def __init__(self):
        self.count = 0

    def __call__(self, sps, pps):
        try:
            return edgpu.mp4_init(sps, pps)
        except edgpu.EdgpuError as e:
            if e.code != edgpu.BAD_ARGUMENT:
                raise
            self.count += 1
            return edgpu.mp4_init(STAND_IN_SPS, STAND_IN_PPS)


class StandInHeader:
    """The `header` callable of flv.Recorder: edgpu.flv_header, with the stand-in parameter sets
    where it refuses the stream's own."""

    def __init__(self):
        self.count = 0

    def __call__(self, sps, pps, timestamp_ms=0, parts=0):
        try:
            return edgpu.flv_header(sps, pps, timestamp_ms, parts)
        except edgpu.EdgpuError as e:
            if e.code != edgpu.BAD_ARGUMENT:
                raise
            self.count += 1
            return edgpu.flv_header(STAND_IN_SPS, STAND_IN_PPS, timestamp_ms, parts)


def synthetic(nsessions, seconds, audio=False):
    tracks = [TrackSpec("video", "H264/90000", 96, bitrate=1_000_000, gop=30, idr_bytes=20_000),
              TrackSpec("audio", "MPEG4-GENERIC/48000/2", 97, extra={"rfc3640": True}) if audio else TrackSpec("audio", "PCMA/8000", 8)]
    sdps = [make_sdp(tracks)] * nsessions
    pushes = [session_packets(tracks, seconds * 1000, SEED_BASE + i) for i in range(nsessions)]
    return sdps, pushes


def from_trace(path):
    from easydarwin_amd import trace
    tr = trace.Trace.from_bytes(open(path, "rb").read())
    pushes = [[] for _ in tr.sdps]
    for ev in tr.events:                    # the pushed packets only: sessions live for the whole trace here
        if ev[0] == trace.PKT:
            _, t, s, ch, data = ev
            pushes[s].append((t, ch, data))
    return list(tr.sdps), pushes


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--trace")
    ap.add_argument("--sessions", type=int, default=2)
    ap.add_argument("--seconds", type=int, default=3)
    ap.add_argument("--tick-ms", type=int, default=100)
    ap.add_argument("--segment", type=float, default=300.0, help="seconds per file")
    ap.add_argument("--out", required=True)
    ap.add_argument("--mp4", action="store_true", help="record fragmented MP4 instead of Annex-B")
    ap.add_argument("--flv", action="store_true", help="record FLV instead of Annex-B")
    ap.add_argument("--audio", action="store_true", help="also record every MPEG4-GENERIC track as ADTS .aac")
    a = ap.parse_args()
    if a.mp4 and a.flv:
        ap.error("--mp4 and --flv exclude each other")
    os.makedirs(a.out, exist_ok=True)
    sdps, pushes = from_trace(a.trace) if a.trace else synthetic(a.sessions, a.seconds, a.audio)
    arec = None
    if a.audio:
        from easydarwin_amd import aac
        arec = aac.Recorder(a.out, a.segment)
    if a.mp4:
        from easydarwin_amd import mp4
        init = StandInInit()
        rec = mp4.Recorder(a.out, a.segment, init)
    elif a.flv:
        from easydarwin_amd import flv
        init = StandInHeader()
        rec = flv.Recorder(a.out, a.segment, init)
    else:
        rec = Recorder(a.out, int(a.segment * 1000))
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
                if arec is None:
                    continue
                try:
                    ctx.aac_tap_enable(s, t, edgpu.aac_config_parse(sdp, t))
                except edgpu.EdgpuError as e:
                    if e.code != edgpu.BAD_ARGUMENT:
                        raise                                       # (no MPEG4-GENERIC track the tap supports)
        merged = sorted(((t, i, ch, d) for i, pk in enumerate(pushes) for t, ch, d in pk), key=lambda x: x[0])
        end = merged[-1][0] + 1 if merged else 0
        k = 0
        flushed_at = 0
        for tick in range(0, end + a.tick_ms, a.tick_ms):
            batch = []
            while k < len(merged) and merged[k][0] < tick + a.tick_ms:
                t, i, ch, d = merged[k]
                batch.append((sess[i], ch, t, d))
                k += 1
            if batch:
                ctx.ingest_host(*edgpu.build_batch(batch))
                ctx.keyframe_index()
            if a.mp4:
                data, samples, frags, rows, streams = ctx.tap_drain_mp4(flush=tick + a.tick_ms > end)
                units += len(rows)
                rec.push(data, samples, frags, streams)
            elif a.flv:
                data, tags, rows, streams = ctx.tap_drain_flv(flush=tick + a.tick_ms > end)
                units += len(rows)
                rec.push(data, tags, streams)
            else:
                rec.take(*ctx.tap_drain(flush=tick + a.tick_ms > end))
            if arec is not None:
                last = tick + a.tick_ms > end or tick + a.tick_ms - flushed_at >= int(a.segment * 1000)
                if last:
                    flushed_at = tick + a.tick_ms
                arec.push(*ctx.aac_tap_drain(flush=last), flushed=last)
    rec.close()
    audio = {}
    if arec is not None:
        arec.close()
        audio = {"audio_files": len(arec.files), "audio_frames": arec.frames}
    if a.mp4 or a.flv:
        print(json.dumps({"files": sum(len(v["files"]) for v in rec.summary().values()), "units": units,
                          "streams": rec.summary(), "stand_in_init": init.count, **audio}))
    else:
        print(json.dumps({"files": len(rec.files), "units": rec.drained_units, **audio}))


if __name__ == "__main__":
    main()
