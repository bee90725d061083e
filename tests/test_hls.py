"""CPU: easydarwin_amd/hls.py fed by tests/ts_model.py on a synthetic 3-stream, 12-s sequence -- cuts only
at KEY units, EXTINF values, target duration, media sequence under a window, the discontinuity tag,
the end list -- and every segment file through tests/ts_demux.py."""
import os

import numpy as np

import ts_demux
import ts_model as tm
from easydarwin_amd import edgpu, hls

KEY, DAMAGED = edgpu.TAP_KEY, edgpu.TAP_DAMAGED
FPS = 25
STEP = 90000 // FPS


def stream_units(gop, start_ts, first_key=0, damaged=(), seconds=12):
    """`seconds` of 25-fps units, a KEY unit every `gop` frames from frame `first_key`."""
    out = []
    for f in range(seconds * FPS):
        key = f >= first_key and (f - first_key) % gop == 0
        es = bytes([0, 0, 0, 1, 0x65 if key else 0x41]) + bytes((f + j) & 0xFF for j in range(20 + f % 300))
        out.append((es, (start_ts + f * STEP) & 0xFFFFFFFF, (KEY if key else 0) | (DAMAGED if f in damaged else 0)))
    return out


def drains(per_stream, cfgs, per_drain=40):
    """The sequence as tap_drain_ts would hand it over: `per_drain` units of every stream per call."""
    states = [tm.new_state() for _ in per_stream]
    n = max(len(s) for s in per_stream)
    for lo in range(0, n, per_drain):
        es, units, streams = bytearray(), [], []
        for i, s in enumerate(per_stream):
            part = s[lo:lo + per_drain]
            streams.append(dict(session=i + 1, track=0, unit_first=len(units), unit_count=len(part)))
            for b, ts, fl in part:
                units.append(dict(offset=len(es), bytes=len(b), rtp_ts=ts, flags=fl))
                es += b
        out, rows, _ = tm.mux(cfgs, bytes(es), units, streams, states)
        yield np.frombuffer(out, dtype=np.uint8), rows, streams


def playlist(path):
    return open(os.path.join(path, "index.m3u8")).read().split("\n")


def test_segmenter_on_three_streams(tmp_path):
    per_stream = [
        stream_units(25, 1000),                                    # a KEY every second
        stream_units(40, (1 << 32) - 5 * 90000, first_key=10, damaged=(130,)),   # every 1.6 s; the RTP timestamp wraps; starts mid-GOP
        stream_units(75, 77),                                      # every 3 s: longer than the target
    ]
    seg = hls.Segmenter(str(tmp_path), segment=2.0, window=3)
    for data, rows, streams in drains(per_stream, tm.Config(pts_offset=(1 << 33) - 3 * 90000)):   # the PTS wraps too
        seg.push(data, rows, streams)
        for d in os.listdir(tmp_path):                              # a playlist in progress has no end list
            if os.path.exists(tmp_path / d / "index.m3u8"):
                assert "#EXT-X-ENDLIST" not in playlist(tmp_path / d)
    seg.close()
    assert sorted(os.listdir(tmp_path)) == ["1_0", "2_0", "3_0"]

    # stream 1: cuts at 2, 4, .. 10 s: six segments of 2 s
    # stream 2: first KEY at frame 10, then every 40: cuts at the first KEY >= 2 s on: frames 10, 90, 170, 250, then 300 ends it
    # stream 3: KEY every 75 frames: segments of 3 s
    want = {"1_0": [2.0] * 6, "2_0": [3.2, 3.2, 3.2, 2.0], "3_0": [3.0] * 4}
    first_frame = {"1_0": [0, 50, 100, 150, 200, 250], "2_0": [10, 90, 170, 250], "3_0": [0, 75, 150, 225]}
    for i, name in enumerate(("1_0", "2_0", "3_0")):
        lines = playlist(tmp_path / name)
        durs = want[name]
        assert lines[:2] == ["#EXTM3U", "#EXT-X-VERSION:3"]
        assert lines[2] == "#EXT-X-TARGETDURATION:%d" % -(-max(durs) // 1)
        listed = list(range(len(durs)))[-3:]
        assert lines[3] == "#EXT-X-MEDIA-SEQUENCE:%d" % listed[0]
        body = lines[4:]
        expect = []
        for n in listed:
            if name == "2_0" and n == 1:                            # frame 130 is in segment 1 (frames 90..169)
                expect.append("#EXT-X-DISCONTINUITY")
            expect += ["#EXTINF:%.3f," % durs[n], "seg%d.ts" % n]
        assert body == expect + ["#EXT-X-ENDLIST", ""]
        # every segment (those that left the window too) starts with PAT, PMT and a random-access unit
        units = per_stream[i]
        for n, f0 in enumerate(first_frame[name]):
            d = ts_demux.demux(open(tmp_path / name / ("seg%d.ts" % n), "rb").read())
            f1 = first_frame[name][n + 1] if n + 1 < len(durs) else len(units)
            assert d["pes"][0]["packet"] == 2 and d["pes"][0]["rai"] and d["pat"] >= 1
            assert [e["payload"][6:] for e in d["pes"]] == [u[0] for u in units[f0:f1]]
        assert not os.path.exists(tmp_path / name / ("seg%d.ts" % len(durs)))


def test_window_zero_keeps_every_segment(tmp_path):
    seg = hls.Segmenter(str(tmp_path), segment=1.0, window=0)
    for data, rows, streams in drains([stream_units(25, 5, seconds=4)], None, per_drain=7):
        seg.push(data, rows, streams)
    seg.close()
    lines = playlist(tmp_path / "1_0")
    assert lines[2:4] == ["#EXT-X-TARGETDURATION:1", "#EXT-X-MEDIA-SEQUENCE:0"]
    assert [l for l in lines if l.startswith("seg")] == ["seg%d.ts" % n for n in range(4)]
    assert [l for l in lines if l.startswith("#EXTINF")] == ["#EXTINF:1.000,"] * 4 and lines[-2] == "#EXT-X-ENDLIST"
