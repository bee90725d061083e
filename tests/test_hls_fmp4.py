"""CPU: hls.Fmp4Segmenter and mp4.Recorder on the model's fragments (tests/mp4_model.py): playlist
text, EXT-X-MAP, the cutting rules, and every written file through tests/mp4_demux.py."""
import os

import mp4_demux
import mp4_model as mm
from easydarwin_amd import hls, mp4
from mp4_model import DAMAGED, KEY
from test_mp4_init import PPS, sps

SC = b"\x00\x00\x00\x01"
SPS = sps(66, 30, 40, 30)
FPS_STEP = 3000                 # 30 fps at 90 kHz


def drains(n_units=300, gop=30, per_drain=37, damaged=(), no_params_before=0):
    """The model's output for one stream in drains of `per_drain` units: [(bytes, samples, frags, streams)]."""
    units = []
    for j in range(n_units):
        if j % gop == 0:
            head = (SC + SPS + SC + PPS) if j >= no_params_before else b""
            units.append((head + SC + bytes([0x65, 1 + j % 200, 7]), FPS_STEP * j, KEY | (DAMAGED if j in damaged else 0)))
        else:
            units.append((SC + bytes([0x41, 1 + j % 200]), FPS_STEP * j, DAMAGED if j in damaged else 0))
    out, state = [], mm.new_state()
    for a in range(0, n_units, per_drain):
        es, rows = bytearray(), []
        for b, ts, fl in units[a:a + per_drain]:
            rows.append(dict(offset=len(es), bytes=len(b), rtp_ts=ts, flags=fl))
            es += b
        streams = [dict(session=3, track=1, unit_first=0, unit_count=len(rows))]
        data, samples, frags, _ = mm.mux(None, bytes(es), rows, streams, [state])
        out.append((data, samples, frags, streams))
    return units, out


def annexb_of(path, skip_init):
    data = open(path, "rb").read()
    if skip_init:
        top = mp4_demux.boxes(data)
        assert [t for t, _, _ in top[:2]] == [b"ftyp", b"moov"]
        init = mp4_demux.init_segment(data[:top[1][2]])
        assert init["sps"] == SPS and init["pps"] == PPS and (init["width"], init["height"]) == (640, 480)
        data = data[top[1][2]:]
    frags = mp4_demux.fragments(data)
    return frags, b"".join(s[3] for d in frags for s in d["samples"])


def test_fmp4_segmenter(tmp_path):
    units, parts = drains(damaged={95})
    seg = hls.Fmp4Segmenter(str(tmp_path), segment=2.0)
    for p in parts:
        seg.push(*p)
    seg.close()
    d = tmp_path / "3_1"
    init = mp4_demux.init_segment(open(d / "init.mp4", "rb").read())
    assert init["sps"] == SPS and init["pps"] == PPS and init["timescale"] == 90000
    lines = open(d / "index.m3u8").read().split("\n")
    # GOPs of 1 s, segments of 2 s: cuts at units 60, 120, ...; 300 units = 5 segments
    assert lines[:5] == ["#EXTM3U", "#EXT-X-VERSION:7", "#EXT-X-TARGETDURATION:2", "#EXT-X-MEDIA-SEQUENCE:0", '#EXT-X-MAP:URI="init.mp4"']
    assert lines[-2:] == ["#EXT-X-ENDLIST", ""]
    body = lines[5:-2]
    assert body == ["#EXTINF:2.000,", "seg0.m4s", "#EXT-X-DISCONTINUITY", "#EXTINF:2.000,", "seg1.m4s", "#EXTINF:2.000,", "seg2.m4s",
                    "#EXTINF:2.000,", "seg3.m4s", "#EXTINF:2.000,", "seg4.m4s"]
    es, seq = b"", 0
    for n in range(5):
        frags, e = annexb_of(d / ("seg%d.m4s" % n), False)
        assert frags[0]["samples"][0][1] == 0x02000000 and frags[0]["tfdt"] == 2 * 90000 * n
        for f in frags:
            seq += 1
            assert f["sequence"] == seq                     # the sequence runs through the segments
        es += e
    assert es == b"".join(u[0] for u in units)
    assert seg.summary() == {"3_1": dict(segments=5, seconds=10.0)}


def test_fmp4_segmenter_waits_for_parameter_sets_and_keeps_a_window(tmp_path):
    units, parts = drains(n_units=200, no_params_before=31, per_drain=200)
    seg = hls.Fmp4Segmenter(str(tmp_path), segment=1.0, window=2)
    for p in parts:
        seg.push(*p)
    seg.close()
    d = tmp_path / "3_1"
    lines = open(d / "index.m3u8").read().split("\n")
    assert "#EXT-X-MEDIA-SEQUENCE:3" in lines and [l for l in lines if l.endswith(".m4s")] == ["seg3.m4s", "seg4.m4s"]
    # the last segment ends with the stream: 20 units whose durations sum to 20 steps
    assert lines[lines.index("seg4.m4s") - 1] == "#EXTINF:%.3f," % (20 * FPS_STEP / 90000)
    _, es = annexb_of(d / "seg0.m4s", False)
    assert es.startswith(units[60][0])                      # units 0..59 had no SPS / PPS in their key units


def test_recorder_cuts_on_key_fragments(tmp_path):
    units, parts = drains()
    rec = mp4.Recorder(str(tmp_path), seconds=3.5)
    for p in parts:
        rec.push(*p)
    rec.close()
    assert rec.summary()["3_1"]["files"] == ["3_1_0.mp4", "3_1_1.mp4", "3_1_2.mp4"]
    es, firsts = b"", []
    for name in rec.summary()["3_1"]["files"]:
        frags, e = annexb_of(os.path.join(tmp_path, name), True)
        assert frags[0]["samples"][0][1] == 0x02000000
        firsts.append(frags[0]["tfdt"] // FPS_STEP)
        es += e
    assert firsts == [0, 120, 240]                          # the first key fragment at least 3.5 s after the file's first
    assert es == b"".join(u[0] for u in units)


def test_parameter_sets():
    sample, _ = mm.sample_of(SC + bytes([9, 0xF0]) + SC + SPS + SC + PPS + SC + bytes([0x65, 1]))
    assert mp4.parameter_sets(sample) == (SPS, PPS)
    assert mp4.parameter_sets(mm.sample_of(SC + bytes([0x41, 1]))[0]) == (None, None)
