"""CPU: easydarwin_amd/flv.py (Recorder, LiveStream) fed from tests/flv_model.py: the files parse in
tests/flv_demux.py and hold the original NALs, the sequence header appears once and again exactly
when a parameter set changes, nothing precedes the first key tag, and a viewer's join() plus
tags_since() equals the recorder's file from that key tag on."""
import numpy as np

import flv_demux
import flv_model as fm
from easydarwin_amd import edgpu, flv
from flv_model import KEY, PARAMS
from test_mp4_init import CASES, PPS

SC = b"\x00\x00\x00\x01"
SPS_A, SPS_B = CASES["baseline 640x480"][0], CASES["high 1920x1080"][0]
PPS_B = bytes([0x68, 0xEE, 0x3C, 0x80])


def slice_nal(k, n=30):
    return bytes([0x41]) + bytes(((k * 13 + j) % 250) + 1 for j in range(n))


def idr(k, n=200):
    return bytes([0x65]) + bytes(((k * 7 + j) % 250) + 1 for j in range(n))


def stream_units(gops, first_params=(SPS_A, PPS), change_at=None, gop=5):
    """[(NALs, rtp_ts, flags)]: three slices before the first key unit, then `gops` GOPs; from GOP `change_at` on SPS_B / PPS_B."""
    out, k = [], 0
    for j in range(3):
        out.append(([slice_nal(k)], 3000 * k, 0))
        k += 1
    for g in range(gops):
        sps, pps = first_params if change_at is None or g < change_at else (SPS_B, PPS_B)
        out.append(([sps, pps, idr(k)], 3000 * k, KEY | PARAMS))
        k += 1
        for j in range(gop - 1):
            out.append(([slice_nal(k)], 3000 * k, 0))
            k += 1
    return out


def drains(per_stream, cuts):
    """The model's (bytes, tag rows, stream rows) per drain: every stream's units [a, b) for each cut, states carried."""
    states = [fm.new_state() for _ in per_stream]
    for a, b in zip(cuts, cuts[1:]):
        es, units, streams = bytearray(), [], []
        for s, us in enumerate(per_stream):
            es += bytes(-len(es) % 16)
            streams.append(dict(session=10 + s, track=0, unit_first=len(units), unit_count=len(us[a:b])))
            for nals, ts, fl in us[a:b]:
                raw = b"".join(SC + n for n in nals)
                units.append(dict(offset=len(es), bytes=len(raw), rtp_ts=ts, flags=fl))
                es += raw
        data, rows, _ = fm.mux(None, bytes(es), units, streams, states)
        tags = np.zeros(len(rows), dtype=edgpu.FLV_TAG_DTYPE)
        for i, r in enumerate(rows):
            for f, v in r.items():
                tags[i][f] = v
        yield data, tags, streams


def test_recorder_files_parse_and_hold_the_nals(tmp_path):
    a, b = stream_units(4), stream_units(4, change_at=2)
    rec = flv.Recorder(str(tmp_path))
    for d in drains([a, b], [0, 1, 4, 9, 10, 23]):
        rec.push(*d)
    rec.close()
    summary = rec.summary()
    assert sorted(summary) == ["10_0", "11_0"] and all(len(v["files"]) == 1 for v in summary.values())
    for name, units, changes in (("10_0_0.flv", a, 0), ("11_0_0.flv", b, 1)):
        parsed = flv_demux.file(open(tmp_path / name, "rb").read())
        assert [t["type"] for t in parsed[:3]] == [18, 9, 9] and parsed[1]["packet_type"] == 0
        assert parsed[0]["meta"] == dict(width=640.0, height=480.0, videocodecid=7.0)
        frames = [t for t in parsed[1:] if t["packet_type"] == 1]
        assert [t["nals"] for t in frames] == [u[0] for u in units[3:]]         # nothing from before the first key tag
        assert frames[0]["key"] and frames[0]["timestamp"] == 100 == parsed[1]["timestamp"]
        seqs = [(i, t) for i, t in enumerate(parsed) if t["type"] == 9 and t["packet_type"] == 0]
        assert len(seqs) == 1 + changes
        if changes:                                         # the new sequence header stands right before the tag that changed it
            i, t = seqs[1]
            assert t["config"]["sps"] == SPS_B and t["config"]["pps"] == PPS_B
            assert parsed[i + 1]["nals"][:2] == [SPS_B, PPS_B] and parsed[i + 1]["timestamp"] == t["timestamp"] == (3 + 10) * 3000 // 90
        assert seqs[0][1]["config"]["sps"] == SPS_A and seqs[0][1]["config"]["pps"] == PPS


def test_recorder_needs_parameter_sets_and_cuts_on_key_tags(tmp_path):
    units = [([idr(0)], 0, KEY)] + stream_units(6)          # a key unit without parameter sets comes first: dropped
    units = [(n, 3000 * k, f) for k, (n, _, f) in enumerate(units)]
    rec = flv.Recorder(str(tmp_path), seconds=0.3)          # a GOP is 5 x 33 ms: every second key tag is 0.33 s on
    for d in drains([units], [0, 7, 40]):
        rec.push(*d)
    rec.close()
    files = rec.summary()["10_0"]["files"]
    assert files == ["10_0_0.flv", "10_0_1.flv", "10_0_2.flv"]
    got = []
    for name in files:
        parsed = flv_demux.file(open(tmp_path / name, "rb").read())
        assert [t["type"] for t in parsed[:2]] == [18, 9] and parsed[1]["packet_type"] == 0 and parsed[2]["key"]
        assert sum(1 for t in parsed if t["type"] == 9 and t["packet_type"] == 0) == 1
        got += [t["nals"] for t in parsed[2:]]
    assert got == [u[0] for u in units[4:]]
    assert rec.summary()["10_0"]["tags"] == len(units) - 4


def test_live_stream_join_and_follow(tmp_path):
    a, b = stream_units(4, change_at=2), stream_units(4)
    cuts = [0, 2, 4, 6, 9, 13, 14, 19, 23]
    live = flv.LiveStream((10, 0))
    rec = flv.Recorder(str(tmp_path))
    assert live.join() is None and not live.ready
    viewers = []                                            # [bytes so far, cursor]
    for d in drains([a, b], cuts):
        live.push(*d)
        rec.push(*d)
        for v in viewers:
            more, v[1] = live.tags_since(v[1])
            v[0] += more
        if live.ready:
            data, cursor = live.join()
            parsed = flv_demux.file(data)
            assert [t["type"] for t in parsed[:2]] == [18, 9] and parsed[1]["packet_type"] == 0 and parsed[2]["key"]
            assert sum(1 for t in parsed[2:] if t.get("key") and t["packet_type"] == 1) == 1     # never more than one GOP
            assert len(parsed) - 2 <= 5 and len(live.gop) <= 5 and len(live.buf) < 5 + 5
            viewers.append([data, cursor])
        assert live.tags_since(live.first + len(live.buf)) == (b"", live.first + len(live.buf))
    rec.close()
    whole = flv_demux.file(open(tmp_path / "10_0_0.flv", "rb").read())
    assert len(viewers) == 7
    for data, _ in viewers:
        parsed = flv_demux.file(data)
        # from its key tag on, the viewer has what the recorder's file has: tags, timestamps, sequence headers
        start = next(i for i, t in enumerate(whole) if t["type"] == 9 and t["packet_type"] == 1 and t["timestamp"] == parsed[2]["timestamp"])
        strip = lambda ts: [(t["timestamp"], t["packet_type"], t.get("nals"), t.get("config")) for t in ts]
        assert strip(parsed[2:]) == strip(whole[start:])
        assert parsed[1]["config"]["sps"] == parsed[2]["nals"][0]
    # a cursor that fell out of the GOP resumes at the current key tag behind a sequence header
    data, cursor = live.tags_since(0)
    parsed = flv_demux.tags(data)
    assert parsed[0]["packet_type"] == 0 and parsed[1]["key"] and cursor == live.first + len(live.buf)
    assert [t["nals"] for t in parsed[1:]] == [u[0] for u in a[-5:]]
