"""CPU: the rules of the fragmented-MP4 mux (include/edgpu.h, edgpu_mp4_mux) on tests/mp4_model.py:
the header's worked vector, a hand-written vector for every rule, and the round trip through the
independent reader tests/mp4_demux.py."""
import random
import struct

import mp4_demux
import mp4_model as mm
from mp4_model import DAMAGED, KEY, NONE

SC = b"\x00\x00\x00\x01"


def unit(n, k=0, nal=0x41):
    return (SC + bytes([nal]) + bytes(((k * 31 + 7 * j) % 255) + 1 for j in range(max(n - 5, 0))))[:n]


def test_worked_vector():
    out, rows, frags, st = mm.mux_stream(None, [(bytes.fromhex("0000000165AABB"), 0, KEY)])
    want = ("000000646D6F6F66" "000000106D66686400000000" "00000001" "0000004C74726166" "00000010746668640002000000000001"
            "0000001474666474010000000000000000000000" "000000207472756E00000701000000010000006C" "00000E100000000702000000"
            "0000000F6D6461740000000365AABB")
    assert len(out) == 115 and out.hex().upper() == want
    assert (st["sequence"], st["started"], st["last_step"]) == (1, 1, 0)
    assert rows == [dict(offset=108, dts=0, bytes=7, duration=3600, flags=KEY, fragment=0)]
    assert frags == [dict(offset=0, tfdt=0, duration=3600, bytes=115, sequence=1, unit_first=0, samples=1, flags=KEY, stream=0)]


def test_fragment_starts():
    u = [(unit(10, j), 3000 * j, KEY if j in (2, 5) else 0) for j in range(8)]
    _, rows, frags, st = mm.mux_stream(None, u)
    assert [(f["unit_first"], f["samples"], f["flags"] & KEY) for f in frags] == [(0, 2, 0), (2, 3, 1), (5, 3, 1)]
    assert [f["sequence"] for f in frags] == [1, 2, 3] and st["sequence"] == 3
    _, rows, frags, st = mm.mux_stream(mm.Config(max_samples=2), u, st)
    # first sample; max_samples; key; max_samples; key; max_samples
    assert [(f["unit_first"], f["samples"]) for f in frags] == [(0, 2), (2, 2), (4, 1), (5, 2), (7, 1)]
    assert [f["sequence"] for f in frags] == [4, 5, 6, 7, 8]
    assert [r["fragment"] for r in rows] == [0, 0, 1, 1, 2, 3, 3, 4]


def test_zero_byte_unit():
    out, rows, frags, st = mm.mux_stream(None, [(unit(9), 1000, 0), (b"", 4000, KEY), (unit(9), 7000, 0)])
    assert rows[1] == dict(offset=0, dts=3000, bytes=0, duration=0, flags=KEY, fragment=NONE)
    assert len(frags) == 1 and frags[0]["samples"] == 2 and frags[0]["flags"] == 0
    assert rows[0]["duration"] == 6000 and rows[2]["dts"] == 6000
    # a zero-byte unit alone still starts the stream
    _, rows, frags, st = mm.mux_stream(None, [(b"", 500, 0)])
    assert frags == [] and (st["started"], st["origin"], st["ext_ts"], st["sequence"]) == (1, 500, 500, 0)


def test_backward_timestamp_and_clamps():
    step = (1 << 31) - 1
    u = [(unit(8), 5000, 0), (unit(8), 2000, 0), (b"", 2000 + step, 0), (b"", 2000 + 2 * step, 0), (b"", 2000 + 3 * step, 0),
         (unit(8), 2000 + 3 * step + 10, 0), (unit(8), 2000 + 3 * step + 20, 0)]
    _, rows, frags, st = mm.mux_stream(None, u)
    assert rows[0]["duration"] == 0                         # a step back
    assert rows[1]["dts"] == (-3000) & mm.M64               # dts follows ext, mod 2^64
    assert rows[1]["duration"] == 0xFFFFFFFF                # 3 (2^31 - 1) + 10, clamped
    assert rows[5]["duration"] == 10 and rows[6]["duration"] == 10 and st["last_step"] == 10
    assert frags[0]["duration"] == 0xFFFFFFFF + 20


def test_last_step_carried_and_defaulted():
    _, rows, _, st = mm.mux_stream(mm.Config(default_duration=1234), [(unit(8), 0, 0)])
    assert rows[0]["duration"] == 1234 and st["last_step"] == 0
    _, rows, _, st = mm.mux_stream(None, [(unit(8), 100, 0), (unit(8), 400, 0), (unit(8), 400, 0)], st)
    assert [r["duration"] for r in rows] == [300, 0, 300] and st["last_step"] == 300
    _, rows, _, st = mm.mux_stream(mm.Config(default_duration=1234), [(unit(8), 900, 0)], st)
    assert rows[0]["duration"] == 300 and rows[0]["dts"] == 900     # carried; tfdt from ext, not from summed durations


def test_time_offset():
    _, rows, frags, _ = mm.mux_stream(mm.Config(time_offset=(1 << 40) + 7), [(unit(8), 0xFFFFFF00, KEY), (unit(8), 0x100, 0)])
    assert frags[0]["tfdt"] == (1 << 40) + 7 and rows[1]["dts"] == (1 << 40) + 7 + 0x200 and rows[0]["duration"] == 0x200


def sample_payload(es):
    out, rows, frags, _ = mm.mux_stream(None, [(es, 0, 0)])
    return out[rows[0]["offset"]:rows[0]["offset"] + rows[0]["bytes"]], rows[0]["flags"]


def test_start_code_rules():
    assert sample_payload(bytes([0x41, 2, 3]) + SC + bytes([0x41, 9])) == (bytes([0x41, 2, 3, 0, 0, 0, 2, 0x41, 9]), DAMAGED)
    assert sample_payload(SC + bytes([0x41, 0, 0, 1, 7])) == (bytes([0, 0, 0, 5, 0x41, 0, 0, 1, 7]), 0)       # 00 00 01 is data
    assert sample_payload(SC + bytes([0x41]) + b"\x00" + SC + bytes([0x42])) == \
        (bytes([0, 0, 0, 2, 0x41, 0, 0, 0, 0, 1, 0x42]), 0)                                                   # 00 00 00 00 01
    assert sample_payload(SC + SC + bytes([0x41])) == (bytes([0, 0, 0, 0, 0, 0, 0, 1, 0x41]), 0)              # back to back
    assert sample_payload(SC) == (bytes(4), 0)
    assert sample_payload(SC + bytes([0x41, 0, 0, 0])) == (bytes([0, 0, 0, 4, 0x41, 0, 0, 0]), 0)             # cut by the unit's end
    # ... even when the next unit begins with the 01 that would complete it
    out, rows, _, _ = mm.mux_stream(None, [(SC + bytes([0x41, 0, 0, 0]), 0, 0), (bytes([1, 0x41]), 1, 0)])
    assert out[rows[0]["offset"]:][:8] == bytes([0, 0, 0, 4, 0x41, 0, 0, 0]) and out[rows[1]["offset"]:] == bytes([1, 0x41])
    assert rows[1]["flags"] == DAMAGED
    assert sample_payload(bytes([0, 0, 1])) == (bytes([0, 0, 1]), DAMAGED)


def test_streams_are_aligned_and_uncovered_units_zero():
    units = [dict(offset=0, bytes=7, rtp_ts=5, flags=KEY), dict(offset=7, bytes=6, rtp_ts=9, flags=0),
             dict(offset=16, bytes=5, rtp_ts=1, flags=0)]
    es = SC + b"\x65\x01\x02" + SC + b"\x41\x03" + bytes(3) + SC + b"\x41"
    streams = [dict(unit_first=0, unit_count=1), dict(unit_first=0, unit_count=0), dict(unit_first=2, unit_count=1)]
    states = [mm.new_state() for _ in streams]
    out, rows, frags, total = mm.mux(None, es, units, streams, states, fill=0xEE)
    assert [f["offset"] for f in frags] == [0, 128] and total == 128 + 113 and out[115:128] == b"\xEE" * 13
    assert rows[1] == dict(offset=0, dts=0, bytes=0, duration=0, flags=0, fragment=0)
    assert states[1] == mm.new_state()


def test_round_trip_every_length():
    units = [(unit(n, n), 3000 * n, KEY if n % 50 == 0 else 0) for n in range(0, 3001)]
    out, rows, frags, _ = mm.mux_stream(mm.Config(max_samples=64), units)
    got = mp4_demux.fragments(out, prefixed=False)
    assert [(d["offset"], d["bytes"], d["sequence"], d["tfdt"]) for d in got] == \
        [(f["offset"], f["bytes"], f["sequence"], f["tfdt"]) for f in frags]
    samples = [s for d in got for s in d["samples"]]
    with_es = [u for u in units if u[0]]
    assert len(samples) == len(with_es)
    for (dur, fl, raw, _), (es, ts, flags) in zip(samples, with_es):
        if len(es) >= 4:                                    # shorter ones hold no start code: copied as they are
            assert mp4_demux.annexb(raw) == es
        else:
            assert raw == es
        assert fl == (0x02000000 if flags & KEY else 0x01010000)


def test_round_trip_random_nals():
    rng = random.Random(7)
    units = []
    for k in range(200):
        es = b""
        for _ in range(rng.randint(1, 6)):
            body = bytes(rng.choice([0, 0, 1, 2, 3, 0x80, 0xFF]) for _ in range(rng.randint(0, 40)))
            while SC in body or body.endswith(b"\x00"):    # a NAL holds no start code and does not end in 00
                body = body.replace(SC, b"\x00\x00\x03\x01").rstrip(b"\x00")
            es += SC + body
        units.append((es, 3003 * k, KEY if rng.random() < 0.1 else 0))
    out, rows, frags, _ = mm.mux_stream(None, units)
    got = mp4_demux.fragments(out)
    assert b"".join(s[3] for d in got for s in d["samples"]) == b"".join(u[0] for u in units)
    assert all(not r["flags"] & DAMAGED for r in rows)


def test_split_calls_against_one_call():
    units = [(unit(20 + j % 90, j), 3000 * j, KEY if j % 30 == 0 else 0) if j % 17 != 3 else (b"", 3000 * j, 0) for j in range(200)]
    one, _, one_frags, _ = mm.mux_stream(None, units)

    def es_and_keys(data, frags, base=0):
        got = mp4_demux.fragments(data)
        return b"".join(s[3] for d in got for s in d["samples"]), \
            {base + f["unit_first"]: d["tfdt"] for f, d in zip(frags, got) if f["flags"] & KEY}
    one_es, one_keys = es_and_keys(one, one_frags)
    st, split_es, split_keys = None, b"", {}
    for a, b in ((0, 1), (1, 45), (45, 64), (64, 65), (65, 200)):
        data, _, frags, st = mm.mux_stream(None, units[a:b], st)
        e, k = es_and_keys(data, frags, a)
        split_es += e
        split_keys.update(k)
    assert one_es == split_es == b"".join(u[0] for u in units)
    assert one_keys == split_keys and len(one_keys) == 7


def test_demux_rejects_broken_nesting():
    out, _, _, _ = mm.mux_stream(None, [(unit(30), 0, KEY), (unit(31), 3000, 0)])
    mp4_demux.fragments(out)
    for pos, val in ((3, out[3] + 1), (8 + 16 + 3, 0x50), (0x57, out[0x57] + 1)):      # moof size, traf size, data_offset
        bad = bytearray(out)
        bad[pos] = val
        try:
            mp4_demux.fragments(bytes(bad))
        except (mp4_demux.DemuxError, struct.error):
            continue
        raise AssertionError(f"a broken byte at {pos} went unnoticed")
