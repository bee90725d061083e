"""CPU: the rules of the FLV mux (include/edgpu.h, edgpu_flv_mux) on tests/flv_model.py: one tag
spelled out byte by byte, a hand-written vector for every rule, and the round trip through the
independent reader tests/flv_demux.py."""
import pytest

import flv_demux
import flv_model as fm
import tap_traces as tt
from flv_model import DAMAGED, KEY, PARAMS
from tap_model import depacketise

SC = b"\x00\x00\x00\x01"


def unit(n, k=0, nal=0x41):
    return (SC + bytes([nal]) + bytes(((k * 31 + 7 * j) % 255) + 1 for j in range(max(n - 5, 0))))[:n]


def row(**kw):
    r = fm.zero_row()
    r.update(kw)
    return r


def test_one_tag_byte_by_byte():
    out, rows, st = fm.mux_stream(fm.Config(time_offset=90 * 0x01020304), [(bytes.fromhex("0000000165AABB"), 777, KEY)])
    want = ("09" "00000C" "020304" "01" "000000"           # video, DataSize 7 + 5, timestamp 0x01020304, stream id
            "17" "01" "000000"                              # key frame + AVC, NALU, composition time
            "00000003" "65AABB"                             # the NAL's length where the start code was
            "00000017")                                     # PreviousTagSize 7 + 16
    assert out.hex().upper() == want and len(out) == 7 + 20
    assert rows == [row(offset=0, bytes=27, timestamp_ms=0x01020304, flags=KEY)]
    assert st == dict(ext_ts=777, origin=777, started=1)
    out, rows, _ = fm.mux_stream(None, [(bytes.fromhex("0000000141"), 5, 0)])
    assert out.hex().upper() == "09" "00000A" "000000" "00" "000000" "27" "01" "000000" "00000001" "41" "00000015"


def test_timestamp_extension_byte():
    # ext - origin = 90 * 2^24: the 24 low bits are 0 and the extension byte is 1
    st = dict(ext_ts=1000, origin=1000, started=1)
    big = 90 << 24
    out, rows, st = fm.mux_stream(None, [(b"", (1000 + (1 << 31) - 1) & 0xFFFFFFFF, 0), (unit(9), (1000 + big) & 0xFFFFFFFF, 0)], st)
    assert st["ext_ts"] == 1000 + big
    assert rows[1]["timestamp_ms"] == 1 << 24 and out[4:8] == bytes([0, 0, 0, 1])
    (t,) = flv_demux.tags(out)
    assert t["timestamp"] == 1 << 24
    # floor division, and the stamp mod 2^32
    out, rows, _ = fm.mux_stream(fm.Config(time_offset=89), [(unit(9), 0, 0), (unit(9), 1, 0), (unit(9), 91, 0)])
    assert [r["timestamp_ms"] for r in rows] == [0, 1, 2]
    out, rows, _ = fm.mux_stream(fm.Config(time_offset=90 * ((1 << 32) + 5) + 3), [(unit(9), 12345, 0)])
    assert rows[0]["timestamp_ms"] == 5


def test_timestamp_steps_back():
    out, rows, st = fm.mux_stream(None, [(unit(9), 9000, KEY), (unit(9), 18000, 0), (unit(9), 13500, 0)])
    assert [r["timestamp_ms"] for r in rows] == [0, 100, 50] and st["ext_ts"] == 13500
    # below the origin: t90 wraps mod 2^64 before the division, the stamp is its low 32 bits
    out, rows, st = fm.mux_stream(None, [(unit(9), 9000, 0), (unit(9), 8910, 0)])
    assert rows[1]["timestamp_ms"] == (((1 << 64) - 90) // 90) & 0xFFFFFFFF


def test_zero_byte_unit():
    out, rows, st = fm.mux_stream(None, [(unit(9), 1000, 0), (b"", 10000, KEY | DAMAGED), (unit(10), 19000, 0)])
    assert rows[1] == row(offset=29, bytes=0, timestamp_ms=100, flags=KEY | DAMAGED)
    assert rows[2]["offset"] == 29 and rows[2]["timestamp_ms"] == 200 and len(out) == 29 + 30
    assert len(flv_demux.tags(out)) == 2
    out, rows, st = fm.mux_stream(None, [(b"", 500, PARAMS)])
    assert out == b"" and st == dict(ext_ts=500, origin=500, started=1) and rows[0]["sps_bytes"] == 0


def sample(es, flags=0):
    out, rows, _ = fm.mux_stream(None, [(es, 0, flags)])
    assert len(out) == len(es) + 20 == rows[0]["bytes"]
    return out[16:-4], rows[0]["flags"]


def test_start_code_rules():
    assert sample(bytes([0x41, 2, 3]) + SC + bytes([0x41, 9])) == (bytes([0x41, 2, 3, 0, 0, 0, 2, 0x41, 9]), DAMAGED)
    assert sample(SC + bytes([0x41]) + b"\x00" + SC + bytes([0x42])) == (bytes([0, 0, 0, 2, 0x41, 0, 0, 0, 0, 1, 0x42]), 0)  # 00 00 00 00 01
    assert sample(SC + bytes([0x41, 0, 0, 1, 7])) == (bytes([0, 0, 0, 5, 0x41, 0, 0, 1, 7]), 0)       # 00 00 01 is data
    assert sample(bytes([0, 0, 1, 0x41])) == (bytes([0, 0, 1, 0x41]), DAMAGED)
    assert sample(SC + bytes([0x41, 0, 0, 0])) == (bytes([0, 0, 0, 4, 0x41, 0, 0, 0]), 0)             # cut by the unit's end
    out, rows, _ = fm.mux_stream(None, [(SC + bytes([0x41, 0, 0, 0]), 0, 0), (bytes([1, 0x41]), 1, 0)])
    assert out[16:24] == bytes([0, 0, 0, 4, 0x41, 0, 0, 0]) and out[28 + 16:28 + 18] == bytes([1, 0x41])
    assert rows[1]["flags"] == DAMAGED
    assert sample(SC + SC + bytes([0x41])) == (bytes([0, 0, 0, 0, 0, 0, 0, 1, 0x41]), 0)              # a NAL of length 0


def params_unit(at, extra=()):
    """NAL number `at` (from 1) is an SPS of 6 bytes, the one after it a PPS of 3; slices around them."""
    nals = [bytes([0x41, k + 1]) for k in range(at - 1)] + [bytes([0x67, 1, 2, 3, 4, 5]), bytes([0x68, 9, 8])] + list(extra)
    return b"".join(SC + n for n in nals), 16 + 6 * (at - 1) + 4


def test_parameter_sets():
    es, off = params_unit(1)
    _, rows, _ = fm.mux_stream(None, [(es, 0, KEY | PARAMS)])
    assert (rows[0]["sps_offset"], rows[0]["sps_bytes"], rows[0]["pps_offset"], rows[0]["pps_bytes"]) == (20, 6, 30, 3)
    _, rows, _ = fm.mux_stream(None, [(es, 0, KEY)])                    # without PARAMS nothing is looked for
    assert rows[0]["sps_bytes"] == rows[0]["pps_bytes"] == 0
    es, off = params_unit(7)                                            # SPS at NAL 7, PPS at NAL 8
    _, rows, _ = fm.mux_stream(None, [(es, 0, PARAMS)])
    assert (rows[0]["sps_offset"], rows[0]["sps_bytes"], rows[0]["pps_offset"], rows[0]["pps_bytes"]) == (off, 6, off + 10, 3)
    es, off = params_unit(8)                                            # SPS at NAL 8, PPS at NAL 9: beyond the eighth
    _, rows, _ = fm.mux_stream(None, [(es, 0, PARAMS)])
    assert (rows[0]["sps_offset"], rows[0]["sps_bytes"], rows[0]["pps_offset"], rows[0]["pps_bytes"]) == (off, 6, 0, 0)
    es, off = params_unit(9)
    _, rows, _ = fm.mux_stream(None, [(es, 0, PARAMS)])
    assert (rows[0]["sps_offset"], rows[0]["sps_bytes"], rows[0]["pps_offset"], rows[0]["pps_bytes"]) == (0, 0, 0, 0)
    # the first of each wins; a second SPS is not reported
    es = SC + bytes([0x67, 1]) + SC + bytes([0x67, 2, 2]) + SC + bytes([0x68, 3]) + SC + bytes([0x68])
    _, rows, _ = fm.mux_stream(None, [(es, 0, PARAMS)])
    assert (rows[0]["sps_offset"], rows[0]["sps_bytes"], rows[0]["pps_offset"], rows[0]["pps_bytes"]) == (20, 2, 33, 2)
    # a zero-length NAL counts among the eight and is never reported; the byte after it belongs to the next start code
    es = SC + SC + bytes([0x67, 7, 7])
    _, rows, _ = fm.mux_stream(None, [(es, 0, PARAMS)])
    assert (rows[0]["sps_offset"], rows[0]["sps_bytes"]) == (24, 3)
    es = b"".join([SC] * 8) + bytes([0x67, 7, 7])                       # seven empty NALs, the SPS is the eighth
    _, rows, _ = fm.mux_stream(None, [(es, 0, PARAMS)])
    assert (rows[0]["sps_offset"], rows[0]["sps_bytes"]) == (16 + 32, 3)
    es = b"".join([SC] * 9) + bytes([0x67, 7, 7])                       # ... the ninth
    _, rows, _ = fm.mux_stream(None, [(es, 0, PARAMS)])
    assert rows[0]["sps_bytes"] == 0
    # counted from the first start code: bytes before it are no NAL
    es = bytes([0x67, 1, 2]) + SC + bytes([0x68, 5])
    _, rows, _ = fm.mux_stream(None, [(es, 0, PARAMS)])
    assert (rows[0]["sps_bytes"], rows[0]["pps_offset"], rows[0]["pps_bytes"], rows[0]["flags"]) == (0, 23, 2, PARAMS | DAMAGED)
    # a parameter set that ends in a start code cut by the unit's end keeps those bytes
    es = SC + bytes([0x68, 5, 0, 0, 0])
    _, rows, _ = fm.mux_stream(None, [(es, 0, PARAMS)])
    assert (rows[0]["pps_offset"], rows[0]["pps_bytes"]) == (20, 5)


def test_streams_are_aligned_and_uncovered_units_zero():
    units = [dict(offset=0, bytes=7, rtp_ts=5, flags=KEY), dict(offset=7, bytes=6, rtp_ts=9, flags=0),
             dict(offset=16, bytes=5, rtp_ts=1, flags=0)]
    es = SC + b"\x65\x01\x02" + SC + b"\x41\x03" + bytes(3) + SC + b"\x41"
    streams = [dict(unit_first=0, unit_count=1), dict(unit_first=0, unit_count=0), dict(unit_first=2, unit_count=1)]
    states = [fm.new_state() for _ in streams]
    out, rows, total = fm.mux(None, es, units, streams, states, fill=0xEE)
    assert [r["offset"] for r in rows] == [0, 0, 32] and total == 32 + 25 and out[27:32] == b"\xEE" * 5
    assert rows[1] == fm.zero_row() and rows[2]["stream"] == 2
    assert states[1] == fm.new_state()


def test_size_limits():
    assert not fm.bad_argument([dict(bytes=fm.MAX_UNIT)], [dict(unit_first=0, unit_count=1)])
    assert fm.bad_argument([dict(bytes=fm.MAX_UNIT + 1)], [])
    n = 256
    units = [dict(bytes=fm.MAX_UNIT)] * n
    assert (fm.MAX_UNIT + 20) * (n - 1) < 1 << 32 <= (fm.MAX_UNIT + 20) * n
    assert fm.bad_argument(units, [dict(unit_first=0, unit_count=n)])
    assert not fm.bad_argument(units, [dict(unit_first=0, unit_count=n - 1), dict(unit_first=n - 1, unit_count=1)])


@pytest.mark.parametrize("mtu", [100, 1400])
def test_round_trip_every_nal_length(mtu):
    """packetiser -> tap model -> FLV model -> demuxer gives back every NAL, for every length 1..3000."""
    types = [1, 5, 7, 8, 6, 23]
    aus = [[tt.nal(types[n % len(types)], n)] for n in range(1, 3001)]
    pk, _ = tt.packetise(aus, mtu=mtu, seq0=65000)
    es, units, _ = depacketise(pk, flush=False)
    assert len(units) == len(aus)
    out, rows, total = fm.mux(None, es, units, [dict(unit_first=0, unit_count=len(units))], [fm.new_state()])
    got = flv_demux.tags(out)
    assert [t["nals"] for t in got] == aus
    assert [(t["offset"], t["bytes"]) for t in got] == [(r["offset"], r["bytes"]) for r in rows]
    assert [t["timestamp"] for t in got] == [(3000 * k) // 90 for k in range(len(aus))]
    for n, t, r in zip(range(1, 3001), got, rows):
        typ = types[n % len(types)]
        assert t["key"] == (typ == 5)
        assert (r["sps_offset"], r["sps_bytes"]) == ((20, n) if typ == 7 else (0, 0))
        assert (r["pps_offset"], r["pps_bytes"]) == ((20, n) if typ == 8 else (0, 0))


def test_round_trip_multi_nal_units():
    aus = [[tt.nal(7, 24), tt.nal(8, 8), tt.nal(5, 3001)], [tt.nal(1, 50)], [tt.nal(6, 9), tt.nal(1, 1), tt.nal(1, 1500)]]
    pk, _ = tt.packetise(aus, mtu=1400, stap=True)
    es, units, _ = depacketise(pk, flush=False)
    out, rows, _ = fm.mux(None, es, units, [dict(unit_first=0, unit_count=3)], [fm.new_state()])
    got = flv_demux.tags(out)
    assert [t["nals"] for t in got] == aus and [t["key"] for t in got] == [True, False, False]
    r = rows[0]
    assert out[r["sps_offset"]:r["sps_offset"] + r["sps_bytes"]] == aus[0][0]
    assert out[r["pps_offset"]:r["pps_offset"] + r["pps_bytes"]] == aus[0][1]


def test_split_calls_against_one_call():
    units = [(unit(20 + j % 90, j), 3000 * j - (4000 if j % 23 == 5 else 0), KEY if j % 30 == 0 else 0) if j % 17 != 3
             else (b"", 3000 * j, 0) for j in range(1, 120)]
    one, one_rows, one_st = fm.mux_stream(fm.Config(time_offset=77), units)
    for cut in range(len(units) + 1):                       # split at every unit boundary, the state carried
        a, rows_a, st = fm.mux_stream(fm.Config(time_offset=77), units[:cut])
        b, rows_b, st = fm.mux_stream(fm.Config(time_offset=77), units[cut:], st)
        assert a + b == one and st == one_st
        for r in rows_b:
            r["offset"] += len(a)
        assert rows_a + rows_b == one_rows


def test_demux_rejects_broken_tags():
    out, _, _ = fm.mux_stream(None, [(unit(30), 0, KEY), (unit(31), 3000, 0)])
    flv_demux.tags(out)
    for pos, val in ((0, 8), (3, out[3] + 1), (10, 1), (11, 0x37), (11, 0x12), (12, 2), (15, 1), (19, out[19] + 1), (49, out[49] ^ 1)):
        bad = bytearray(out)
        bad[pos] = val
        with pytest.raises(flv_demux.DemuxError):
            flv_demux.tags(bytes(bad))
