"""CPU: tests/aac_model.py against hand-written vectors, one assertion per sentence of the audio tap's
rules in include/edgpu.h, and the round trip packetiser (tests/aac_traces.py) -> model -> ADTS reader
(tests/adts_reader.py), neither of which shares code with the model."""
import struct

import pytest

import aac_traces as at
import adts_reader
from aac_model import ADTS, COUNTERS, DISCONT, FRAGMENTED, HBR, LBR, RAW, AacModel, adts_header, depacketise


def pk(seq, payload, ts=0, marker=True, **kw):
    return at.rtp(seq, ts, marker, payload, **kw)


def hbr(sizes, idx=None):
    """AU-header section by hand: 16 bits per header, AU-size << 3 | index."""
    idx = idx or [0] * len(sizes)
    return struct.pack(">H", 16 * len(sizes)) + b"".join(struct.pack(">H", (s << 3) | i) for s, i in zip(sizes, idx))


def lbr(sizes, idx=None):
    idx = idx or [0] * len(sizes)
    return struct.pack(">H", 8 * len(sizes)) + bytes((s << 2) | i for s, i in zip(sizes, idx))


def counters(**kw):
    return dict(dict.fromkeys(COUNTERS, 0), **kw)


A, B, C = bytes(range(1, 11)), bytes(range(50, 70)), bytes(range(100, 105))


# ---- entries, parse, gap ----

def test_entries_in_queue_order_and_empty_entries_ignored():
    b, f, c = depacketise([pk(1, hbr([10]) + A), b"", pk(2, hbr([20]) + B, ts=1024)], framing=RAW)
    assert b == A + B and [x["first_seq"] for x in f] == [1, 2]
    assert c == counters(packets=2, frames=2)


def test_lost_entries_count_in_missed_and_set_discont():
    m = AacModel(framing=RAW)
    for s in range(4):
        m.push(pk(s, hbr([10]) + A))
    m.lose(3)
    _, f = m.drain()
    assert m.c["missed"] == 3 and len(f) == 1 and f[0]["flags"] == DISCONT and m.c["discontinuities"] == 1


@pytest.mark.parametrize("bad", [bytes(11), b"\x40" + bytes(20), at.rtp(5, 0, True, b"", cc=1)[:14],
                                 at.rtp(5, 0, True, b"")[:12], at.rtp(5, 0, True, bytes(3), pad=0)[:12] + b"",
                                 bytes([0xA0]) + bytes(11) + bytes([0, 0, 0, 0])])
def test_bad_packets_count_in_skipped(bad):
    b, f, c = depacketise([pk(1, hbr([10]) + A), bad, pk(2, hbr([10]) + A)], framing=RAW)
    assert c == counters(packets=3, skipped=1, frames=2) and [x["flags"] for x in f] == [0, 0]


def test_csrcs_extension_and_padding_are_stepped_over():
    b, f, c = depacketise([pk(1, hbr([10]) + A, cc=3, ext=2, pad=5)], framing=RAW)
    assert b == A and c == counters(packets=1, frames=1)


def test_gap_is_previous_good_sequence_plus_one():
    b, f, c = depacketise([pk(65535, hbr([10]) + A), pk(0, hbr([10]) + A), pk(2, hbr([10]) + A), pk(1, hbr([10]) + A)],
                          framing=RAW)
    assert [x["flags"] for x in f] == [0, 0, DISCONT, DISCONT]        # the wrap is no gap; nothing is reordered
    assert c["discontinuities"] == 2


# ---- AU-header section ----

@pytest.mark.parametrize("payload", [b"\x00", b"\x00\x00" + A, struct.pack(">H", 8) + A, struct.pack(">H", 24) + bytes(20),
                                     hbr([10, 10, 10])[:7]])
def test_malformed_sections_drop_the_whole_packet_hbr(payload):
    b, f, c = depacketise([pk(1, payload), pk(2, hbr([10]) + A)], framing=RAW)
    assert c == counters(packets=2, malformed=1, frames=1, discontinuities=1) and b == A and f[0]["flags"] == DISCONT


def test_bit_count_must_be_a_multiple_of_the_header_lbr():
    assert depacketise([pk(1, struct.pack(">H", 12) + bytes(20))], mode=LBR)[2]["malformed"] == 1
    assert depacketise([pk(1, lbr([10]) + A)], mode=LBR, framing=RAW)[0] == A


def test_h_past_the_payload_is_malformed_before_n_is_judged():
    assert depacketise([pk(1, struct.pack(">H", 16 * 17) + bytes(30))])[2] == counters(packets=1, malformed=1)


def test_more_than_max_aus_is_unsupported():
    sizes = [1] * 17
    b, f, c = depacketise([pk(1, hbr(sizes) + bytes(17)), pk(2, hbr([10]) + A)], framing=RAW)
    assert c == counters(packets=2, unsupported=1, frames=1, discontinuities=1) and f[0]["flags"] == DISCONT
    assert depacketise([pk(1, hbr([1] * 16) + bytes(16))], framing=RAW)[2] == counters(packets=1, frames=16)


@pytest.mark.parametrize("idx", [[1, 0], [0, 1], [0, 0, 7]])
def test_au_index_or_delta_means_interleaving(idx):
    sizes = [5] * len(idx)
    b, f, c = depacketise([pk(1, hbr(sizes, idx) + bytes(5 * len(idx))), pk(2, hbr([10]) + A)], framing=RAW)
    assert c == counters(packets=2, unsupported=1, frames=1, discontinuities=1) and b == A
    assert depacketise([pk(1, lbr(sizes, [min(i, 3) for i in idx]) + bytes(5 * len(idx)))], mode=LBR)[2]["unsupported"] == 1


def test_au_size_is_the_top_13_or_6_bits():
    big = bytes(1500)
    assert depacketise([pk(1, hbr([1500]) + big)], framing=RAW)[1][0]["bytes"] == 1500
    assert depacketise([pk(1, lbr([63]) + bytes(63))], mode=LBR, framing=RAW)[1][0]["bytes"] == 63


# ---- whole frames ----

def test_aus_in_order_from_byte_h_with_timestamps_and_rows():
    b, f, c = depacketise([pk(7, hbr([10, 20, 5]) + A + B + C + b"tail", ts=0xFFFFFC00)], framing=RAW, frame_samples=1024)
    assert b == A + B + C                                          # bytes after the last AU are ignored
    assert [(x["offset"], x["bytes"], x["au_index"], x["rtp_ts"]) for x in f] == \
        [(0, 10, 0, 0xFFFFFC00), (10, 20, 1, 0), (30, 5, 2, 0x400)]     # mod 2^32
    assert all(x["first_seq"] == 7 and x["n_packets"] == 1 and x["arrival_ms"] == 0 and x["flags"] == 0 for x in f)


def test_single_au_that_fits_exactly_is_whole():
    b, f, c = depacketise([pk(1, hbr([10]) + A)], framing=RAW)
    assert b == A and f[0]["flags"] == 0


@pytest.mark.parametrize("sizes,body,kept", [([10, 0, 5], A + C, 1), ([10, 30], A + B, 1), ([0, 10], A, 0)])
def test_bad_au_ends_the_packet_and_counts_once(sizes, body, kept):
    b, f, c = depacketise([pk(1, hbr(sizes) + body), pk(2, hbr([5]) + C)], framing=RAW)
    assert c == counters(packets=2, malformed=1, frames=kept + 1, discontinuities=1)
    assert b == A[:10 * kept] + C and f[-1]["flags"] == DISCONT and all(x["flags"] == 0 for x in f[:-1])


# ---- fragments ----

def frags(body, room, seq0=10, ts=5000, size=None):
    size = len(body) if size is None else size
    return [pk(seq0 + k, hbr([size]) + body[o:o + room], ts=ts, marker=o + room >= len(body))
            for k, o in enumerate(range(0, len(body), room))]


BIG = bytes((7 * j) & 0xFF for j in range(100))


def test_fragment_chain_completes_when_bytes_equal_size():
    p = frags(BIG, 30)
    p[-1] = pk(13, hbr([100]) + BIG[90:], ts=5000, marker=False)   # whatever the marker bit says
    b, f, c = depacketise(p, framing=RAW)
    assert b == BIG and c == counters(packets=4, frames=1)
    assert f == [dict(offset=0, bytes=100, rtp_ts=5000, arrival_ms=0, flags=FRAGMENTED, first_seq=10, n_packets=4, au_index=0)]


def test_fragment_in_lbr_is_malformed():
    assert depacketise([pk(1, lbr([40]) + bytes(10))], mode=LBR)[2] == counters(packets=1, malformed=1)


@pytest.mark.parametrize("what", ["gap", "ts", "size"])
def test_chain_broken_opens_a_new_chain_and_orphans(what):
    p = frags(BIG, 30)
    if what == "gap":
        q = p[:2] + frags(BIG, 30, seq0=20)
    elif what == "ts":
        q = p[:2] + frags(BIG, 30, seq0=12, ts=6024)
    else:
        q = p[:2] + frags(BIG + b"x", 30, seq0=12)
    b, f, c = depacketise(q, framing=RAW)
    assert c == counters(packets=6, orphans=2, frames=1, discontinuities=1)
    assert f[0]["flags"] == FRAGMENTED | DISCONT and f[0]["n_packets"] == 4 and b[:100] == BIG


def test_overrun_is_dropped_and_abandons_the_chain():
    p = frags(BIG, 30)[:3] + [pk(13, hbr([100]) + bytes(11), ts=5000), pk(14, hbr([10]) + A, ts=6024)]
    b, f, c = depacketise(p, framing=RAW)
    assert c == counters(packets=5, malformed=1, orphans=3, frames=1, discontinuities=1) and b == A


def test_any_other_good_packet_abandons_the_chain():
    p = frags(BIG, 30)[:2] + [pk(12, hbr([10]) + A, ts=6024)] + [pk(13 + k, x[12:], ts=5000) for k, x in enumerate(frags(BIG, 30)[2:])]
    b, f, c = depacketise(p, framing=RAW)
    # the whole frame abandons two fragments; the late fragments open a chain that never completes
    assert c == counters(packets=5, orphans=4, frames=1, discontinuities=1) and b == A and f[0]["flags"] == DISCONT


def test_a_bad_packet_does_not_abandon_but_its_gap_does():
    p = frags(BIG, 30)
    b, f, c = depacketise(p[:2] + [bytes(5)] + p[2:], framing=RAW)
    assert c == counters(packets=5, skipped=1, frames=1) and b == BIG


def test_whole_units_only_and_flush():
    m = AacModel(framing=RAW)
    p = frags(BIG, 30)
    for k, x in enumerate([pk(9, hbr([10]) + A)] + p[:3]):
        m.push(x, 100 + k)
    b, f = m.drain()
    assert b == A and m.c == counters(packets=1, frames=1) and len(m.queue) == 3      # the fragments wait with their counters
    m.push(p[3], 104)
    b, f = m.drain()
    assert b == BIG and f[0]["arrival_ms"] == 101 and f[0]["flags"] == FRAGMENTED and m.c == counters(packets=5, frames=2)
    for x in frags(BIG, 30, seq0=14, ts=9000)[:2]:
        m.push(x)
    b, f = m.drain(flush=True)
    assert b == b"" and m.c == counters(packets=7, orphans=2, frames=2) and not m.queue and m.pending
    m.push(pk(16, hbr([10]) + A))
    assert m.drain()[1][0]["flags"] == DISCONT


def test_gap_at_a_waiting_chain_is_seen_again_by_the_next_drain():
    m = AacModel(framing=RAW)
    m.push(pk(1, hbr([10]) + A))
    p = frags(BIG, 60, seq0=5)
    m.push(p[0])
    assert m.drain()[0] == A and (m.has_prev, m.prev_seq, m.pending) == (True, 1, False)
    m.push(p[1])
    assert m.drain()[1][0]["flags"] == FRAGMENTED | DISCONT


def test_chain_abandoned_by_a_fragment_that_waits_is_not_forgotten():
    m = AacModel(framing=RAW)
    a, b = frags(BIG, 40, seq0=1, ts=1000), frags(BIG[::-1], 60, seq0=3, ts=2000)
    for x in a[:2] + b[:1]:
        m.push(x)
    assert m.drain() == (b"", []) and len(m.queue) == 1         # A's fragments are consumed, B's waits
    assert m.c == counters(packets=2, orphans=2) and m.pending   # and A's loss is on record
    m.push(b[1])
    _, f = m.drain()
    assert f[0]["flags"] == FRAGMENTED | DISCONT and m.c == counters(packets=4, orphans=2, frames=1, discontinuities=1)
    # the same in one drain gives the same totals
    assert depacketise(a[:2] + b, framing=RAW)[2] == m.c


# ---- ADTS ----

def test_adts_header_bytes():
    assert adts_header(1, 2, 4, 2)[:4] == bytes.fromhex("FFF15080")           # AAC-LC 44.1 kHz stereo
    assert adts_header(300, 2, 4, 2) == bytes([0xFF, 0xF1, 0x50, 0x80, 307 >> 3, ((307 & 7) << 5) | 0x1F, 0xFC])
    assert adts_header(8184, 4, 12, 7) == bytes([0xFF, 0xF1, 0xC0 | (12 << 2) | 1, 0xC0 | 3, 0xFF, 0xFF, 0xFC])
    b, f, c = depacketise([pk(1, hbr([10, 5]) + A + C)], object_type=2, freq_index=4, channels=2)
    assert b == adts_header(10, 2, 4, 2) + A + adts_header(5, 2, 4, 2) + C
    assert [(x["offset"], x["bytes"]) for x in f] == [(0, 17), (17, 12)]      # the header is in `bytes`


def test_frame_too_long_for_adts_is_dropped():
    body = bytes(8185)
    p = frags(body, 1400) + [pk(16, hbr([10]) + A, ts=9000)]
    b, f, c = depacketise(p)
    assert c == counters(packets=7, unsupported=6, frames=1, discontinuities=1) and f[0]["flags"] == DISCONT
    assert depacketise(p, framing=RAW)[2] == counters(packets=7, frames=2)
    ok = frags(bytes(8184), 1400)
    assert depacketise(ok)[1][0]["bytes"] == 8191


# ---- round trips ----

def round_trip(frames, **kw):
    packets = at.packetise(frames, **kw)
    b, rows, c = depacketise(packets, mode=HBR if kw.get("hbr", True) else LBR, framing=ADTS)
    prof, freq, chan, got = adts_reader.read(b)
    assert (prof, freq, chan) == (1, 4, 2)
    assert c["frames"] == len(frames) and c["packets"] == len(packets)
    assert c["malformed"] == c["orphans"] == c["unsupported"] == c["skipped"] == c["discontinuities"] == 0
    return got, rows, packets


def test_round_trip_every_hbr_length():
    frames = [at.frame(n) for n in range(1, 8185)]
    got, rows, packets = round_trip(frames, mtu=1400)
    assert got == frames
    assert [r["rtp_ts"] for r in rows] == [(1024 * k) & 0xFFFFFFFF for k in range(len(frames))]
    assert any(r["flags"] & FRAGMENTED for r in rows) and any(r["au_index"] == 15 for r in rows)


def test_round_trip_every_lbr_length():
    frames = [at.frame(n, 3) for n in range(1, 64)]
    got, rows, _ = round_trip(frames, hbr=False, mtu=1400)
    assert got == frames and max(r["au_index"] for r in rows) == 15


@pytest.mark.parametrize("count", range(1, 17))
def test_round_trip_every_aggregation_count(count):
    for hbr_mode in (True, False):
        frames = [at.frame(1 + (5 * k + count) % 60, count) for k in range(3 * count + 1)]
        got, rows, packets = round_trip(frames, hbr=hbr_mode, mtu=1400, max_aus=count)
        assert got == frames and len(packets) == 4 and max(r["au_index"] for r in rows) == count - 1
