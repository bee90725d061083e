"""CPU: tests/tap_model.py (the executable statement of the tap's rules) against a round trip that
knows nothing of the model, and hand-written vectors for every rule."""
import struct

import numpy as np
import pytest

import tap_traces as tt
from tap_model import DAMAGED, KEY, NOMARKER, OPEN_END, PARAMS, START, TapModel, depacketise, parse


def rtp(seq, ts, m, payload, b0=0x80, tail=b""):
    return struct.pack(">BBHII", b0, (0x80 if m else 0) | 96, seq & 0xFFFF, ts, 7) + payload + tail


def fu(typ, s, e, body=b"\xAA\xBB", nri=0x60):
    return bytes([nri | 28, (0x80 if s else 0) | (0x40 if e else 0) | typ]) + body


def flags(units):
    return [u["flags"] for u in units]


# ---- round trip, no model knowledge ----

@pytest.mark.parametrize("mtu", [100, 1400])
def test_round_trip_every_nal_length(mtu):
    types = [1, 5, 7, 8, 6, 23]
    aus = [[tt.nal(types[n % len(types)], n)] for n in range(1, 3001)]
    pk, reached = tt.packetise(aus, mtu=mtu, seq0=65000)
    assert {"single", "fu", "fu-middle", "seq-wrap"} <= reached
    got, units, c = depacketise(pk, flush=False)
    assert got == tt.annexb(aus)
    assert len(units) == len(aus)
    for n, u in zip(range(1, 3001), units):
        t = types[n % len(types)]
        assert u["flags"] == (KEY if t == 5 else PARAMS if t in (7, 8) else 0), (n, u)
        assert u["bytes"] == n + 4 and u["n_nals"] == 1
    assert c["packets"] == len(pk) and not any(c[k] for k in ("skipped", "malformed", "orphans", "unsupported", "missed"))
    assert c["damaged_units"] == 0


@pytest.mark.parametrize("extra", [dict(stap=True), dict(cc=3), dict(ext=0), dict(ext=3), dict(pad=1), dict(pad=7),
                                   dict(stap=True, cc=15, ext=2, pad=4)])
def test_round_trip_with_extras(extra):
    aus = [[tt.nal(7, 24), tt.nal(8, 8), tt.nal(5, 3001)], [tt.nal(1, 50)], [tt.nal(6, 9), tt.nal(1, 1), tt.nal(1, 1500)]]
    pk, reached = tt.packetise(aus, mtu=1400, **extra)
    assert {"stap": "stap", "cc": "cc", "ext": "ext", "pad": "pad"}[next(iter(extra))] in reached
    got, units, c = depacketise(pk, flush=False)
    assert got == tt.annexb(aus)
    assert flags(units) == [KEY | PARAMS, 0, 0]
    assert [u["n_nals"] for u in units] == [3, 1, 3]


# ---- rule 1: parse ----

def test_parse_rules():
    pay = b"\x41\x01\x02"
    for cc in range(1, 16):
        p = tt.header(5, 6, True, cc=cc) + pay
        assert parse(p) == (1, 5, 6, pay)
        assert parse(p[:12 + 4 * cc]) is None                  # empty payload
    for ext in (0, 3):
        p = tt.header(5, 6, False, ext=ext) + pay
        assert parse(p) == (0, 5, 6, pay)
        assert parse(p[:14]) is None                            # the extension header does not fit
    base = rtp(1, 2, 0, pay, b0=0xA0)
    assert parse(base + b"\x01") == (0, 1, 2, pay)              # pad 1
    assert parse(base[:-1] + b"\x00") is None                   # pad 0
    n = len(base) + 1
    assert parse(base + bytes([n - 12])) is None                # pad = len - hdr: nothing left
    assert parse(base + bytes([n - 12 + 1])) is None            # reaches into the header
    assert parse(base + bytes([n - 12 - 1])) == (0, 1, 2, pay[:1])
    for v in (0, 3):
        assert parse(rtp(1, 2, 0, pay, b0=v << 6)) is None
    full = rtp(1, 2, 0, pay)
    assert [parse(full[:k]) is None for k in (0, 11, 12, 13)] == [True, True, True, False]


def test_bad_packets_are_counted_and_leave_a_gap():
    pk = [rtp(10, 100, 1, b"\x41a"), rtp(11, 200, 1, b"\x41b", b0=0x00), b"", bytes(11), rtp(12, 200, 1, b"\x41c")]
    got, units, c = depacketise(pk)
    assert got == START + b"\x41a" + START + b"\x41c"
    assert c["packets"] == 4 and c["skipped"] == 2
    assert flags(units) == [0, DAMAGED]                         # seq 11 was not trusted: 10 -> 12 is a gap


# ---- rule 4: FU-A ----

def fu_run(seqs_payloads, ts=None):
    return [rtp(s, (ts or {}).get(k, 500), m, p) for k, (s, m, p) in enumerate(seqs_payloads)]


def test_fu_complete_and_rebuilt_header():
    pk = fu_run([(1, 0, fu(5, 1, 0, b"ab")), (2, 0, fu(5, 0, 0, b"cd")), (3, 1, fu(5, 0, 1, b"ef"))])
    got, units, c = depacketise(pk)
    assert got == START + b"\x65abcdef"
    assert flags(units) == [KEY] and units[0]["n_nals"] == 1 and units[0]["n_packets"] == 3


@pytest.mark.parametrize("lost,want,orphans", [
    (0, b"", 2),                                                # S lost: nothing of the chain
    (1, START + b"\x65ab", 1),                                  # middle lost: the start survives
    (2, START + b"\x65abcd", 0),                                # E lost: the chain stays open
])
def test_fu_fault_positions(lost, want, orphans):
    run = [(1, 0, fu(5, 1, 0, b"ab")), (2, 0, fu(5, 0, 0, b"cd")), (3, 1, fu(5, 0, 1, b"ef"))]
    pk = [rtp(0, 400, 1, b"\x41x")] + fu_run([r for k, r in enumerate(run) if k != lost])
    got, units, c = depacketise(pk)
    assert got == START + b"\x41x" + want
    assert c["orphans"] == orphans
    assert units[1]["flags"] & DAMAGED
    if lost == 2:
        assert units[1]["flags"] & NOMARKER and units[1]["flags"] & OPEN_END


def test_fu_type_change_timestamp_change_and_s_with_e():
    # type change mid-chain
    got, units, c = depacketise(fu_run([(1, 0, fu(5, 1, 0, b"ab")), (2, 0, fu(1, 0, 0, b"cd")), (3, 1, fu(5, 0, 1, b"ef"))]))
    assert got == START + b"\x65ab" and c["orphans"] == 2 and flags(units) == [KEY | DAMAGED]
    # timestamp change mid-chain: a new access unit, the chain does not cross it
    got, units, c = depacketise(fu_run([(1, 0, fu(5, 1, 0, b"ab")), (2, 0, fu(5, 0, 0, b"cd")), (3, 1, fu(5, 0, 1, b"ef"))],
                                       ts={1: 600, 2: 600}))
    assert got == START + b"\x65ab" and c["orphans"] == 2
    assert flags(units) == [KEY | DAMAGED | NOMARKER, DAMAGED]
    # S and E together, and a one-byte FU payload
    got, units, c = depacketise(fu_run([(1, 0, fu(5, 1, 1, b"ab")), (2, 0, bytes([0x7C])), (3, 1, b"\x41z")]))
    assert got == START + b"\x41z" and c["malformed"] == 2 and flags(units) == [DAMAGED]
    # S and E together closes an open chain
    got, units, c = depacketise(fu_run([(1, 0, fu(5, 1, 0, b"ab")), (2, 0, fu(5, 1, 1, b"cd")), (3, 1, fu(5, 0, 1, b"ef"))]))
    assert got == START + b"\x65ab" and c["malformed"] == 1 and c["orphans"] == 1
    # a non-FU packet closes the chain
    got, units, c = depacketise(fu_run([(1, 0, fu(5, 1, 0, b"ab")), (2, 0, b"\x06s"), (3, 1, fu(5, 0, 1, b"ef"))]))
    assert got == START + b"\x65ab" + START + b"\x06s" and c["orphans"] == 1


def test_sequence_wrap_inside_a_chain():
    pk = fu_run([(65534, 0, fu(1, 1, 0, b"ab")), (65535, 0, fu(1, 0, 0, b"cd")), (0, 0, fu(1, 0, 0, b"ef")),
                 (1, 1, fu(1, 0, 1, b"gh"))])
    got, units, c = depacketise(pk)
    assert got == START + b"\x61abcdefgh" and flags(units) == [0] and c["orphans"] == 0


def test_segmented_scan_not_a_neighbour_test():
    """A fragment after a dropped one is dropped too, though its own neighbour is in sequence."""
    pk = fu_run([(1, 0, fu(5, 1, 0, b"ab")), (3, 0, fu(5, 0, 0, b"cd")), (4, 0, fu(5, 0, 0, b"ef")), (5, 1, fu(5, 0, 1, b"gh"))])
    got, units, c = depacketise(pk)
    assert got == START + b"\x65ab" and c["orphans"] == 3


# ---- STAP-A and the other types ----

def test_stap_faults_after_one_good_unit():
    good = struct.pack(">H", 3) + b"\x67ab"
    for bad in (struct.pack(">H", 0) + b"\x68", struct.pack(">H", 9) + b"\x68cd", b"\x00"):
        got, units, c = depacketise([rtp(1, 5, 1, bytes([0x78]) + good + bad)])
        assert got == START + b"\x67ab" and c["malformed"] == 1
        assert flags(units) == [PARAMS | DAMAGED] and units[0]["n_nals"] == 1
    got, units, c = depacketise([rtp(1, 5, 1, bytes([0x78]) + good + struct.pack(">H", 2) + b"\x65z")])
    assert got == START + b"\x67ab" + START + b"\x65z" and flags(units) == [KEY | PARAMS] and c["malformed"] == 0


@pytest.mark.parametrize("t", [0, 25, 26, 27, 29, 30, 31])
def test_unsupported_types(t):
    got, units, c = depacketise([rtp(1, 5, 1, bytes([0x60 | t]) + b"abc")])
    assert got == b"" and c["unsupported"] == 1 and flags(units) == [DAMAGED] and units[0]["bytes"] == 0


# ---- access units ----

def test_markerless_stream_is_cut_by_timestamp():
    pk = [rtp(k, 1000 * (k // 2), 0, bytes([0x41, k])) for k in range(6)]
    m = TapModel()
    for p in pk:
        m.push(p)
    got, units = m.drain()
    assert len(units) == 2 and flags(units) == [NOMARKER, NOMARKER]       # the third waits for a later packet
    assert len(m.queue) == 2
    got2, units2 = m.drain(flush=True)
    assert flags(units2) == [NOMARKER | OPEN_END] and got + got2 == b"".join(START + bytes([0x41, k]) for k in range(6))


def test_damage_reaches_the_previous_unit_only_without_a_marker():
    def run(marker):
        return [rtp(1, 100, 0, b"\x41a"), rtp(2, 100, marker, b"\x41b"), rtp(4, 200, 1, b"\x41c")]
    assert flags(depacketise(run(1))[1]) == [0, DAMAGED]
    assert flags(depacketise(run(0))[1]) == [DAMAGED | NOMARKER, DAMAGED]


def test_missed_packets_damage_the_next_unit():
    m = TapModel()
    for k in range(4):
        m.push(rtp(k, 100 * k, 1, bytes([0x41, k])))
    m.lose(2)
    got, units = m.drain()
    assert m.c["missed"] == 2 and flags(units) == [DAMAGED, 0] and m.c["damaged_units"] == 1


# ---- every cut ----

def three_au_run():
    aus = [[tt.nal(7, 20), tt.nal(8, 6), tt.nal(5, 700)], [tt.nal(1, 330)], [tt.nal(1, 90), tt.nal(1, 250)]]
    pk, _ = tt.packetise(aus, mtu=100, stap=True, drop=(5, 13))
    pk.insert(3, bytes(5))                                  # a bad packet and an empty entry on the way
    pk.insert(9, b"")
    return pk


@pytest.mark.parametrize("flush_last", [False, True])
def test_every_cut_equals_one_drain(flush_last):
    pk = three_au_run()
    want_b, want_u, want_c = depacketise(pk, flush=flush_last)
    assert len(want_u) == 3 and any(u["flags"] & DAMAGED for u in want_u)
    for cut in range(len(pk) + 1):
        m = TapModel()
        for k, p in enumerate(pk[:cut]):
            m.push(p, k)
        b1, u1 = m.drain()
        for k, p in enumerate(pk[cut:]):
            m.push(p, cut + k)
        b2, u2 = m.drain(flush=flush_last)
        for u in u2:
            u["offset"] += len(b1)
        assert b1 + b2 == want_b, cut
        assert u1 + u2 == want_u, cut
        assert m.c == want_c, cut


def test_synthetic_h264_stream_one_unit_per_frame():
    from easydarwin_amd.synth import TrackSpec, _video_h264
    tr = TrackSpec("video", "H264/90000", 96, bitrate=1_000_000, gop=15, idr_bytes=9000)
    _, pk = _video_h264(np.random.Generator(np.random.PCG64(11)), tr, 2000, 0)
    got, units, c = depacketise([p for _, p in pk], flush=False)
    assert len(units) == 60
    assert [k for k, u in enumerate(units) if u["flags"] & KEY] == [0, 15, 30, 45]
    assert all(u["flags"] == (KEY | PARAMS if k % 15 == 0 else 0) for k, u in enumerate(units))
    assert c["packets"] == len(pk) and c["orphans"] == 0
