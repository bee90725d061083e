"""CPU: tests/stats_model.py, the restatement the GPU statistics are compared with, pinned on
vectors worked out by hand (RFC 3550 A.1 / A.8, ReflectorStream::UpdateBitRate)."""
import struct

import pytest

from stats_model import SessionModel, StreamModel, clock_rate_of


def rtp(seq, ts=0, ssrc=0x11223344, size=12):
    return struct.pack(">BBHII", 0x80, 96, seq & 0xFFFF, ts & 0xFFFFFFFF, ssrc) + bytes(size - 12)


def run(seqs, clock=0):
    m = StreamModel(clock, False, 0)
    for s in seqs:
        m.push(0, 0, rtp(s))
    return m.record()


def test_sequence_wrap_counts_a_cycle():
    r = run([65534, 65535, 0, 1])
    assert (r["cycles"], r["base_seq"], r["max_seq"], r["expected"], r["received"], r["lost"]) == (65536, 65534, 1, 4, 4, 0)


def test_jump_of_3000_restarts_on_its_successor_and_2999_does_not():
    r = run([10, 3010])                     # udelta 3000: not accepted, bad_seq = 3011
    assert (r["received"], r["max_seq"], r["bad_seq"], r["restarts"]) == (1, 10, 3011, 0)
    r = run([10, 3010, 3011])               # its successor: init_seq(3011)
    assert (r["restarts"], r["base_seq"], r["max_seq"], r["received"], r["expected"], r["bad_seq"]) == \
        (1, 3011, 3011, 1, 1, 0x10000)
    r = run([10, 3009])                     # udelta 2999: an ordinary loss of 2998
    assert (r["restarts"], r["max_seq"], r["received"], r["expected"], r["lost"]) == (0, 3009, 2, 3000, 2998)


def test_misorder_window_is_below_100():
    # udelta = 65536 - k; accepted as misordered only when udelta > 65536 - 100, i.e. k < 100
    r = run([1000, 901])                    # 99 behind
    assert (r["misordered"], r["received"], r["max_seq"]) == (1, 2, 1000)
    for behind in (100, 101):
        r = run([1000, 1000 - behind])
        assert (r["misordered"], r["received"], r["bad_seq"]) == (0, 1, 1000 - behind + 1)


def test_duplicate_is_accepted_and_not_misordered():
    r = run([5, 5])
    assert (r["received"], r["misordered"], r["expected"], r["lost"]) == (2, 0, 1, -1)


def test_single_loss():
    r = run([7, 8, 10])
    assert (r["expected"], r["received"], r["lost"]) == (4, 3, 1)


def test_ssrc_change_restarts_the_stream():
    m = StreamModel(8000, False, 0)
    m.push(0, 1000, rtp(100, 0))
    m.push(0, 1040, rtp(101, 0))            # d = 320: jitter 320
    assert m.jitter_scaled == 320
    m.push(0, 1080, rtp(7, 0, ssrc=0x55))
    r = m.record()
    assert (r["ssrc_changes"], r["ssrc"], r["base_seq"], r["received"], r["jitter_scaled"], r["has_transit"]) == \
        (1, 0x55, 7, 1, 0, 1)
    assert r["packets"] == 3


def test_constant_spacing_gives_no_jitter():
    m = StreamModel(90000, False, 0)
    for i in range(50):
        m.push(0, 1_000_000 + 40 * i, rtp(i, 777 + 3600 * i))
    assert m.record()["jitter_scaled"] == 0 and m.record()["received"] == 50


def test_four_packet_jitter_by_hand():
    """Clock 8000 (8 units / ms).  Arrivals 1000, 1020, 1045, 1060 ms -> 8000, 8160, 8360, 8480;
    timestamps 0, 160, 320, 480; transits 8000, 8000, 8040, 8000; |D| = 0, 40, 40.
    J: 0 -> 0 + 0 - (8 >> 4) = 0 -> 0 + 40 - (8 >> 4) = 40 -> 40 + 40 - (48 >> 4 = 3) = 77."""
    m = StreamModel(8000, False, 0)
    for i, t in enumerate((1000, 1020, 1045, 1060)):
        m.push(0, t, rtp(i, 160 * i))
    r = m.record()
    assert (r["jitter_scaled"], r["jitter"], r["transit"]) == (77, 4, 8000)


def test_rtp_timestamp_wrap():
    m = StreamModel(90000, False, 0)
    for i in range(4):                      # 0xFFFFF000 + 3600 i wraps at i = 2
        m.push(0, 5000 + 40 * i, rtp(i, 0xFFFFF000 + 3600 * i))
    assert m.record()["jitter_scaled"] == 0
    m.push(0, 5000 + 40 * 4 + 5, rtp(4, 0xFFFFF000 + 3600 * 4))     # 5 ms late: 450 units
    assert m.record()["jitter_scaled"] == 450


def test_arrival_rtp_wrap():
    """47721840 ms * 90 = 4294965600 < 2^32; 40 ms later 4294969200 wraps to 1904."""
    m = StreamModel(90000, False, 0)
    m.push(0, 47721840, rtp(0, 1000))
    assert m.transit == 4294964600
    m.push(0, 47721880, rtp(1, 4600))
    assert (m.transit, m.jitter_scaled) == (4294964600, 0)
    m.push(0, 47721925, rtp(2, 8200))       # 45 ms after: 4050 - 3600 = 450
    assert m.jitter_scaled == 450


def test_no_clock_rate_no_jitter():
    m = StreamModel(0, False, 0)
    m.push(0, 10, rtp(0, 0))
    m.push(0, 500, rtp(1, 0))
    assert (m.jitter_scaled, m.has_transit, m.received) == (0, 0, 2)


@pytest.mark.parametrize("name,rate", [("H264/90000", 90000), ("MPEG4-GENERIC/44100/2", 44100), ("PCMA/8000", 8000),
                                       ("H264", 0), ("X/", 0), ("X/abc", 0), (b"L16/48000/2", 48000)])
def test_clock_rate_parsing(name, rate):
    assert clock_rate_of(name) == rate


def test_short_and_empty_packets():
    m = StreamModel(90000, False, 0)
    m.push(0, 1, b"")
    m.push(0, 1, bytes(11))
    m.push(0, 1, rtp(3))
    r = m.record()
    assert (r["packets"], r["bytes"], r["short_packets"], r["received"], r["interval_bytes"]) == (2, 23, 1, 1, 23)


def test_sender_report_capture():
    sr = struct.pack(">BBHIQIII", 0x80, 200, 6, 0xAABBCCDD, 0x0102030405060708, 0x11121314, 21, 2200)
    assert len(sr) == 28
    m = StreamModel(90000, True, 0)
    m.push(1, 50, sr[:27])                  # too short
    m.push(1, 60, b"\x80\xc9" + sr[2:])     # PT 201
    assert m.sr_count == 0
    m.push(1, 70, sr + bytes(24))
    m.push(1, 80, struct.pack(">BBHIQIII", 0x80, 200, 6, 1, 2, 3, 4, 5))
    r = m.record()
    assert (r["sr_count"], r["sr_ntp"], r["sr_rtp"], r["sr_packets"], r["sr_octets"], r["sr_arrival_ms"]) == (2, 2, 3, 4, 5, 80)
    assert (r["rtcp_packets"], r["rtcp_bytes"]) == (4, 27 + 28 + 52 + 28)
    assert r["interval_bytes"] == 0         # UDP push: the odd port is RTCP


def test_tcp_push_counts_both_channels_in_the_bitrate():
    s = SessionModel(["H264/90000"], False, 0)
    s.push(0, 1, rtp(0, size=100))
    s.push(1, 1, bytes(40))
    assert s.records()[0]["interval_bytes"] == 140


def test_bitrate_sample_is_strictly_after_30_s():
    m = StreamModel(0, False, 1000)
    for _ in range(3):
        m.push(0, 1500, bytes(1000))
    m.sample(31000)                         # 1000 + 30000 < 31000 is false
    assert (m.bitrate, m.interval_bytes, m.last_sample_ms) == (0, 3000, 1000)
    m.sample(31001)                         # float32(24000) / float32(30001) * 1000 = 799.97...
    assert (m.bitrate, m.interval_bytes, m.last_sample_ms) == (799, 0, 31001)
    m.sample(31001)                         # the stream's second sender at the same `now`: no-op
    m.sample(31002)
    assert (m.bitrate, m.last_sample_ms) == (799, 31001)


def test_bitrate_is_two_float32_operations():
    """961712 bits / 30001 ms: the float32 quotient 32.056 times 1000 is 32056; in double
    arithmetic it would be 32055."""
    m = StreamModel(0, False, 0)
    m.interval_bytes = 120214
    m.sample(30001)
    assert m.bitrate == 32056


def test_bitrate_keeps_the_32_bit_wrap():
    m = StreamModel(0, False, 0)
    m.interval_bytes = 600_000_000          # * 8 = 4.8e9 -> 505032704 mod 2^32
    m.sample(30001)
    assert m.bitrate == 16833864


def test_packets_over_2060_are_clamped():
    s = SessionModel(["H264/90000"], False, 0)
    s.push(0, 1, rtp(0, size=3000))
    assert s.records()[0]["bytes"] == 2060
