"""CPU: tests/ts_model.py (the rules of edgpu_ts_mux) against bytes written out by hand and against
tests/ts_demux.py, a demultiplexer that shares nothing with it."""
import pytest

import ts_demux
import ts_model as tm
from ts_model import AUD, KEY, NOAUD, Config, mux_stream

PAT = bytes.fromhex("00B00D0001C100000001F0002AB104B2")
PMT = bytes.fromhex("02B0120001C10000E100F0001BE100F00015BD4D56")


def test_psi_sections_of_the_default_configuration():
    assert tm.pat_section(Config()) == PAT
    assert tm.pmt_section(Config()) == PMT
    assert tm.crc32_mpeg2(PAT) == 0 and tm.crc32_mpeg2(PMT) == 0
    assert tm.crc32_mpeg2(b"123456789") == 0x0376E6E7         # the catalogue's check value of CRC-32/MPEG-2


def test_hand_written_key_unit():
    es = bytes([0, 0, 0, 1, 0x65])
    out, rows, st = mux_stream(None, [(es, 90000, KEY)])
    # pts 90000 = 0x15F90; pcr base 27000 = 0x6978
    pat = bytes.fromhex("47400010 00") + PAT + b"\xFF" * (188 - 5 - 16)
    pmt = bytes.fromhex("47500010 00") + PMT + b"\xFF" * (188 - 5 - 21)
    pes = bytes.fromhex("000001E0 0000 84 80 05 21 0005 BF21 00000001 09F0") + es
    assert len(pes) == 25
    video = bytes.fromhex("47410030") + bytes([7 + 151, 0x50]) + bytes.fromhex("000034BC 7E00") + b"\xFF" * 151 + pes
    assert out == pat + pmt + video
    assert rows == [dict(offset=0, bytes=564, flags=KEY, pts=90000, stream=0)]
    assert st == dict(ext_ts=90000, started=1, cc_pat=1, cc_pmt=1, cc_video=1)


def test_hand_written_non_key_unit():
    es = bytes([0, 0, 0, 1, 0x09, 0xF0, 0, 0, 0, 1, 0x41, 0x9A])        # it brings its own delimiter
    state = dict(ext_ts=90000, started=1, cc_pat=3, cc_pmt=3, cc_video=15)
    out, rows, st = mux_stream(None, [(es, 93000, 0)], state)
    # pts 93000 = 0x16B48; pcr base 30000 = 0x7530
    pes = bytes.fromhex("000001E0 0000 84 80 05 21 0005 D691") + es
    video = bytes.fromhex("4741003F") + bytes([7 + 150, 0x10]) + bytes.fromhex("00003A98 7E00") + b"\xFF" * 150 + pes
    assert out == video
    assert st == dict(ext_ts=93000, started=1, cc_pat=3, cc_pmt=3, cc_video=0)


@pytest.mark.parametrize("v", [0, 1, (1 << 32) - 1, 1 << 32, (1 << 33) - 1, (1 << 33) + 5])
def test_pts_and_pcr_bytes(v):
    off = v - 7
    cfg = Config(pts_offset=off % (1 << 64), pcr_lead=1000)
    out, rows, _ = mux_stream(cfg, [(b"\x00\x00\x00\x01\x41", 7, 0)])
    pts = v % (1 << 33)
    pcr = (v - 1000) % (1 << 33)
    assert rows[0]["pts"] == pts
    want_pts = bytes([0x21 | ((pts >> 30) << 1), (pts >> 22) & 0xFF, (((pts >> 15) & 0x7F) << 1) | 1, (pts >> 7) & 0xFF, ((pts & 0x7F) << 1) | 1])
    want_pcr = ((pcr << 15) | (0x3F << 9)).to_bytes(6, "big")
    assert out[6:12] == want_pcr
    i = out.index(b"\x00\x00\x01\xE0")
    assert out[i + 9:i + 14] == want_pts
    d = ts_demux.demux(out)["pes"][0]
    assert d["pts"] == pts and d["pcr"] == (pcr, 0)


def test_pcr_base_wraps_below_zero():
    out, rows, _ = mux_stream(None, [(b"\x00\x00\x00\x01\x41", 100, 0)])
    d = ts_demux.demux(out)["pes"][0]
    assert d["pts"] == 100 and d["pcr"] == ((1 << 33) + 100 - 63000, 0)


def es_unit(n, k=0, nal=0x41):
    body = bytes([0, 0, 0, 1, nal]) + bytes((k * 31 + 7 * j) & 0xFF for j in range(max(n - 5, 0)))
    return body[:n]


@pytest.mark.parametrize("flags", [AUD, NOAUD])
def test_round_trip_every_length(flags):
    cfg = Config(flags=flags)
    units = [(es_unit(n, n, 0x09 if n % 7 == 3 else 0x41), 3000 * n, KEY if n % 50 == 1 else 0) for n in range(1, 3001)]
    out, rows, st = mux_stream(cfg, units)
    d = ts_demux.demux(out)
    assert d["video_pid"] == 0x100 and d["pcr_pid"] == 0x100 and d["pmt_pid"] == 0x1000 and d["stream_type"] == 0x1B
    assert d["pat"] == d["pmt"] == 60 and len(d["pes"]) == 3000
    for (es, ts, fl), e, r in zip(units, d["pes"], rows):
        due = flags == AUD and (len(es) < 5 or es[4] & 0x1F != 9)
        assert e["payload"] == (b"\x00\x00\x00\x01\x09\xF0" if due else b"") + es, len(es)
        assert e["pts"] == ts and e["rai"] == bool(fl & KEY)
        assert e["packet"] * 188 == r["offset"] + (376 if fl & KEY else 0)
        p = 14 + (6 if due else 0) + len(es)
        assert r["bytes"] == 188 * (2 * bool(fl & KEY) + 1 + -(-max(0, p - 176) // 184))


def sequence():
    ts = [(1 << 32) - 7000, (1 << 32) - 4000, (1 << 32) - 1000, 2000, 5000, 3500, 8000, 8000, 11000]
    units = []
    for k, t in enumerate(ts * 3):
        n = [5, 170, 0, 700, 162, 156, 0, 3000, 346][k % 9]
        units.append((es_unit(n, k, 0x65 if k % 4 == 0 else 0x41), t + 9000 * (k // 9), KEY if k % 4 == 0 and n else 0))
    return units


def test_one_call_equals_a_call_per_unit():
    cfg = Config(pts_offset=(1 << 33) - (1 << 32) - 100)
    units = sequence()
    whole, rows, st = mux_stream(cfg, units)
    state, parts, prow = tm.new_state(), b"", []
    for u in units:
        b, r, state = mux_stream(cfg, [u], state)
        prow.append(dict(r[0], offset=len(parts)))
        parts += b
    assert parts == whole and state == st and prow == rows
    d = ts_demux.demux(whole)
    with_es = [(u, r) for u, r in zip(units, rows) if u[0]]
    assert [e["pts"] for e in d["pes"]] == [r["pts"] for _, r in with_es]
    # signed steps: the step back gives a smaller PTS, the wrap of the RTP timestamp does not
    ext = [r["pts"] for r in rows]
    assert (ext[5] - ext[4]) % (1 << 33) == (1 << 33) - 1500 and (ext[3] - ext[2]) % (1 << 33) == 3000
    assert any(a > b for a, b in zip(ext, ext[1:]))             # the PTS crosses 2^33 too


def test_zero_byte_unit_advances_the_clock_only():
    out, rows, st = mux_stream(None, [(b"", 500, KEY), (es_unit(9), 3500, 0)])
    assert rows[0] == dict(offset=0, bytes=0, flags=KEY, pts=500, stream=0) and rows[1]["offset"] == 0
    assert st == dict(ext_ts=3500, started=1, cc_pat=0, cc_pmt=0, cc_video=1) and len(out) == 188
