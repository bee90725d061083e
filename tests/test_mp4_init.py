"""CPU: edgpu_mp4_init (ftyp + moov for one H.264 track) against libedgpu.so, no device: SPS vectors
from this file's own exp-Golomb bit writer go in, and tests/mp4_demux.py reads back the same SPS /
PPS, the width and height the SPS codes, the timescale and the avcC extension bytes."""
import ctypes as C

import pytest

import mp4_demux
from easydarwin_amd import edgpu


class BitWriter:
    def __init__(self):
        self.bits = []

    def u(self, n, v):
        self.bits += [(v >> (n - 1 - i)) & 1 for i in range(n)]
        return self

    def ue(self, v):
        n = (v + 1).bit_length()
        return self.u(n - 1, 0).u(n, v + 1)

    def se(self, v):
        return self.ue(2 * v - 1 if v > 0 else -2 * v)

    def rbsp(self):
        bits = self.bits + [1]
        bits += [0] * (-len(bits) % 8)
        return bytes(int("".join(map(str, bits[i:i + 8])), 2) for i in range(0, len(bits), 8))


def escape(rbsp: bytes) -> bytes:
    out, zeros = bytearray(), 0
    for b in rbsp:
        if zeros >= 2 and b <= 3:
            out.append(3)
            zeros = 0
        out.append(b)
        zeros = zeros + 1 if b == 0 else 0
    return bytes(out)


def sps(profile, level, w_mbs, h_map, frame_mbs_only=1, crop=None, chroma=None, depth=(8, 8), scaling=False, separate=0,
        sps_id=0, poc_type=0, poc_offset=-3):
    w = BitWriter().u(8, profile).u(8, 0).u(8, level).ue(sps_id)
    if chroma is not None:
        w.ue(chroma)
        if chroma == 3:
            w.u(1, separate)
        w.ue(depth[0] - 8).ue(depth[1] - 8).u(1, 0).u(1, 1 if scaling else 0)
        if scaling:
            for i in range(8 if chroma != 3 else 12):
                present = i in (0, 6, 7)
                w.u(1, 1 if present else 0)
                if present:
                    n = 16 if i < 6 else 64
                    if i == 7:
                        w.se(-8)                            # next scale 0: the rest of the list is not coded
                    else:
                        for j in range(n):
                            w.se((j % 5) - 2)
    w.ue(0).ue(poc_type)
    if poc_type == 0:
        w.ue(2)
    elif poc_type == 1:
        w.u(1, 0).se(poc_offset).se(4).ue(2).se(1).se(-1)
    w.ue(3).u(1, 0).ue(w_mbs - 1).ue(h_map - 1).u(1, frame_mbs_only)
    if not frame_mbs_only:
        w.u(1, 0)
    w.u(1, 1)
    if crop:
        w.u(1, 1)
        for c in crop:
            w.ue(c)
    else:
        w.u(1, 0)
    w.u(1, 0)                                               # vui_parameters_present_flag
    return bytes([0x67]) + escape(w.rbsp())


PPS = bytes([0x68, 0xCE, 0x3C, 0x80])

CASES = {
    "baseline 640x480": (sps(66, 30, 40, 30), 640, 480, b""),
    "high 1920x1080": (sps(100, 40, 120, 68, crop=(0, 0, 0, 4), chroma=1), 1920, 1080, bytes([0xFD, 0xF8, 0xF8, 0])),
    "high, scaling lists": (sps(100, 31, 80, 45, chroma=1, scaling=True), 1280, 720, bytes([0xFD, 0xF8, 0xF8, 0])),
    "interlaced": (sps(100, 40, 120, 34, frame_mbs_only=0, crop=(0, 0, 0, 2), chroma=1, poc_type=1), 1920, 1080,
                   bytes([0xFD, 0xF8, 0xF8, 0])),
    "4:4:4": (sps(244, 40, 20, 15, crop=(1, 2, 3, 4), chroma=3, depth=(10, 9)), 320 - 3, 240 - 7, b""),
    "high 10 4:2:2": (sps(122, 40, 20, 15, crop=(1, 2, 3, 4), chroma=2, depth=(10, 10)), 320 - 6, 240 - 7, bytes([0xFE, 0xFA, 0xFA, 0])),
    "monochrome": (sps(100, 40, 20, 15, crop=(1, 0, 1, 0), chroma=0), 319, 239, bytes([0xFC, 0xF8, 0xF8, 0])),
}
# a long exp-Golomb code (offset_for_non_ref_pic) puts 00 00 0x into the RBSP: the first offset whose SPS needs an escape
CASES["emulation prevention"] = next((n, 640, 480, b"") for n in (sps(66, 30, 40, 30, poc_type=1, poc_offset=v)
                                                                   for v in range(1 << 28, (1 << 28) + 64)) if b"\x00\x00\x03" in n)


@pytest.mark.parametrize("name", sorted(CASES))
def test_init_segment(name):
    nal, width, height, ext = CASES[name]
    for timescale in (0, 12800):
        d = mp4_demux.init_segment(edgpu.mp4_init(nal, PPS, timescale))
        assert d["sps"] == nal and d["pps"] == PPS
        assert (d["width"], d["height"]) == (width, height) == (d["tkhd_width"], d["tkhd_height"])
        assert d["timescale"] == (timescale or 90000)
        assert d["avcc_ext"] == ext


def raw(sps_nal, pps_nal, cap=4096):
    lib = edgpu.load()
    buf = C.create_string_buffer(b"\xA7" * max(cap, 1), max(cap, 1))
    n = C.c_uint64(0)
    rc = lib.edgpu_mp4_init(sps_nal, len(sps_nal), pps_nal, len(pps_nal), 0, buf if cap else None, cap, C.byref(n))
    return rc, n.value, buf.raw[:cap]


def test_documented_codes():
    good = CASES["high 1920x1080"][0]
    rc, n, data = raw(good, PPS)
    assert rc == edgpu.OK and data[n:] == b"\xA7" * (4096 - n)
    for cap in (0, 8, n - 1):                               # a short buffer: the size comes back, nothing is written
        rc2, need, data = raw(good, PPS, cap)
        assert rc2 == edgpu.OUT_OVERFLOW and need == n and data == b"\xA7" * cap
    for cut in range(4, len(good) - 1):                     # truncated: the parse runs off the end
        assert raw(good[:cut], PPS)[0] == edgpu.BAD_ARGUMENT, cut
    assert raw(PPS, PPS)[0] == edgpu.BAD_ARGUMENT           # not an SPS
    assert raw(good, good)[0] == edgpu.BAD_ARGUMENT         # not a PPS
    assert raw(bytes([0x65]) + good[1:], PPS)[0] == edgpu.BAD_ARGUMENT
    with pytest.raises(edgpu.EdgpuError) as e:
        edgpu.mp4_init(PPS, good)
    assert e.value.code == edgpu.BAD_ARGUMENT
