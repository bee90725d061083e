"""CPU: the FLV part of the C ABI -- the records' layouts against C and the ctypes / numpy mirrors, the
entry points declared, exported and bound, NULL arguments refused before any device work, and
edgpu_flv_header (host only) byte for byte: the file header, the onMetaData tag, the AVC sequence
header against the avcC box of edgpu_mp4_init for every SPS of tests/test_mp4_init.py."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import flv_demux
import flv_model as fm
import mp4_demux
from easydarwin_amd import edgpu
from test_mp4_init import CASES, PPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "edgpu.h")

RECORDS = [("edgpu_flv_config", edgpu.FlvConfig, None), ("edgpu_flv_state", edgpu.FlvState, edgpu.FLV_STATE_DTYPE),
           ("edgpu_flv_tag", edgpu.FlvTag, edgpu.FLV_TAG_DTYPE), ("edgpu_flv_result", edgpu.FlvResult, None)]


def test_layouts_match_c(tmp_path):
    lines = []
    for cname, mirror, _ in RECORDS:
        fields = [f for f, _ in mirror._fields_]
        lines.append(f'printf("%zu", sizeof({cname}));')
        lines += [f'printf(" %zu", offsetof({cname}, {f}));' for f in fields]
        lines.append('printf("\\n");')
    lines.append('printf("%u %u %u\\n", EDGPU_FLV_FILE, EDGPU_FLV_META, EDGPU_FLV_SEQ);')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "edgpu.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    for (cname, mirror, dtype), line in zip(RECORDS, out):
        got = [int(v) for v in line.split()]
        assert got[0] == C.sizeof(mirror), cname
        assert got[1:] == [getattr(mirror, f).offset for f, _ in mirror._fields_], cname
        if dtype is not None:
            assert dtype.itemsize == got[0] and [dtype.fields[f][1] for f, _ in mirror._fields_] == got[1:], cname
    assert [C.sizeof(m) for _, m, _ in RECORDS] == [16, 24, 40, 16]
    assert [int(v) for v in out[-1].split()] == [edgpu.FLV_FILE, edgpu.FLV_META, edgpu.FLV_SEQ] == [fm.FILE, fm.META, fm.SEQ]


def test_declared_exported_and_bound():
    src = open(HEADER).read()
    for s in ("edgpu_flv_mux", "edgpu_flv_header"):
        assert re.search(rf"\b{s}\s*\(", src), s
        assert s in edgpu.EXPORTED
    lib = edgpu.load()
    out = subprocess.run(["nm", "-D", "--defined-only", edgpu.LIB_PATH], capture_output=True, text=True).stdout
    for s in ("edgpu_flv_mux", "edgpu_flv_header"):
        assert re.search(rf"\bT {s}$", out, re.M), s
    assert len(lib.edgpu_flv_mux.argtypes) == 15 and len(lib.edgpu_flv_header.argtypes) == 9
    for section in ("H.264 elementary-stream tap", "MPEG-2 transport-stream mux", "Fragmented MP4 (CMAF) mux"):
        body = src[src.index("---- " + section):]
        assert "edgpu_flv_mux" in body[:body.index("typedef struct")], section      # the muxers name each other
    assert (edgpu.TAP_KEY, edgpu.TAP_PARAMS, edgpu.TAP_DAMAGED) == (fm.KEY, fm.PARAMS, fm.DAMAGED)


def test_null_arguments_are_refused_before_any_device_work():
    lib = edgpu.load()
    res = edgpu.FlvResult()
    one = np.zeros(1, dtype=np.uint8)
    assert lib.edgpu_flv_mux(None, None, None, 0, edgpu.PTR_HOST, None, 0, None, 0, None, None, 0, edgpu.PTR_HOST, None,
                             C.byref(res)) == edgpu.BAD_ARGUMENT
    assert lib.edgpu_flv_mux(None, None, one.ctypes.data, 1, edgpu.PTR_HOST, None, 0, None, 0, None, one.ctypes.data, 1,
                             edgpu.PTR_HOST, None, None) == edgpu.BAD_ARGUMENT
    n = C.c_uint64()
    sps = CASES["baseline 640x480"][0]
    assert lib.edgpu_flv_header(None, len(sps), PPS, len(PPS), 0, 0, one.ctypes.data, 1, C.byref(n)) == edgpu.BAD_ARGUMENT
    assert lib.edgpu_flv_header(sps, len(sps), None, len(PPS), 0, 0, one.ctypes.data, 1, C.byref(n)) == edgpu.BAD_ARGUMENT
    assert lib.edgpu_flv_header(sps, len(sps), PPS, len(PPS), 0, 0, one.ctypes.data, 1, None) == edgpu.BAD_ARGUMENT
    assert lib.edgpu_flv_header(sps, len(sps), PPS, len(PPS), 0, 0, None, 1, C.byref(n)) == edgpu.BAD_ARGUMENT


# ---- edgpu_flv_header ----

def avcc_of(sps, pps):
    """The payload of the avcC box inside edgpu_mp4_init's output."""
    init = edgpu.mp4_init(sps, pps)
    at = init.index(b"avcC")
    size = int.from_bytes(init[at - 4:at], "big")
    return init[at + 4:at - 4 + size]


def test_file_header_and_meta_byte_for_byte():
    sps, width, height, _ = CASES["high 1920x1080"]
    assert edgpu.flv_header(sps, PPS, parts=edgpu.FLV_FILE) == bytes.fromhex("464C5601010000000900000000")
    meta = edgpu.flv_header(sps, PPS, parts=edgpu.FLV_META)
    want = (bytes.fromhex("12" "00004D" "000000" "00" "000000")
            + bytes.fromhex("02000A") + b"onMetaData" + bytes.fromhex("0800000003")
            + bytes.fromhex("0005") + b"width" + b"\x00" + struct.pack(">d", 1920.0)
            + bytes.fromhex("0006") + b"height" + b"\x00" + struct.pack(">d", 1080.0)
            + bytes.fromhex("000C") + b"videocodecid" + b"\x00" + struct.pack(">d", 7.0)
            + bytes.fromhex("000009") + bytes.fromhex("00000058"))
    assert meta == want and len(meta) == 92
    assert struct.pack(">d", 1920.0) == bytes.fromhex("409E000000000000")


def test_parts():
    sps = CASES["baseline 640x480"][0]
    file, meta, seq = (edgpu.flv_header(sps, PPS, 0x01ABCDEF, p) for p in (edgpu.FLV_FILE, edgpu.FLV_META, edgpu.FLV_SEQ))
    assert len(file) == 13 and len(meta) == 92
    for parts in range(8):
        want = b"".join(b for bit, b in ((1, file), (2, meta), (4, seq)) if (parts or 7) & bit)
        assert edgpu.flv_header(sps, PPS, 0x01ABCDEF, parts) == want, parts
    assert seq[4:8] == bytes.fromhex("ABCDEF01")            # the timestamp's low 24 bits, then its extension byte
    assert seq != edgpu.flv_header(sps, PPS, 0, edgpu.FLV_SEQ) and meta == edgpu.flv_header(sps, PPS, 0, edgpu.FLV_META)
    with pytest.raises(edgpu.EdgpuError) as e:
        edgpu.flv_header(sps, PPS, 0, 8)
    assert e.value.code == edgpu.BAD_ARGUMENT


@pytest.mark.parametrize("name", sorted(CASES))
def test_sequence_header_is_the_avcc_payload(name):
    sps, width, height, ext = CASES[name]
    rec = avcc_of(sps, PPS)
    d = mp4_demux.init_segment(edgpu.mp4_init(sps, PPS))
    assert (d["sps"], d["pps"], d["avcc_ext"]) == (sps, PPS, ext)
    assert rec.endswith(PPS + ext) and rec[8:8 + len(sps)] == sps
    for ms in (0, 0x7FEDCBA9):
        whole = edgpu.flv_header(sps, PPS, ms)
        assert whole == fm.header(rec, width, height, ms)
        meta, seq = flv_demux.file(whole)
        assert meta["meta"] == dict(width=float(width), height=float(height), videocodecid=7.0)
        assert seq["timestamp"] == ms and seq["key"] and seq["packet_type"] == 0
        assert seq["config"] == dict(sps=sps, pps=PPS, ext=ext, record=rec)
        assert whole[13 + 92 + 16:-4] == rec


def test_header_then_tags_parse_as_a_file():
    sps = CASES["high 1920x1080"][0]
    es = b"\x00\x00\x00\x01" + sps + b"\x00\x00\x00\x01" + PPS + b"\x00\x00\x00\x01\x65" + bytes(range(1, 90))
    tags, rows, _ = fm.mux_stream(None, [(es, 0, fm.KEY | fm.PARAMS), (b"\x00\x00\x00\x01\x41\x07", 3000, 0)])
    r = rows[0]
    got_sps, got_pps = tags[r["sps_offset"]:][:r["sps_bytes"]], tags[r["pps_offset"]:][:r["pps_bytes"]]
    assert (got_sps, got_pps) == (sps, PPS)
    parsed = flv_demux.file(edgpu.flv_header(got_sps, got_pps, r["timestamp_ms"]) + tags)
    assert [t["type"] for t in parsed] == [18, 9, 9, 9]
    assert parsed[2]["nals"][:2] == [sps, PPS] and parsed[2]["key"] and not parsed[3]["key"]


def raw(sps_nal, pps_nal, cap=4096, parts=0):
    lib = edgpu.load()
    buf = C.create_string_buffer(b"\xA7" * max(cap, 1), max(cap, 1))
    n = C.c_uint64(0)
    rc = lib.edgpu_flv_header(sps_nal, len(sps_nal), pps_nal, len(pps_nal), 0, parts, buf if cap else None, cap, C.byref(n))
    return rc, n.value, buf.raw[:cap]


def test_documented_codes():
    good = CASES["high 1920x1080"][0]
    rc, n, data = raw(good, PPS)
    assert rc == edgpu.OK and data[n:] == b"\xA7" * (4096 - n)
    for cap in (0, 8, n - 1):                               # a short buffer: the size comes back, nothing is written
        rc2, need, data = raw(good, PPS, cap)
        assert rc2 == edgpu.OUT_OVERFLOW and need == n and data == b"\xA7" * cap
    assert raw(good, PPS, 12, edgpu.FLV_FILE)[:2] == (edgpu.OUT_OVERFLOW, 13)
    for cut in range(4, len(good) - 1):                     # truncated: the parse runs off the end
        assert raw(good[:cut], PPS)[0] == edgpu.BAD_ARGUMENT, cut
    assert raw(PPS, PPS)[0] == edgpu.BAD_ARGUMENT           # not an SPS
    assert raw(good, good)[0] == edgpu.BAD_ARGUMENT         # not a PPS
    assert raw(bytes([0x65]) + good[1:], PPS)[0] == edgpu.BAD_ARGUMENT
    assert raw(good, PPS, parts=8)[0] == edgpu.BAD_ARGUMENT
    with pytest.raises(edgpu.EdgpuError) as e:
        edgpu.flv_header(PPS, good)
    assert e.value.code == edgpu.BAD_ARGUMENT
