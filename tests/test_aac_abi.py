"""CPU: the audio tap's part of the C ABI -- the records' layouts against C and the ctypes / numpy
mirrors, the entry points declared, exported and bound, and edgpu_aac_config_parse (host only) on
fmtp lines: both modes, keys in either case, the known configs and every refusal the header lists."""
import ctypes as C
import os
import re
import subprocess

import pytest

import aac_model
from easydarwin_amd import edgpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "edgpu.h")
NAMES = ("edgpu_aac_config_parse", "edgpu_aac_tap_enable", "edgpu_aac_tap_disable", "edgpu_aac_tap_drain")
RECORDS = [("edgpu_aac_config", edgpu.AacConfig, None), ("edgpu_aac_frame", edgpu.AacFrame, edgpu.AAC_FRAME_DTYPE),
           ("edgpu_aac_stream", edgpu.AacStream, edgpu.AAC_STREAM_DTYPE), ("edgpu_aac_result", edgpu.AacResult, None)]


def test_layouts_match_c(tmp_path):
    lines = []
    for cname, mirror, _ in RECORDS:
        lines.append(f'printf("%zu", sizeof({cname}));')
        lines += [f'printf(" %zu", offsetof({cname}, {f}));' for f, _ in mirror._fields_]
        lines.append('printf("\\n");')
    lines.append('printf("%u %u %u %u %u %u %u %u\\n", EDGPU_AAC_HBR, EDGPU_AAC_LBR, EDGPU_AAC_ADTS, EDGPU_AAC_RAW, '
                 'EDGPU_AAC_MAX_AUS, EDGPU_AAC_DISCONT, EDGPU_AAC_FRAGMENTED, EDGPU_AAC_FLUSH);')
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
    assert [C.sizeof(m) for _, m, _ in RECORDS] == [24, 48, 96, 16]
    consts = [edgpu.AAC_HBR, edgpu.AAC_LBR, edgpu.AAC_ADTS, edgpu.AAC_RAW, edgpu.AAC_MAX_AUS, edgpu.AAC_DISCONT,
              edgpu.AAC_FRAGMENTED, edgpu.AAC_FLUSH]
    assert [int(v) for v in out[-1].split()] == consts
    assert consts == [aac_model.HBR, aac_model.LBR, aac_model.ADTS, aac_model.RAW, aac_model.MAX_AUS, aac_model.DISCONT,
                      aac_model.FRAGMENTED, 1]
    assert tuple(edgpu.AAC_FRAME_DTYPE.names[:8]) == aac_model.FRAME_FIELDS
    assert tuple(edgpu.AAC_STREAM_DTYPE.names[6:]) == aac_model.COUNTERS


def test_declared_exported_and_bound():
    src = open(HEADER).read()
    lib = edgpu.load()
    out = subprocess.run(["nm", "-D", "--defined-only", edgpu.LIB_PATH], capture_output=True, text=True).stdout
    for s in NAMES:
        assert re.search(rf"\bint\s+{s}\s*\(", src), s
        assert s in edgpu.EXPORTED and re.search(rf"\bT {s}$", out, re.M), s
    assert [len(getattr(lib, s).argtypes) for s in NAMES] == [4, 4, 3, 10]
    for m in ("aac_tap_enable", "aac_tap_disable", "aac_tap_drain"):
        assert callable(getattr(edgpu.Context, m))
    assert src.index("---- FLV mux of tapped access units") < src.index("---- AAC audio tap ----")
    tap = src[src.index("---- H.264 elementary-stream tap"):src.index("#define EDGPU_TAP_KEY")]
    assert "Out of scope: audio" not in tap and "AAC audio tap" in tap      # the tap points at the new section


def test_null_arguments_are_refused_before_any_device_work():
    lib = edgpu.load()
    cfg, res = edgpu.AacConfig(), edgpu.AacResult()
    assert lib.edgpu_aac_config_parse(None, 0, 0, C.byref(cfg)) == edgpu.BAD_ARGUMENT
    assert lib.edgpu_aac_config_parse(b"m=audio", 7, 0, None) == edgpu.BAD_ARGUMENT
    assert lib.edgpu_aac_tap_enable(None, 0, 0, C.byref(cfg)) == edgpu.BAD_ARGUMENT
    assert lib.edgpu_aac_tap_disable(None, 0, 0) == edgpu.BAD_ARGUMENT
    assert lib.edgpu_aac_tap_drain(None, 0, None, 0, edgpu.PTR_HOST, None, 0, None, 0, C.byref(res)) == edgpu.BAD_ARGUMENT


# ---- edgpu_aac_config_parse ----

HBR_FMTP = "streamtype=5; profile-level-id=15; mode=AAC-hbr; config=1210; SizeLength=13; IndexLength=3; IndexDeltaLength=3"


def sdp(*fmtp, video_first=True):
    s = "v=0\r\no=- 1 1 IN IP4 127.0.0.1\r\ns=x\r\nt=0 0\r\n"
    if video_first:
        s += "m=video 0 RTP/AVP 96\r\na=rtpmap:96 H264/90000\r\na=fmtp:96 packetization-mode=1\r\na=control:trackID=1\r\n"
    for k, f in enumerate(fmtp):
        s += f"m=audio 0 RTP/AVP {97 + k}\r\na=rtpmap:{97 + k} MPEG4-GENERIC/44100/2\r\n"
        if f is not None:
            s += f"a=fmtp:{97 + k} {f}\r\n"
        s += f"a=control:trackID={2 + k}\r\n"
    return s


def fields(c):
    return (c.mode, c.framing, c.object_type, c.freq_index, c.channels, c.frame_samples)


def test_both_modes_either_case_and_known_configs():
    assert fields(edgpu.aac_config_parse(sdp(HBR_FMTP), 1)) == (edgpu.AAC_HBR, 0, 2, 4, 2, 0)
    assert fields(edgpu.aac_config_parse(sdp(HBR_FMTP.replace("1210", "1190")), 1)) == (edgpu.AAC_HBR, 0, 2, 3, 2, 0)
    assert fields(edgpu.aac_config_parse(sdp(HBR_FMTP.upper().replace("AAC-HBR", "aac-HBR")), 1)) == (edgpu.AAC_HBR, 0, 2, 4, 2, 0)
    assert fields(edgpu.aac_config_parse(sdp(HBR_FMTP.lower()), 1)) == (edgpu.AAC_HBR, 0, 2, 4, 2, 0)
    lbr = "mode=AAC-lbr;config=1208;sizelength=6;indexlength=2;indexdeltalength=2;constantduration=1024"
    assert fields(edgpu.aac_config_parse(sdp(lbr), 1)) == (edgpu.AAC_LBR, 0, 2, 4, 1, 0)
    # the track-th section's line, with or without a video section before it; a longer config is fine
    two = sdp(HBR_FMTP, lbr.replace("1208", "11885600"), video_first=False)
    assert fields(edgpu.aac_config_parse(two, 0))[:1] == (edgpu.AAC_HBR,)
    assert fields(edgpu.aac_config_parse(two, 1)) == (edgpu.AAC_LBR, 0, 2, 3, 1, 0)
    assert fields(edgpu.aac_config_parse(two.replace("\r\n", "\n"), 1, framing=edgpu.AAC_RAW, frame_samples=960)) == \
        (edgpu.AAC_LBR, edgpu.AAC_RAW, 2, 3, 1, 960)
    zero = HBR_FMTP + "; auxiliarydatasizelength=0; CTSDeltaLength=0; dtsdeltalength=0; randomaccessindication=0; streamstateindication=0"
    assert fields(edgpu.aac_config_parse(sdp(zero), 1)) == (edgpu.AAC_HBR, 0, 2, 4, 2, 0)


REFUSED = {
    "another mode": HBR_FMTP.replace("AAC-hbr", "CELP-vbr"),
    "no mode": HBR_FMTP.replace("mode=AAC-hbr; ", ""),
    "hbr with lbr lengths": "mode=AAC-hbr;config=1210;sizelength=6;indexlength=2;indexdeltalength=2",
    "lbr with hbr lengths": "mode=AAC-lbr;config=1210;sizelength=13;indexlength=3;indexdeltalength=3",
    "sizelength 12": HBR_FMTP.replace("SizeLength=13", "SizeLength=12"),
    "indexlength 2": HBR_FMTP.replace("IndexLength=3", "IndexLength=2"),
    "indexdeltalength missing": HBR_FMTP.replace("; IndexDeltaLength=3", ""),
    "auxiliarydatasizelength": HBR_FMTP + "; auxiliarydatasizelength=8",
    "ctsdeltalength": HBR_FMTP + "; CTSDeltaLength=16",
    "dtsdeltalength": HBR_FMTP + "; DTSDeltaLength=16",
    "randomaccessindication": HBR_FMTP + "; randomAccessIndication=1",
    "streamstateindication": HBR_FMTP + "; streamStateIndication=4",
    "config of one byte": HBR_FMTP.replace("config=1210", "config=12"),
    "no config": HBR_FMTP.replace(" config=1210;", ""),
    "config not hex": HBR_FMTP.replace("config=1210", "config=12g0"),
    "object type 0": HBR_FMTP.replace("config=1210", "config=0210"),
    "object type 5": HBR_FMTP.replace("config=1210", "config=2A10"),
    "frequency index 13": HBR_FMTP.replace("config=1210", "config=1690"),
    "channels 0": HBR_FMTP.replace("config=1210", "config=1200"),
    "channels 8": HBR_FMTP.replace("config=1210", "config=1240"),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusals(name):
    with pytest.raises(edgpu.EdgpuError) as e:
        edgpu.aac_config_parse(sdp(REFUSED[name]), 1)
    assert e.value.code == edgpu.BAD_ARGUMENT


def test_no_such_section_or_no_fmtp_line():
    for text, track in ((sdp(HBR_FMTP), 2), (sdp(None), 1), ("", 0)):
        with pytest.raises(edgpu.EdgpuError) as e:
            edgpu.aac_config_parse(text, track)
        assert e.value.code == edgpu.BAD_ARGUMENT
