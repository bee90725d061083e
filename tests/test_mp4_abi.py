"""CPU: the fragmented-MP4 part of the C ABI -- the records' layouts against C and the ctypes / numpy
mirrors, the entry points declared, exported and bound, NULL arguments refused before any device work."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from easydarwin_amd import edgpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "edgpu.h")

RECORDS = [("edgpu_mp4_config", edgpu.Mp4Config, None), ("edgpu_mp4_state", edgpu.Mp4State, edgpu.MP4_STATE_DTYPE),
           ("edgpu_mp4_sample", edgpu.Mp4Sample, edgpu.MP4_SAMPLE_DTYPE), ("edgpu_mp4_frag", edgpu.Mp4Frag, edgpu.MP4_FRAG_DTYPE),
           ("edgpu_mp4_result", edgpu.Mp4Result, None)]


def test_layouts_match_c(tmp_path):
    lines = []
    for cname, mirror, _ in RECORDS:
        fields = [f for f, _ in mirror._fields_]
        lines.append(f'printf("%zu", sizeof({cname}));')
        lines += [f'printf(" %zu", offsetof({cname}, {f}));' for f in fields]
        lines.append('printf("\\n");')
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
    assert [C.sizeof(m) for _, m, _ in RECORDS] == [24, 32, 32, 48, 24]


def test_declared_exported_and_bound():
    src = open(HEADER).read()
    declared = sorted(set(re.findall(r"\b(edgpu_[a-z0-9_]+)\s*\(", src)))
    assert sorted(edgpu.EXPORTED + edgpu.EXPORTED_MP4) == declared
    assert sorted(edgpu.EXPORTED_MP4) == ["edgpu_mp4_init", "edgpu_mp4_mux"]
    lib = edgpu.load()
    out = subprocess.run(["nm", "-D", "--defined-only", edgpu.LIB_PATH], capture_output=True, text=True).stdout
    for s in edgpu.EXPORTED_MP4:
        assert re.search(rf"\bT {s}$", out, re.M), s
    assert len(lib.edgpu_mp4_mux.argtypes) == 17 and len(lib.edgpu_mp4_init.argtypes) == 8
    assert "TS muxing" not in src and "MP4 muxing" not in src and "MP4 and fMP4" not in src


def test_null_arguments_are_refused_before_any_device_work():
    lib = edgpu.load()
    res = edgpu.Mp4Result()
    one = np.zeros(1, dtype=np.uint8)
    # no context: refused whatever else is passed (there is no device on this path)
    assert lib.edgpu_mp4_mux(None, None, None, 0, edgpu.PTR_HOST, None, 0, None, 0, None, None, 0, edgpu.PTR_HOST, None, None, 0,
                             C.byref(res)) == edgpu.BAD_ARGUMENT
    assert lib.edgpu_mp4_mux(None, None, one.ctypes.data, 1, edgpu.PTR_HOST, None, 0, None, 0, None, one.ctypes.data, 1,
                             edgpu.PTR_HOST, None, None, 0, None) == edgpu.BAD_ARGUMENT
    n = C.c_uint64()
    sps, pps = bytes([0x67, 66, 0, 30, 0xEC, 0x80]), bytes([0x68, 0xCE])
    assert lib.edgpu_mp4_init(None, 6, pps, 2, 0, one.ctypes.data, 1, C.byref(n)) == edgpu.BAD_ARGUMENT
    assert lib.edgpu_mp4_init(sps, 6, None, 2, 0, one.ctypes.data, 1, C.byref(n)) == edgpu.BAD_ARGUMENT
    assert lib.edgpu_mp4_init(sps, 6, pps, 2, 0, one.ctypes.data, 1, None) == edgpu.BAD_ARGUMENT
    assert lib.edgpu_mp4_init(sps, 6, pps, 2, 0, None, 1, C.byref(n)) == edgpu.BAD_ARGUMENT
