"""CPU: the transport-stream mux's records and constants agree between the C header, the ctypes /
numpy mirrors and tests/ts_model.py, and the entry point is declared and bound."""
import ctypes
import os
import re
import subprocess

from easydarwin_amd import edgpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = [("edgpu_ts_config", edgpu.TsConfig), ("edgpu_ts_state", edgpu.TsState), ("edgpu_ts_unit", edgpu.TsUnit),
           ("edgpu_ts_result", edgpu.TsResult)]


def test_ts_layouts_match_c(tmp_path):
    lines = ['printf("%zu\\n", sizeof(' + c + "));" for c, _ in STRUCTS]
    lines += [f'printf("%zu\\n", offsetof({c}, {n}));' for c, t in STRUCTS for n, _ in t._fields_]
    lines += ['printf("%u %u %u\\n", EDGPU_TS_AUD, EDGPU_TS_NOAUD, EDGPU_TS_PACKET);']
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "edgpu.h"\nint main(void) {\n' + "\n".join(lines) +
                   "\nreturn 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert [int(v) for v in out[:4]] == [ctypes.sizeof(t) for _, t in STRUCTS] == [24, 16, 32, 16]
    offs = [int(v) for v in out[4:4 + sum(len(t._fields_) for _, t in STRUCTS)]]
    assert offs == [getattr(t, n).offset for _, t in STRUCTS for n, _ in t._fields_]
    U, S = edgpu.TS_UNIT_DTYPE, edgpu.TS_STATE_DTYPE
    assert [U.fields[n][1] for n in U.names] == [getattr(edgpu.TsUnit, n).offset for n, _ in edgpu.TsUnit._fields_]
    assert [S.fields[n][1] for n in S.names] == [getattr(edgpu.TsState, n).offset for n, _ in edgpu.TsState._fields_]
    assert (U.itemsize, S.itemsize) == (32, 16)
    assert [int(v) for v in out[4 + len(offs)].split()] == [edgpu.TS_AUD, edgpu.TS_NOAUD, edgpu.TS_PACKET]


def test_model_constants_are_the_header_constants():
    import ts_model
    assert (ts_model.AUD, ts_model.NOAUD, ts_model.PACKET, ts_model.KEY) == (edgpu.TS_AUD, edgpu.TS_NOAUD, edgpu.TS_PACKET, edgpu.TAP_KEY)
    from easydarwin_amd import hls
    assert (hls.KEY, hls.DAMAGED) == (edgpu.TAP_KEY, edgpu.TAP_DAMAGED)


def test_ts_entry_point_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "edgpu.h")).read()
    lib = edgpu.load()
    assert re.search(r"\bint\s+edgpu_ts_mux\s*\(", header)
    assert "edgpu_ts_mux" in edgpu.EXPORTED and len(lib.edgpu_ts_mux.argtypes) == 15
    for m in ("ts_mux_raw", "tap_drain_ts"):
        assert callable(getattr(edgpu.Context, m))
    assert "TS muxing" not in header


def test_mux_rejects_bad_arguments_without_a_device():
    """The argument checks come before any device work: NULL context and result."""
    lib = edgpu.load()
    res = edgpu.TsResult()
    assert lib.edgpu_ts_mux(None, None, None, 0, 0, None, 0, None, 0, None, None, 0, 0, None, ctypes.byref(res)) == edgpu.BAD_ARGUMENT
