"""CPU: the tap's records (edgpu_tap_unit, edgpu_tap_stream) agree between the C header and the
ctypes / numpy mirrors, and the header declares the three entry points."""
import ctypes
import os
import re
import subprocess

from easydarwin_amd import edgpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tap_layouts_match_c(tmp_path):
    unit = [n for n, _ in edgpu.TapUnit._fields_]
    stream = [n for n, _ in edgpu.TapStream._fields_]
    lines = ['printf("%zu %zu %zu\\n", sizeof(edgpu_tap_unit), sizeof(edgpu_tap_stream), sizeof(edgpu_tap_result));']
    lines += [f'printf("%zu\\n", offsetof(edgpu_tap_unit, {n}));' for n in unit]
    lines += [f'printf("%zu\\n", offsetof(edgpu_tap_stream, {n}));' for n in stream]
    lines += ['printf("%u %u %u %u %u %u %u\\n", EDGPU_TAP_KEY, EDGPU_TAP_PARAMS, EDGPU_TAP_DAMAGED, EDGPU_TAP_NOMARKER, '
              'EDGPU_TAP_OPEN_END, EDGPU_TAP_FLUSH, EDGPU_TAP_ROUND);']
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "edgpu.h"\nint main(void) {\n' + "\n".join(lines) +
                   "\nreturn 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    sizes = [int(v) for v in out[0].split()]
    offs = [int(v) for v in out[1:1 + len(unit) + len(stream)]]
    U, S = edgpu.TAP_UNIT_DTYPE, edgpu.TAP_STREAM_DTYPE
    assert sizes == [ctypes.sizeof(edgpu.TapUnit), ctypes.sizeof(edgpu.TapStream), ctypes.sizeof(edgpu.TapResult)]
    assert sizes[:2] == [U.itemsize, S.itemsize]
    assert offs == [getattr(edgpu.TapUnit, n).offset for n in unit] + [getattr(edgpu.TapStream, n).offset for n in stream]
    assert offs == [U.fields[n][1] for n in unit] + [S.fields[n][1] for n in stream]
    assert list(U.names) == unit and list(S.names) == stream
    consts = [int(v) for v in out[1 + len(unit) + len(stream)].split()]
    assert consts == [edgpu.TAP_KEY, edgpu.TAP_PARAMS, edgpu.TAP_DAMAGED, edgpu.TAP_NOMARKER, edgpu.TAP_OPEN_END,
                      edgpu.TAP_FLUSH, edgpu.TAP_ROUND]


def test_model_flags_are_the_header_flags():
    import tap_model
    assert (tap_model.KEY, tap_model.PARAMS, tap_model.DAMAGED, tap_model.NOMARKER, tap_model.OPEN_END) == \
        (edgpu.TAP_KEY, edgpu.TAP_PARAMS, edgpu.TAP_DAMAGED, edgpu.TAP_NOMARKER, edgpu.TAP_OPEN_END)


def test_tap_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "edgpu.h")).read()
    lib = edgpu.load()
    for name in ("edgpu_tap_enable", "edgpu_tap_disable", "edgpu_tap_drain"):
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        assert name in edgpu.EXPORTED and getattr(lib, name).argtypes
    for m in ("tap_enable", "tap_disable", "tap_drain"):
        assert callable(getattr(edgpu.Context, m))
