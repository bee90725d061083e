"""CPU: the edgpu_stream_stats record's ctypes / numpy mirrors agree with the C header."""
import ctypes
import os
import subprocess

from easydarwin_amd import edgpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_stats_layout_matches_c(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "edgpu.h"
int main(void) {
  printf("%zu %zu %zu %zu\n", sizeof(edgpu_stream_stats), offsetof(edgpu_stream_stats, lost),
         offsetof(edgpu_stream_stats, sr_ntp), offsetof(edgpu_stream_stats, last_sample_ms));
  return 0;
}''')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = edgpu.StreamStats
    assert got == [ctypes.sizeof(S), S.lost.offset, S.sr_ntp.offset, S.last_sample_ms.offset]
    d = edgpu.STREAM_STATS_DTYPE
    assert got == [d.itemsize, d.fields["lost"][1], d.fields["sr_ntp"][1], d.fields["last_sample_ms"][1]]
    assert [n for n, _ in S._fields_] == list(d.names)


def test_stats_entry_points_are_bound():
    lib = edgpu.load()
    for name in ("edgpu_stream_stats_enable", "edgpu_stream_stats_disable", "edgpu_stream_stats_sample",
                 "edgpu_stream_stats_get", "edgpu_session_bitrate"):
        assert name in edgpu.EXPORTED and getattr(lib, name).argtypes
    for m in ("stream_stats_enable", "stream_stats_disable", "stream_stats_sample", "stream_stats", "session_bitrate"):
        assert callable(getattr(edgpu.Context, m))
