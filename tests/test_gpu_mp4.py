"""GPU: the fragmented-MP4 mux (edgpu_mp4_mux, edgpu_mp4.hip) byte for byte against tests/mp4_model.py
-- output, sample rows, fragment rows, state rows, totals -- with the output pre-filled with a
sentinel that must survive everywhere outside the streams' runs, and end to end through the tap
against tests/mp4_demux.py.

The shapes are the smallest at which the kernels can go wrong: every ES length 0..600 (every source
phase against every destination phase, head and tail paths), a start code at every position mod 16
at every source phase, one 70-KiB NAL (its length crosses 35 chunks of the start-code search), 300
tiny NALs, 130 units in a stream (two plan rounds and a bit), 300 streams (two placement blocks)."""
import numpy as np
import pytest

import mp4_demux
import mp4_model as mm
from easydarwin_amd import edgpu
from mp4_model import KEY
from test_gpu_ts import SMALL, es_unit, layout

pytestmark = pytest.mark.gpu

SENTINEL = 0xA7
SLACK = 4096
SC = b"\x00\x00\x00\x01"
STATE_FIELDS = ("ext_ts", "origin", "sequence", "last_step", "started")


@pytest.fixture(scope="module")
def ctx():
    with edgpu.Context(**SMALL) as c:
        yield c


def to_rows(states):
    a = np.zeros(len(states), dtype=edgpu.MP4_STATE_DTYPE)
    for i, s in enumerate(states):
        for f in STATE_FIELDS:
            a[i][f] = s[f]
    return a


def to_dicts(rows):
    return [{f: int(r[f]) for f in STATE_FIELDS} for r in rows]


def gpu_mux(ctx, kw, es, units, streams, states, cap, frag_cap=None, es_kind="host", out_kind="host"):
    """-> (rc, result, the whole output buffer (cap + SLACK bytes), sample rows, fragment rows, state rows)."""
    cfg = edgpu.Mp4Config(**kw) if kw is not None else None
    rows = to_rows(states)
    samples = np.zeros(len(units), dtype=edgpu.MP4_SAMPLE_DTYPE)
    samples.view(np.uint8)[:] = SENTINEL
    frags = np.zeros(len(units) + 2 if frag_cap is None else frag_cap + 2, dtype=edgpu.MP4_FRAG_DTYPE)
    frags.view(np.uint8)[:] = SENTINEL
    nf = len(frags) - 2
    keep = []
    esa = np.frombuffer(es, dtype=np.uint8)
    if es_kind == "host":
        es_ptr, ek = (esa.ctypes.data if len(esa) else 0), edgpu.PTR_HOST
    elif es_kind == "pinned":
        b = ctx.host_alloc(max(len(esa), 16))
        b.array[:len(esa)] = esa
        keep.append(b)
        es_ptr, ek = b.ptr, edgpu.PTR_PINNED
    else:
        b = ctx.device_alloc(max(len(esa), 16))
        ctx.copy_to_device(b.ptr, esa)
        keep.append(b)
        es_ptr, ek = b.ptr, edgpu.PTR_DEVICE
    fill = np.full(cap + SLACK, SENTINEL, dtype=np.uint8)
    if out_kind == "host":
        out, out_ptr, ok = fill, fill.ctypes.data, edgpu.PTR_HOST
    elif out_kind == "pinned":
        b = ctx.host_alloc(cap + SLACK)
        b.array[:] = SENTINEL
        keep.append(b)
        out, out_ptr, ok = b.array, b.ptr, edgpu.PTR_PINNED
    else:
        b = ctx.device_alloc(cap + SLACK)
        ctx.copy_to_device(b.ptr, fill)
        keep.append(b)
        out, out_ptr, ok = None, b.ptr, edgpu.PTR_DEVICE
    rc, res = ctx.mp4_mux_raw(cfg, es_ptr, len(es), ek, units, streams, rows, out_ptr, cap, ok, samples, frags[:nf])
    got = ctx.copy_to_host(out_ptr, cap + SLACK) if out is None else np.array(out, copy=True)
    for b in keep:
        b.free()
    assert np.all(frags[nf:].view(np.uint8) == SENTINEL), "fragment rows written beyond frag_cap"
    return rc, res, got, samples, frags[:nf], rows


def check(ctx, kw, per_stream, states=None, what="", laid=None, **kinds):
    """One call against the model; returns the new states (dicts)."""
    es, units, streams = laid if laid is not None else layout(per_stream)
    states = [mm.new_state() for _ in streams] if states is None else states
    want_states = [dict(s) for s in states]
    want, want_rows, want_frags, total = mm.mux(mm.Config(**kw) if kw is not None else None, es, units, streams,
                                               want_states, fill=SENTINEL)
    rc, res, got, rows, frags, new = gpu_mux(ctx, kw, es, units, streams, states, total, **kinds)
    assert rc == edgpu.OK, f"{what}: status {rc}"
    assert (int(res.bytes), int(res.units), int(res.frags), int(res.streams)) == (total, len(units), len(want_frags), len(streams)), what
    g = got[:total].tobytes()
    if g != want:                                           # the model fills the gaps between runs with the sentinel
        first = next(i for i, (a, b) in enumerate(zip(g, want)) if a != b)
        raise AssertionError(f"{what}: bytes differ at {first} of {total}: "
                             f"{g[max(first - 8, 0):first + 8].hex()} / {want[max(first - 8, 0):first + 8].hex()}")
    assert np.all(got[total:] == SENTINEL), f"{what}: bytes written beyond result.bytes"
    for k, (r, w) in enumerate(zip(rows, want_rows)):
        assert {f: int(r[f]) for f in w} == w, f"{what}: sample row {k}"
    for k, w in enumerate(want_frags):
        assert {f: int(frags[k][f]) for f in w} == w, f"{what}: fragment row {k}"
    assert np.all(frags[len(want_frags):].view(np.uint8) == SENTINEL), f"{what}: fragment rows beyond result.frags"
    assert to_dicts(new) == want_states, what
    return want_states


# ---- 1. lengths and phases ----

def test_every_es_length(ctx):
    units = [(es_unit(n, n), 3000 * k, KEY if k % 37 == 3 else 0) for k, n in enumerate(range(0, 601))]
    check(ctx, None, [units], what="ascending")
    check(ctx, None, [units[::-1]], what="descending")      # other source phases against the destination's


def test_start_code_at_every_phase(ctx):
    units = []
    for phase in range(16):                                 # the unit's own source phase
        for p in range(16):                                 # the second start code's position mod 16 in the unit
            body = SC + bytes([0x41]) + bytes(((7 * j + p + 1) & 0xFF) | 1 for j in range(27 + p)) + SC + bytes([0x41]) + \
                bytes(((5 * j + 3) & 0xFF) | 1 for j in range(40))
            units.append((body, 3000 * len(units), 0))
        units.append((SC + bytes([0x41]) + bytes([0x55] * ((phase * 15 + 1) % 16 + 11)), 3000 * len(units), 0))
    check(ctx, None, [units], what="phases")


def nal_units():
    big = SC + bytes([0x65]) + bytes(((j * 7) % 251) + 1 for j in range(70 * 1024))        # no zero byte: one NAL
    tiny = b"".join(SC + bytes([0x41]) + bytes([0x80 | (j & 0x7F)] * (j % 20)) for j in range(300))
    return [
        (big, 0, KEY),
        (tiny, 3000, 0),
        (SC + SC + SC + bytes([0x41, 9]), 6000, 0),         # back to back: lengths 0
        (SC, 9000, 0),                                      # only a start code
        (bytes([0x41, 1, 2, 3, 4, 5]) + SC + bytes([0x41, 7]), 12000, 0),  # no leading start code: DAMAGED
        (bytes([0x41, 0, 0, 1, 9]), 15000, 0),              # no start code at all, 00 00 01 is data
        (SC + bytes([0x41, 0, 0, 0, 0, 1, 0x42, 0, 0, 1, 3, 0, 0, 0]), 18000, 0),   # 00 00 00 00 01; trailing 00 00 00
        (SC + bytes([0x41, 5, 0, 0, 0]), 21000, 0),         # a start code cut by the unit's end ...
        (bytes([1, 0x41, 6, 6]), 24000, 0),                 # ... whose 01 is the next unit's first byte
        (big[:40000] + tiny + big[:3000], 27000, 0),
    ]


def test_nal_lengths(ctx):
    u = nal_units()
    st = check(ctx, None, [u], what="nal lengths")
    check(ctx, None, [u[::-1]], states=st, what="nal lengths reversed")


# ---- 2. the plan's rounds, keys, max_samples ----

@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 129, 130])
def test_units_per_stream_and_keys(ctx, n):
    for keys in ({0}, {63}, {64}, {n - 1}, {0, 63, 64, n - 1}, set()):
        units = [(es_unit(5 + (j * 13) % 90, j, 0x65 if j in keys else 0x41) if j % 11 != 5 else b"",
                  1000 + 2970 * j + (j % 3), KEY if j in keys else 0) for j in range(n)]
        check(ctx, None, [units], what=f"{n} units, keys {sorted(keys)}")


@pytest.mark.parametrize("max_samples", [1, 63, 64, 65])
def test_max_samples(ctx, max_samples):
    units = [(es_unit(6 + (j * 7) % 50, j), 3000 * j, KEY if j in (70, 71, 140) else 0) for j in range(200)]
    check(ctx, dict(max_samples=max_samples), [units], what=f"max_samples {max_samples}")
    check(ctx, dict(max_samples=max_samples, default_duration=1500, time_offset=(1 << 40) + 5), [units[:3], units[3:]],
          what=f"max_samples {max_samples}, two streams")


def test_time_rules(ctx):
    step = (1 << 31) - 1
    units = [(es_unit(20, 1), 5000, KEY), (es_unit(21, 2), 2000, 0),                  # a step back: duration 0
             (b"", 2000 + step, 0), (b"", (2000 + 2 * step) & 0xFFFFFFFF, 0), (b"", (2000 + 3 * step) & 0xFFFFFFFF, 0),
             (es_unit(22, 3), (2000 + 3 * step + 10) & 0xFFFFFFFF, 0),               # above 2^32 - 1: clamped
             (es_unit(23, 4), (2000 + 3 * step + 10 + 1234) & 0xFFFFFFFF, 0)]
    st = check(ctx, None, [units], what="clamps")
    assert st[0]["last_step"] == 1234
    st = check(ctx, None, [[(es_unit(9, 5), units[-1][1] + 1234, 0)]], states=st, what="last_step carried")
    st = check(ctx, None, [[(b"", 1, 0), (b"", 2, 0)]], states=st, what="no samples")
    check(ctx, dict(default_duration=77), [[(es_unit(9, 6), 0xFFFFFFF0, 0)], [(es_unit(9, 7), 5, 0), (es_unit(9, 7), 5, 0)]],
          what="defaulted")


# ---- 3. many streams ----

def test_many_streams(ctx):
    per_stream = [[(es_unit(1 + (s * 29 + j * 11) % 70, s + j), 90000 + 3000 * j, KEY if (s + j) % 4 == 0 else 0)
                   for j in range((s * 7) % 4)] for s in range(300)]
    st = check(ctx, None, per_stream, what="300 streams")
    check(ctx, dict(max_samples=2), per_stream, states=st, what="300 streams again")


def test_units_no_row_covers(ctx):
    es, units, streams = layout([[(es_unit(40, 1), 0, KEY)], [(es_unit(30, 2), 0, 0), (es_unit(31, 3), 9, 0)], [(es_unit(17, 4), 0, 0)]])
    streams[1]["unit_count"] = 1                            # unit 2 is no stream's
    check(ctx, None, None, laid=(es, units, streams), what="uncovered unit")


# ---- 4. state across calls ----

def test_split_calls(ctx):
    units = [(es_unit(30 + (j * 17) % 300, j, 0x65 if j % 25 == 0 else 0x41) if j % 13 != 7 else b"", 3000 * j, KEY if j % 25 == 0 else 0)
             for j in range(150)]
    other = [(es_unit(12, j), 100 * j, 0) for j in range(150)]
    cuts = [0, 1, 50, 64, 65, 149, 150]
    states = None
    for a, b in zip(cuts, cuts[1:]):                        # a sequence of calls equals the model's
        states = check(ctx, None, None, laid=layout([units[a:b], other[a:b]]), states=states, what=f"units {a}..{b}")

    def run(parts):                                         # one call against split calls, both on the GPU, through the demuxer
        st, es, tf = [mm.new_state(), mm.new_state()], b"", {}
        for a, b in parts:
            laid = layout([units[a:b], other[a:b]])
            want_states = [dict(s) for s in st]
            total = mm.mux(None, *laid, want_states)[3]
            rc, res, got, rows, frags, new = gpu_mux(ctx, None, *laid, st, total)
            assert rc == edgpu.OK
            st = to_dicts(new)
            for f in frags[:res.frags]:
                if int(f["stream"]) != 0:
                    continue
                blob = got[int(f["offset"]):int(f["offset"]) + int(f["bytes"])].tobytes()
                (d,) = mp4_demux.fragments(blob)
                es += b"".join(s[3] for s in d["samples"])
                if int(f["flags"]) & KEY:
                    tf[a + int(f["unit_first"])] = d["tfdt"]
        return es, tf
    one_es, one_tf = run([(0, 150)])
    split_es, split_tf = run(list(zip(cuts, cuts[1:])))
    assert one_es == split_es == b"".join(u[0] for u in units)
    assert one_tf == split_tf and len(one_tf) == 6


# ---- 5. overflow ----

@pytest.mark.parametrize("kinds", [dict(), dict(es_kind="device", out_kind="device")])
def test_overflow_writes_nothing(ctx, kinds):
    per_stream = [[(es_unit(100 + j, j), 3000 * j, KEY if j % 4 == 0 else 0) for j in range(10)], [(es_unit(50, 3), 7, 0)]]
    es, units, streams = layout(per_stream)
    states = [mm.new_state(), mm.new_state()]
    _, _, want_frags, total = mm.mux(None, es, units, streams, [dict(s) for s in states])
    for cap, frag_cap in ((total - 1, None), (0, None), (total, len(want_frags) - 1), (total, 0)):
        rc, res, got, rows, frags, new = gpu_mux(ctx, None, es, units, streams, states, cap, frag_cap=frag_cap, **kinds)
        assert rc == edgpu.OUT_OVERFLOW
        assert (int(res.bytes), int(res.units), int(res.frags), int(res.streams)) == (total, len(units), len(want_frags), 2)
        assert np.all(got == SENTINEL) and np.all(rows.view(np.uint8) == SENTINEL) and np.all(frags.view(np.uint8) == SENTINEL)
        assert to_dicts(new) == states
        check(ctx, None, per_stream, states=states, what="retry", **kinds)


# ---- 6. bad arguments ----

def test_bad_arguments(ctx):
    per_stream = [[(es_unit(50, 1), 1000, 0)], [(es_unit(20, 2), 9, 0)]]
    es, units, streams = layout(per_stream)
    states = [mm.new_state(), mm.new_state()]

    def rc_of(u=units, s=streams, kw=None, n=len(es)):
        rc, res, got, rows, frags, new = gpu_mux(ctx, kw, es[:n], u, s, states, 4096)
        if rc != edgpu.OK:
            assert np.all(got == SENTINEL) and np.all(rows.view(np.uint8) == SENTINEL) and to_dicts(new) == states
            assert np.all(frags.view(np.uint8) == SENTINEL)
        return rc

    assert rc_of() == edgpu.OK
    assert rc_of(n=len(es) - 1) == edgpu.BAD_ARGUMENT               # the last unit reaches past es_bytes
    u = units.copy()
    u[0]["offset"] = (1 << 40)
    assert rc_of(u=u) == edgpu.BAD_ARGUMENT
    u = units.copy()
    u[1]["stream"] = 2
    assert rc_of(u=u) == edgpu.BAD_ARGUMENT
    s = streams.copy()
    s[1]["unit_count"] = 2
    assert rc_of(s=s) == edgpu.BAD_ARGUMENT
    s = streams.copy()
    s[1]["unit_first"] = 0xFFFFFFFF
    assert rc_of(s=s) == edgpu.BAD_ARGUMENT
    s = streams.copy()
    s[1]["unit_first"], s[1]["unit_count"] = 0, 1                   # the ranges do not ascend
    s[0]["unit_first"] = 1
    assert rc_of(s=s) == edgpu.BAD_ARGUMENT
    assert rc_of(kw=dict(flags=1)) == edgpu.BAD_ARGUMENT


# ---- 7. pointer kinds ----

@pytest.mark.parametrize("es_kind,out_kind", [("host", "host"), ("device", "device"), ("pinned", "device"), ("device", "pinned")])
def test_pointer_kinds(ctx, es_kind, out_kind):
    per_stream = [[(es_unit(1 + (53 * j) % 900, j, 0x65 if j % 5 == 0 else 0x41), 3000 * j, KEY if j % 5 == 0 else 0) for j in range(40)],
                  [], [(es_unit(300000, 5), 77, KEY)]]      # 300 kB: past the 256-KiB threshold of the reads into pinned memory
    st = check(ctx, None, per_stream, what="first", es_kind=es_kind, out_kind=out_kind)
    check(ctx, None, per_stream, states=st, what="second", es_kind=es_kind, out_kind=out_kind)


# ---- 8. end to end through the tap ----

class Mp4DrainContext(edgpu.Context):
    """Every H.264 track tapped at session add; every tap drained before each fan-out, as Annex-B
    units (mp4=False) or as movie fragments (mp4=True), which the demuxer turns back into Annex-B."""

    def __init__(self, mp4, **cfg):
        super().__init__(**cfg)
        self.mp4, self.tapped, self.got, self.frag_seq = mp4, 0, {}, {}

    def session_add(self, sdp, udp_push=False):
        s = super().session_add(sdp, udp_push=udp_push)
        for t in range(self.session_tracks(s)):
            try:
                self.tap_enable(s, t)
                self.tapped += 1
            except edgpu.EdgpuError as e:
                assert e.code == edgpu.BAD_ARGUMENT
        return s

    def drain(self, flush=False):
        if not self.mp4:
            data, units, streams = self.tap_drain(flush=flush)
            for st in streams:
                key = (int(st["session"]), int(st["track"]))
                for u in units[int(st["unit_first"]):int(st["unit_first"]) + int(st["unit_count"])]:
                    if int(u["bytes"]):
                        self.got.setdefault(key, []).append(data[int(u["offset"]):int(u["offset"]) + int(u["bytes"])].tobytes())
            return
        data, samples, frags, units, streams = self.tap_drain_mp4(flush=flush)
        for f in frags:
            st = streams[int(f["stream"])]
            key = (int(st["session"]), int(st["track"]))
            (d,) = mp4_demux.fragments(data[int(f["offset"]):int(f["offset"]) + int(f["bytes"])].tobytes())
            assert d["sequence"] == int(f["sequence"]) == self.frag_seq.get(key, 0) + 1 and d["tfdt"] == int(f["tfdt"])
            self.frag_seq[key] = d["sequence"]
            assert bool(d["samples"][0][1] == 0x02000000) == bool(int(f["flags"]) & KEY)
            self.got.setdefault(key, []).extend(s[3] for s in d["samples"])

    def fanout(self, now_ms):
        self.drain()
        return super().fanout(now_ms)


@pytest.mark.parametrize("name", ["mixed", "leave"])
def test_goldens_through_tap_and_mux(name):
    from easydarwin_amd.replay import replay
    from scenarios import SCENARIOS
    from test_gpu_tap import replay_cfg
    trace = SCENARIOS[name]()
    with Mp4DrainContext(False, **replay_cfg(trace)) as c:
        replay(trace, ctx=c)
        c.drain(flush=True)
        plain = c.got
        assert c.tapped and plain and c.kernel_times(7) == []   # the mux never ran: nothing recorded
    with Mp4DrainContext(True, **replay_cfg(trace)) as c:
        replay(trace, ctx=c)
        c.drain(flush=True)
        muxed = c.got
        assert c.kernel_times(7)
    assert plain == muxed


def test_tools_on_a_golden(tmp_path):
    """tools/hls_segment.py --fmp4 and tools/tap_record.py --mp4 on the pushes of `mixed`: every file demuxes."""
    import json
    import os
    import subprocess
    import sys
    from scenarios import SCENARIOS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    trace = tmp_path / "mixed.edtr"
    trace.write_bytes(SCENARIOS["mixed"]().to_bytes())

    def tool(name, *args):
        out = subprocess.run([sys.executable, os.path.join(root, "tools", name), "--trace", str(trace), "--tick-ms", "50", *args],
                             capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        return json.loads(out.stdout.strip().split("\n")[-1])

    hls_dir, rec_dir = tmp_path / "hls", tmp_path / "rec"
    report = tool("hls_segment.py", "--fmp4", "--segment", "0.2", "--out", str(hls_dir))
    assert report["streams"] and report["units"] > 0
    for name, row in report["streams"].items():
        d = hls_dir / name
        mp4_demux.init_segment(open(d / "init.mp4", "rb").read())
        lines = open(d / "index.m3u8").read().split("\n")
        assert lines[1] == "#EXT-X-VERSION:7" and '#EXT-X-MAP:URI="init.mp4"' in lines and lines[-2] == "#EXT-X-ENDLIST"
        segs = [l for l in lines if l.endswith(".m4s")]
        assert len(segs) == row["segments"] >= 1
        seq = 0
        for s in segs:
            frags = mp4_demux.fragments(open(d / s, "rb").read())
            assert frags and frags[0]["samples"][0][1] == 0x02000000
            for f in frags:
                assert f["sequence"] > seq
                seq = f["sequence"]
    report = tool("tap_record.py", "--mp4", "--segment", "0.2", "--out", str(rec_dir))
    assert report["files"] >= 1 and report["units"] > 0
    for row in report["streams"].values():
        for name in row["files"]:
            data = open(rec_dir / name, "rb").read()
            top = mp4_demux.boxes(data)
            mp4_demux.init_segment(data[:top[1][2]])
            frags = mp4_demux.fragments(data[top[1][2]:])
            assert frags and frags[0]["samples"][0][1] == 0x02000000
