"""GPU: the transport-stream mux (edgpu_ts_mux, edgpu_ts.hip) byte for byte against tests/ts_model.py
-- packets, unit rows, state rows, totals -- with every output buffer pre-filled with a sentinel and
checked beyond result.bytes, and end to end through the tap against tests/ts_demux.py.

The shapes are the smallest at which the kernels can go wrong: every ES length 0..560 (the
single-packet edge, every stuffing remainder, every source byte phase against every destination
phase), PAT / PMT at every packet position of a 16-B run, 130 units in a stream (two scan rounds and
a bit), 300 streams (two blocks of the placement scan)."""
import numpy as np
import pytest

import ts_demux
import ts_model as tm
from easydarwin_amd import edgpu
from ts_model import KEY

pytestmark = pytest.mark.gpu

SENTINEL = 0xA7
SLACK = 4096
SMALL = dict(max_batch_packets=1 << 15, max_batch_bytes=32 << 20, out_arena_bytes=32 << 20, max_out_packets=1 << 16)


@pytest.fixture(scope="module")
def ctx():
    with edgpu.Context(**SMALL) as c:
        yield c


def es_unit(n, k=0, nal=0x41):
    body = bytes([0, 0, 0, 1, nal]) + bytes((k * 31 + 7 * j + 1) & 0xFF for j in range(max(n - 5, 0)))
    return body[:n]


def layout(per_stream):
    """[[(es bytes, rtp_ts, flags)]] -> (es bytes, unit rows, stream rows) laid out as a tap drain does:
    every stream from a 16-B aligned offset, its units one after the other."""
    es = bytearray()
    units = np.zeros(sum(len(s) for s in per_stream), dtype=edgpu.TAP_UNIT_DTYPE)
    streams = np.zeros(len(per_stream), dtype=edgpu.TAP_STREAM_DTYPE)
    k = 0
    for i, s in enumerate(per_stream):
        es += bytes(-len(es) % 16)
        streams[i]["session"], streams[i]["offset"], streams[i]["unit_first"], streams[i]["unit_count"] = i, len(es), k, len(s)
        for b, ts, fl in s:
            units[k]["offset"], units[k]["bytes"], units[k]["rtp_ts"], units[k]["flags"], units[k]["stream"] = \
                len(es), len(b), ts & 0xFFFFFFFF, fl, i
            es += b
            k += 1
        streams[i]["bytes"] = len(es) - int(streams[i]["offset"])
    return bytes(es), units, streams


def to_rows(states):
    a = np.zeros(len(states), dtype=edgpu.TS_STATE_DTYPE)
    for i, s in enumerate(states):
        for f in ("ext_ts", "started", "cc_pat", "cc_pmt", "cc_video"):
            a[i][f] = s[f]
    return a


def to_dicts(rows):
    return [{f: int(r[f]) for f in ("ext_ts", "started", "cc_pat", "cc_pmt", "cc_video")} for r in rows]


def gpu_mux(ctx, kw, es, units, streams, states, cap, es_kind="host", out_kind="host"):
    """-> (rc, result, the whole output buffer (cap + SLACK bytes), unit rows, state rows)."""
    cfg = edgpu.TsConfig(**kw) if kw is not None else None
    rows = to_rows(states)
    ts_units = np.zeros(len(units), dtype=edgpu.TS_UNIT_DTYPE)
    ts_units.view(np.uint8)[:] = SENTINEL
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
    rc, res = ctx.ts_mux_raw(cfg, es_ptr, len(es), ek, units, streams, rows, out_ptr, cap, ok, ts_units)
    got = ctx.copy_to_host(out_ptr, cap + SLACK) if out is None else np.array(out, copy=True)
    for b in keep:
        b.free()
    return rc, res, got, ts_units, rows


def check(ctx, kw, per_stream, states=None, what="", **kinds):
    """One call against the model; returns the new states (dicts)."""
    es, units, streams = layout(per_stream)
    states = [tm.new_state() for _ in per_stream] if states is None else states
    want_states = [dict(s) for s in states]
    want, want_rows, total = tm.mux(tm.Config(**kw) if kw is not None else None, es, units, streams, want_states)
    rc, res, got, rows, new = gpu_mux(ctx, kw, es, units, streams, states, total, **kinds)
    assert rc == edgpu.OK, f"{what}: status {rc}"
    assert (int(res.bytes), int(res.units), int(res.streams)) == (total, len(units), len(streams)), what
    if got[:total].tobytes() != want:
        g = got[:total].tobytes()
        first = next(i for i, (a, b) in enumerate(zip(g, want)) if a != b)
        raise AssertionError(f"{what}: bytes differ at {first} (packet {first // 188} byte {first % 188}) of {total}: "
                             f"{g[first - first % 4:first - first % 4 + 8].hex()} / {want[first - first % 4:first - first % 4 + 8].hex()}")
    assert np.all(got[total:] == SENTINEL), f"{what}: bytes written beyond result.bytes"
    for k, (r, w) in enumerate(zip(rows, want_rows)):
        assert {f: int(r[f]) for f in w} == w, f"{what}: unit row {k}"
        assert int(r["_pad"]) == 0
    assert to_dicts(new) == want_states, what
    return want_states


# ---- 1. lengths ----

@pytest.mark.parametrize("flags", [edgpu.TS_AUD, edgpu.TS_NOAUD])
def test_every_es_length(ctx, flags):
    lens = list(range(0, 561)) + [3000, 70000]
    units = [(es_unit(n, n, 0x09 if n % 5 == 2 else 0x41), 3000 * k, KEY if k % 37 == 3 else 0) for k, n in enumerate(lens)]
    check(ctx, dict(flags=flags), [units], what=f"flags {flags}")
    # the same lengths backwards: other source phases against the destination's
    check(ctx, dict(flags=flags), [units[::-1]], what=f"flags {flags} reversed")


# ---- 2. KEY placement ----

def test_key_placement(ctx):
    n, k = (lambda j: (es_unit(40 + j, j), 3000 * j, 0)), (lambda j: (es_unit(60 + j, j, 0x65), 3000 * j, KEY))
    per_stream = [
        [k(0), n(1), n(2), k(3), k(4), n(5)],               # first, consecutive
        [n(0), n(1), n(2)],                                 # absent
        [n(0), k(1)],                                       # last; PSI at packet 1 of the stream
        [n(0), n(1), k(2)],
        [n(0), n(1), n(2), k(3)],
        [k(0)],
    ]
    for lead in range(4):                                   # the PSI pairs at every packet position mod 4
        st = check(ctx, None, [[n(9)] * lead] + per_stream, what=f"lead {lead}")
    assert st[1]["cc_pat"] == 3 and st[2]["cc_pat"] == 0


# ---- 3. scan carries ----

def test_a_stream_of_130_units(ctx):
    units = [(es_unit(1 + (7 * j) % 400, j, 0x65 if j % 11 == 0 else 0x41), 1500 * j, KEY if j % 11 == 0 else 0) for j in range(130)]
    check(ctx, None, [units])


def test_300_streams(ctx):
    per_stream = []
    for i in range(300):
        cnt = (0, 1, 70)[i % 3]
        per_stream.append([(es_unit((13 * i + 29 * j) % 300, i + j, 0x65 if j % 9 == 0 else 0x41), 90000 * i + 3000 * j,
                            KEY if j % 9 == 0 else 0) for j in range(cnt)])
    per_stream[4] = [(b"", 3000 * j, KEY) for j in range(3)]                # only zero-byte units
    per_stream[299 - 1] = [(b"", 7, 0)]
    check(ctx, None, per_stream)


# ---- 4. state ----

def sequence():
    ts = [(1 << 32) - 7000, (1 << 32) - 4000, (1 << 32) - 1000, 2000, 5000, 3500, 8000, 8000, 11000]
    units = []
    for j, t in enumerate(ts * 3):
        n = [5, 170, 0, 700, 162, 156, 0, 3000, 346][j % 9]
        units.append((es_unit(n, j, 0x65 if j % 4 == 0 else 0x41), t + 9000 * (j // 9), KEY if j % 4 == 0 else 0))
    return units


def test_state_across_calls(ctx):
    kw = dict(pts_offset=(1 << 33) - (1 << 32) - 100, pcr_lead=45000, video_pid=0x41, pmt_pid=0x40, tsid=7, program=3)
    units = sequence()
    whole = check(ctx, kw, [units, units[3:]], what="whole")
    assert whole[0]["ext_ts"] > 1 << 32                         # the RTP timestamp wrapped inside the call
    es, u, s = layout([units])
    want, _, total = tm.mux(tm.Config(**kw), es, u, s, [tm.new_state()])
    assert total // 188 > 2 * 16                                # the counters wrap
    # split at every unit boundary, the state carried by the caller
    state = [tm.new_state(), tm.new_state()]
    for j, unit in enumerate(units):
        two = [[unit], [units[3 + j]] if 3 + j < len(units) else []]
        state = check(ctx, kw, two, states=state, what=f"unit {j}")
    assert state == whole


def test_one_call_equals_split_calls_on_the_gpu(ctx):
    kw = dict(flags=edgpu.TS_AUD)
    units = sequence()
    es, u, s = layout([units])
    total = len(tm.mux(tm.Config(**kw), es, u, s, [tm.new_state()])[0])
    rc, res, whole, rows, new = gpu_mux(ctx, kw, es, u, s, [tm.new_state()], total)
    assert rc == edgpu.OK and int(res.bytes) == total
    state, parts = [tm.new_state()], b""
    for unit in units:
        es1, u1, s1 = layout([[unit]])
        rc, r1, g1, _, st = gpu_mux(ctx, kw, es1, u1, s1, state, 4 * 188 + len(unit[0]) * 2)
        assert rc == edgpu.OK
        parts += g1[:int(r1.bytes)].tobytes()
        state = to_dicts(st)
    assert parts == whole[:total].tobytes() and state == to_dicts(new)


# ---- 5. overflow ----

def test_overflow_writes_nothing(ctx):
    per_stream = [[(es_unit(500, 1, 0x65), 1000, KEY), (es_unit(30, 2), 4000, 0)], [(es_unit(200, 3), 9, 0)]]
    es, units, streams = layout(per_stream)
    states = [tm.new_state(), dict(ext_ts=5, started=1, cc_pat=2, cc_pmt=9, cc_video=14)]
    want, _, total = tm.mux(None, es, units, streams, [dict(s) for s in states])
    for kinds in (dict(), dict(es_kind="device", out_kind="device")):
        rc, res, got, rows, new = gpu_mux(ctx, None, es, units, streams, states, total - 188, **kinds)
        assert rc == edgpu.OUT_OVERFLOW
        assert (int(res.bytes), int(res.units), int(res.streams)) == (total, 3, 2)
        assert np.all(got == SENTINEL) and np.all(rows.view(np.uint8) == SENTINEL)
        assert to_dicts(new) == states
        check(ctx, None, per_stream, states=states, what="retry", **kinds)


# ---- 6. bad arguments ----

def test_bad_arguments(ctx):
    per_stream = [[(es_unit(50, 1), 1000, 0)], [(es_unit(20, 2), 9, 0)]]
    es, units, streams = layout(per_stream)
    states = [tm.new_state(), tm.new_state()]

    def rc_of(u=units, s=streams, kw=None, n=len(es)):
        rc, res, got, rows, new = gpu_mux(ctx, kw, es[:n], u, s, states, 4096)
        if rc != edgpu.OK:
            assert np.all(got == SENTINEL) and np.all(rows.view(np.uint8) == SENTINEL) and to_dicts(new) == states
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
    assert rc_of(kw=dict(video_pid=0x2000)) == edgpu.BAD_ARGUMENT
    assert rc_of(kw=dict(video_pid=0x30, pmt_pid=0x30)) == edgpu.BAD_ARGUMENT
    assert rc_of(kw=dict(flags=4)) == edgpu.BAD_ARGUMENT


# ---- 7. pointer kinds ----

@pytest.mark.parametrize("es_kind,out_kind", [("host", "host"), ("device", "device"), ("pinned", "device"), ("device", "pinned")])
def test_pointer_kinds(ctx, es_kind, out_kind):
    per_stream = [[(es_unit(1 + (53 * j) % 900, j, 0x65 if j % 5 == 0 else 0x41), 3000 * j, KEY if j % 5 == 0 else 0) for j in range(40)],
                  [], [(es_unit(300000, 5), 77, KEY)]]      # 300 kB: past the 256-KiB threshold of the reads into pinned memory
    st = check(ctx, None, per_stream, what="first", es_kind=es_kind, out_kind=out_kind)
    check(ctx, None, per_stream, states=st, what="second", es_kind=es_kind, out_kind=out_kind)


# ---- 8. end to end through the tap ----

class DrainContext(edgpu.Context):
    """Every H.264 track tapped at session add; every tap drained before each fan-out, as Annex-B
    units (ts=False) or as a transport stream (ts=True)."""

    def __init__(self, ts, **cfg):
        super().__init__(**cfg)
        self.ts, self.tapped, self.got = ts, 0, {}

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
        if self.ts:
            data, units, streams = self.tap_drain_ts(flush=flush)
        else:
            data, units, streams = self.tap_drain(flush=flush)
        for st in streams:
            key = (int(st["session"]), int(st["track"]))
            for u in units[int(st["unit_first"]):int(st["unit_first"]) + int(st["unit_count"])]:
                b = data[int(u["offset"]):int(u["offset"]) + int(u["bytes"])].tobytes()
                self.got.setdefault(key, []).append((b, int(u["pts"]) if self.ts else int(u["rtp_ts"]), int(u["flags"])))

    def fanout(self, now_ms):
        self.drain()
        return super().fanout(now_ms)


def test_hls_segment_tool(tmp_path):
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "hls_segment.py"), "--sessions", "2", "--seconds", "3",
                          "--segment", "1", "--out", str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    report = json.loads(out.stdout.strip().split("\n")[-1])
    assert len(report["streams"]) == 2 and report["units"] > 0
    for name, row in report["streams"].items():
        lines = open(tmp_path / name / "index.m3u8").read().split("\n")
        assert lines[:2] == ["#EXTM3U", "#EXT-X-VERSION:3"] and lines[-2] == "#EXT-X-ENDLIST"
        segs = [l for l in lines if l.endswith(".ts")]
        assert len(segs) == row["segments"] >= 2
        cc = {}
        for s in segs:
            d = ts_demux.demux(open(tmp_path / name / s, "rb").read(), cc)    # continuity runs through the segments
            assert d["pes"][0]["packet"] == 2 and d["pes"][0]["rai"] and d["stream_type"] == 0x1B
            assert d["pes"][0]["payload"][:6] == b"\x00\x00\x00\x01\x09\xF0"


@pytest.mark.parametrize("name", ["mixed", "leave"])
def test_goldens_through_tap_and_mux(name):
    from easydarwin_amd.replay import replay
    from scenarios import SCENARIOS
    from test_gpu_tap import replay_cfg
    trace = SCENARIOS[name]()
    with DrainContext(False, **replay_cfg(trace)) as c:
        replay(trace, ctx=c)
        c.drain(flush=True)
        plain = c.got
        assert c.tapped and plain and c.kernel_times(6) == []   # the mux never ran: nothing recorded
    with DrainContext(True, **replay_cfg(trace)) as c:
        replay(trace, ctx=c)
        c.drain(flush=True)
        muxed = c.got
        assert c.kernel_times(6)
    assert sorted(plain) == sorted(muxed)
    n_pes = 0
    for key, units in plain.items():
        rows = muxed[key]
        assert len(rows) == len(units)
        d = ts_demux.demux(b"".join(r[0] for r in rows))
        with_es = [(u, r) for u, r in zip(units, rows) if u[0]]
        assert len(d["pes"]) == len(with_es) and d["pat"] == d["pmt"] == sum(1 for u, _ in with_es if u[2] & KEY)
        for e, (u, r) in zip(d["pes"], with_es):
            aud = b"" if len(u[0]) >= 5 and u[0][4] & 0x1F == 9 else b"\x00\x00\x00\x01\x09\xF0"
            assert e["payload"] == aud + u[0]
            assert e["pts"] == r[1] and e["rai"] == bool(u[2] & KEY) and r[2] == u[2]
        for (u0, r0), (u1, r1) in zip(zip(units, rows), zip(units[1:], rows[1:])):
            d32 = (u1[1] - u0[1]) & 0xFFFFFFFF
            assert (r1[1] - r0[1]) % (1 << 33) == (d32 - (1 << 32) if d32 >> 31 else d32) % (1 << 33)
        n_pes += len(d["pes"])
    assert n_pes
