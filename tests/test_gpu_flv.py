"""GPU: the FLV mux (edgpu_flv_mux, edgpu_flv.hip) byte for byte against tests/flv_model.py -- output,
tag rows, state rows, totals -- with the output pre-filled with a sentinel that must survive
everywhere outside the streams' runs, and end to end through the tap and flv.Recorder against
tests/flv_demux.py.

The shapes are the smallest at which the kernels can go wrong: unit lengths 0..80 from every ES
offset mod 16 (every source phase against every destination phase and every tail of the funnelled
copy), 63 / 64 / 65 / 129 units in a stream (the plan's rounds), 255 / 256 / 257 streams (the
placement's blocks), start codes across a 32-byte lane and a 2-KiB chunk boundary, and one NAL of
130 KiB + 1 (past one 128-KiB step of the resolve kernel's search)."""
import numpy as np
import pytest

import flv_demux
import flv_model as fm
from easydarwin_amd import edgpu
from flv_model import KEY, PARAMS
from test_gpu_ts import SMALL, es_unit, layout

pytestmark = pytest.mark.gpu

SENTINEL = 0xA7
SLACK = 4096
SC = b"\x00\x00\x00\x01"
STATE_FIELDS = ("ext_ts", "origin", "started")


@pytest.fixture(scope="module")
def ctx():
    with edgpu.Context(**SMALL) as c:
        yield c


def to_rows(states):
    a = np.zeros(len(states), dtype=edgpu.FLV_STATE_DTYPE)
    for i, s in enumerate(states):
        for f in STATE_FIELDS:
            a[i][f] = s[f]
    return a


def to_dicts(rows):
    return [{f: int(r[f]) for f in STATE_FIELDS} for r in rows]


def gpu_mux(ctx, kw, es, units, streams, states, cap, es_kind="host", out_kind="host"):
    """-> (rc, result, the whole output buffer (cap + SLACK bytes), tag rows, state rows)."""
    cfg = edgpu.FlvConfig(**kw) if kw is not None else None
    rows = to_rows(states)
    tags = np.zeros(len(units), dtype=edgpu.FLV_TAG_DTYPE)
    tags.view(np.uint8)[:] = SENTINEL
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
    rc, res = ctx.flv_mux_raw(cfg, es_ptr, len(es), ek, units, streams, rows, out_ptr, cap, ok, tags)
    got = ctx.copy_to_host(out_ptr, cap + SLACK) if out is None else np.array(out, copy=True)
    for b in keep:
        b.free()
    return rc, res, got, tags, rows


def check(ctx, kw, per_stream, states=None, what="", laid=None, **kinds):
    """One call against the model; returns the new states (dicts)."""
    es, units, streams = laid if laid is not None else layout(per_stream)
    states = [fm.new_state() for _ in streams] if states is None else states
    want_states = [dict(s) for s in states]
    want, want_rows, total = fm.mux(fm.Config(**kw) if kw is not None else None, es, units, streams, want_states, fill=SENTINEL)
    rc, res, got, rows, new = gpu_mux(ctx, kw, es, units, streams, states, total, **kinds)
    assert rc == edgpu.OK, f"{what}: status {rc}"
    assert (int(res.bytes), int(res.units), int(res.streams)) == (total, len(units), len(streams)), what
    g = got[:total].tobytes()
    if g != want:                                           # the model fills the gaps between runs with the sentinel
        first = next(i for i, (a, b) in enumerate(zip(g, want)) if a != b)
        raise AssertionError(f"{what}: bytes differ at {first} of {total}: "
                             f"{g[max(first - 8, 0):first + 8].hex()} / {want[max(first - 8, 0):first + 8].hex()}")
    assert np.all(got[total:] == SENTINEL), f"{what}: bytes written beyond result.bytes"
    for k, (r, w) in enumerate(zip(rows, want_rows)):
        assert {f: int(r[f]) for f in w} == w, f"{what}: tag row {k}"
    assert to_dicts(new) == want_states, what
    return want_states


# ---- 1. lengths and phases ----

@pytest.mark.parametrize("group", range(4))
def test_every_length_at_every_phase(ctx, group):
    """Unit lengths 0..80 in one stream, the stream starting at every ES offset mod 16."""
    for phase in range(4 * group, 4 * group + 4):
        units = [(es_unit(n, n + phase), 3000 * k, KEY if k % 37 == 3 else 0) for k, n in enumerate(range(0, 81))]
        es, u, s = layout([units])
        u["offset"] += phase                                # the whole stream moved to this phase
        laid = (bytes(phase) + es, u, s)
        st = check(ctx, None, None, laid=laid, what=f"phase {phase}, ascending")
        es, u, s = layout([units[::-1]])
        u["offset"] += phase
        check(ctx, dict(time_offset=12345), None, laid=(bytes(phase) + es, u, s), states=st, what=f"phase {phase}, descending")


# ---- 2. the plan's rounds, the placement's blocks ----

@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_units_per_stream(ctx, n):
    units = [(es_unit(5 + (j * 13) % 90, j, 0x65 if j % 50 == 0 else 0x41) if j % 11 != 5 else b"",
              1000 + 2970 * j + (j % 3) - (9000 if j % 29 == 7 else 0), KEY if j % 50 == 0 else 0) for j in range(n)]
    st = check(ctx, None, [units], what=f"{n} units")
    check(ctx, dict(time_offset=(1 << 40) + 5), [units[:3], units[3:]], what=f"{n} units, two streams")
    check(ctx, None, [units], states=st, what=f"{n} units again")


@pytest.mark.parametrize("n", [255, 256, 257])
def test_many_streams(ctx, n):
    per_stream = [[(es_unit(1 + (s * 29 + j * 11) % 70, s + j), 90000 + 3000 * j, KEY if (s + j) % 4 == 0 else 0)
                   for j in range((s * 7) % 4)] for s in range(n)]
    assert not per_stream[0] and not per_stream[4] and per_stream[1]            # some rows are empty
    st = check(ctx, None, per_stream, what=f"{n} streams")
    check(ctx, None, per_stream + [[]], states=st + [fm.new_state()], what=f"{n} streams and an empty last row")


def test_units_no_row_covers(ctx):
    es, units, streams = layout([[(es_unit(40, 1), 0, KEY)], [(es_unit(30, 2), 0, 0), (es_unit(31, 3), 9, 0)], [(es_unit(17, 4), 0, 0)]])
    streams[1]["unit_count"] = 1                            # unit 2 is no stream's
    check(ctx, None, None, laid=(es, units, streams), what="uncovered unit")


# ---- 3. start codes and NAL sizes ----

def body(n, k=1):
    return bytes(((j * 7 + k) % 251) + 1 for j in range(n))    # no zero byte: holds no start code


def test_start_code_positions(ctx):
    # a second start code across the 32-byte lane boundary of the mark kernel and across the 2-KiB chunk boundary
    for at in (29, 30, 31, 32, 2045, 2046, 2047, 2048):
        check(ctx, None, [[(SC + b"\x41" + body(at - 5) + SC + b"\x41" + body(100), 0, 0)]], what=f"a start code at {at}")
    lead = [(b"", 0, 0)]
    special = [
        (SC + SC + b"\x41\x09", 0, 0),                      # two start codes 4 bytes apart
        (SC + b"\x41" + SC + SC + SC + b"\x41", 3000, 0),
        (SC + bytes([0x41, 5, 0, 0, 0]), 6000, 0),          # a start code cut by the unit's end ...
        (bytes([1, 0x41, 6, 6]), 9000, 0),                  # ... whose 01 is the next unit's first byte
        (bytes([0x41, 1, 2, 3, 4, 5]) + SC + bytes([0x41, 7]), 12000, 0),       # no leading start code
        (bytes([0x41, 0, 0, 1, 9]), 15000, 0),              # no start code at all; 00 00 01 is data
        (SC + bytes([0x41, 0, 0, 0, 0, 1, 0x42, 0, 0, 1, 3, 0, 0, 0]), 18000, 0),   # 00 00 00 00 01
        (SC, 21000, 0),
    ]
    st = check(ctx, None, [special + lead], what="special")
    check(ctx, None, [special[::-1]], states=st, what="special reversed")


def test_nal_sizes(ctx):
    k3 = SC + b"\x65" + body(3 * 1024 - 1)
    big = SC + b"\x65" + body(130 * 1024)                   # one NAL of 130 KiB + 1
    assert len(big) - 4 == 130 * 1024 + 1
    tiny = b"".join(SC + bytes([0x41]) + bytes([0x80 | (j & 0x7F)] * (j % 20)) for j in range(300))
    units = [(k3, 0, KEY), (big, 3000, KEY), (tiny, 6000, 0), (big[:40000] + tiny + k3, 9000, 0)]
    st = check(ctx, None, [units], what="nal sizes")
    check(ctx, None, [units[::-1], units], states=st + [fm.new_state()], what="nal sizes reversed")


def test_parameter_sets(ctx):
    def with_params(at):
        nals = [bytes([0x41, k + 1]) for k in range(at - 1)] + [bytes([0x67, 1, 2, 3, 4, 5]), bytes([0x68, 9, 8]), b"\x65" + body(50)]
        return b"".join(SC + n for n in nals)
    units = [(with_params(at), 3000 * at, KEY | PARAMS) for at in (1, 7, 8, 9)]
    units += [
        (with_params(1), 40000, KEY),                                                        # no PARAMS flag: not looked for
        (SC + bytes([0x67, 1]) + SC + bytes([0x67, 2, 2]) + SC + bytes([0x68, 3]) + SC + bytes([0x68]), 43000, PARAMS),
        (SC + SC + bytes([0x67, 7, 7]), 46000, PARAMS),                                      # a zero-length NAL
        (b"".join([SC] * 8) + bytes([0x67, 7, 7]), 49000, PARAMS),                           # the SPS is the eighth NAL
        (b"".join([SC] * 9) + bytes([0x67, 7, 7]), 52000, PARAMS),                           # ... the ninth
        (bytes([0x67, 1, 2]) + SC + bytes([0x68, 5]), 55000, PARAMS),                        # bytes before the first start code
        (SC + bytes([0x68, 5, 0, 0, 0]), 58000, PARAMS),                                     # ends in a cut start code
        (b"", 61000, PARAMS),
        (bytes([0x67, 1, 2]), 64000, PARAMS),                                                # no start code at all
        (bytes([0x67]) + body(5000) + SC + bytes([0x67, 4, 4]), 67000, PARAMS),              # the first start code is chunks away
        (SC + b"\x67" + body(140 * 1024) + SC + b"\x68" + body(7), 70000, PARAMS | KEY),     # a long hop
    ]
    es, u, s = layout([units])
    want = fm.mux(None, es, u, s, [fm.new_state()])[1]
    assert [(r["sps_bytes"], r["pps_bytes"]) for r in want[:4]] == [(6, 3), (6, 3), (6, 0), (0, 0)]
    assert (want[13]["sps_offset"], want[13]["sps_bytes"]) == (16 + 5001 + 4, 3) and want[14]["pps_bytes"] == 8
    st = check(ctx, None, [units], what="parameter sets")
    check(ctx, None, [units[::-1]], states=st, what="parameter sets reversed")


# ---- 4. state across calls ----

def test_split_calls(ctx):
    units = [(es_unit(30 + (j * 17) % 300, j, 0x65 if j % 25 == 0 else 0x41) if j % 13 != 7 else b"", 3000 * j, KEY if j % 25 == 0 else 0)
             for j in range(150)]
    other = [(es_unit(12, j), 100 * j, 0) for j in range(150)]

    def run(parts):
        st, data = [fm.new_state(), fm.new_state()], b""
        for a, b in parts:
            laid = layout([units[a:b], other[a:b]])
            want, rows, _ = fm.mux(fm.Config(time_offset=45), *laid, [dict(x) for x in st])
            data += want[:sum(int(r["bytes"]) for r in rows[:b - a])]          # the first stream's run
            st = check(ctx, dict(time_offset=45), None, laid=laid, states=st, what=f"units {a}..{b}")
        return data, st
    one, one_st = run([(0, 150)])
    split, split_st = run([(0, 64), (64, 65), (65, 150)])
    assert one_st == split_st and one == split
    assert flv_demux.annexb(n for t in flv_demux.tags(one) for n in t["nals"]) == b"".join(u[0] for u in units)


# ---- 5. overflow ----

@pytest.mark.parametrize("kinds", [dict(), dict(es_kind="device", out_kind="device")])
def test_overflow_writes_nothing(ctx, kinds):
    per_stream = [[(es_unit(100 + j, j), 3000 * j, KEY if j % 4 == 0 else 0) for j in range(10)], [(es_unit(50, 3), 7, 0)]]
    es, units, streams = layout(per_stream)
    states = [fm.new_state(), fm.new_state()]
    _, _, total = fm.mux(None, es, units, streams, [dict(s) for s in states])
    for cap in (total - 1, 0):
        rc, res, got, rows, new = gpu_mux(ctx, None, es, units, streams, states, cap, **kinds)
        assert rc == edgpu.OUT_OVERFLOW
        assert (int(res.bytes), int(res.units), int(res.streams)) == (total, len(units), 2)
        assert np.all(got == SENTINEL) and np.all(rows.view(np.uint8) == SENTINEL)
        assert to_dicts(new) == states
        check(ctx, None, per_stream, states=states, what="retry", **kinds)


# ---- 6. bad arguments ----

def test_bad_arguments(ctx):
    per_stream = [[(es_unit(50, 1), 1000, 0)], [(es_unit(20, 2), 9, 0)]]
    es, units, streams = layout(per_stream)
    states = [fm.new_state(), fm.new_state()]

    def rc_of(u=units, s=streams, kw=None, n=len(es), data=es):
        rc, res, got, rows, new = gpu_mux(ctx, kw, data[:n], u, s, states, 4096)
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
    s = streams.copy()
    s[1]["unit_first"], s[1]["unit_count"] = 0, 1                   # the ranges do not ascend
    s[0]["unit_first"] = 1
    assert rc_of(s=s) == edgpu.BAD_ARGUMENT
    assert rc_of(kw=dict(flags=1)) == edgpu.BAD_ARGUMENT
    # a unit of more than 0xFFFFFA bytes; 256 units of 0xFFFFFA in one row could reach 2^32 (the checks come before any copy,
    # so the ES is claimed, not held: the pointer kind is host and nothing reads it)
    huge = np.zeros(1 << 24, dtype=np.uint8)
    u, s = units[:1].copy(), streams[:1].copy()
    u[0]["offset"], u[0]["bytes"] = 0, fm.MAX_UNIT + 1
    assert fm.bad_argument(u, s) and rc_of(u=u, s=s, data=huge, n=len(huge)) == edgpu.BAD_ARGUMENT
    u = np.zeros(256, dtype=edgpu.TAP_UNIT_DTYPE)
    u["bytes"] = fm.MAX_UNIT
    s[0]["unit_count"] = 256
    assert fm.bad_argument(u, s) and rc_of(u=u, s=s, data=huge, n=len(huge)) == edgpu.BAD_ARGUMENT


# ---- 7. pointer kinds ----

@pytest.mark.parametrize("es_kind,out_kind", [("host", "host"), ("device", "device"), ("pinned", "device"), ("device", "pinned")])
def test_pointer_kinds(ctx, es_kind, out_kind):
    per_stream = [[(es_unit(1 + (53 * j) % 900, j, 0x65 if j % 5 == 0 else 0x41), 3000 * j, KEY if j % 5 == 0 else 0) for j in range(40)],
                  [], [(es_unit(300000, 5), 77, KEY)]]      # 300 kB: past the 256-KiB threshold of the reads into pinned memory
    st = check(ctx, None, per_stream, what="first", es_kind=es_kind, out_kind=out_kind)
    check(ctx, None, per_stream, states=st, what="second", es_kind=es_kind, out_kind=out_kind)


# ---- 8. end to end through the tap ----

def test_trace_through_tap_mux_and_recorder(tmp_path):
    import tap_traces as tt
    from easydarwin_amd import flv
    from test_mp4_init import CASES, PPS
    from test_gpu_tap import add, ingest
    sps = CASES["baseline 640x480"][0]
    sessions = []
    for k in range(2):
        aus = []
        for a in range(24):
            if a % 8 == 0:
                aus.append([sps, PPS, tt.nal(5, 3000 + 100 * k + a)])
            else:
                aus.append([tt.nal(1, 40 + 37 * a + k), tt.nal(1, 5)])
        sessions.append(aus)
    with edgpu.Context(**SMALL) as c:
        assert c.kernel_times(8) == []
        ids = []
        for k in range(2):
            ids.append(add(c))
        c.tap_drain()
        assert c.kernel_times(8) == []                      # the mux never ran: nothing recorded
        rec = flv.Recorder(str(tmp_path))
        packets = [tt.packetise(aus, mtu=700, stap=True, seq0=1000 * (k + 1))[0] for k, aus in enumerate(sessions)]
        calls = 0
        for part in range(3):
            batch = []
            for k, pk in enumerate(packets):
                lo, hi = len(pk) * part // 3, len(pk) * (part + 1) // 3
                batch += [(ids[k], 0, 10 * part, p) for p in pk[lo:hi]]
            ingest(c, batch)
            data, tags, units, streams = c.tap_drain_flv(flush=part == 2)
            rec.push(data, tags, streams)
            calls += 1 if len(streams) else 0
        rec.close()
        assert len(c.kernel_times(8)) == calls == 3
    summary = rec.summary()
    assert len(summary) == 2
    for k, s in enumerate(ids):
        (name,) = summary["%d_0" % s]["files"]
        parsed = flv_demux.file(open(tmp_path / name, "rb").read())
        assert [t["type"] for t in parsed[:2]] == [18, 9] and parsed[1]["config"]["sps"] == sps and parsed[1]["config"]["pps"] == PPS
        assert sum(1 for t in parsed if t.get("packet_type") == 0) == 1
        assert [t["nals"] for t in parsed[2:]] == sessions[k]
        assert [t["timestamp"] for t in parsed[2:]] == [3000 * a // 90 for a in range(24)]
        assert [t["key"] for t in parsed[2:]] == [a % 8 == 0 for a in range(24)]


def test_tap_record_tool_flv(tmp_path):
    """tools/tap_record.py --flv on the pushes of `mixed`: every file parses."""
    import json
    import os
    import subprocess
    import sys
    from scenarios import SCENARIOS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    trace = tmp_path / "mixed.edtr"
    trace.write_bytes(SCENARIOS["mixed"]().to_bytes())
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "tap_record.py"), "--trace", str(trace), "--tick-ms", "50",
                          "--flv", "--segment", "0.2", "--out", str(tmp_path / "rec")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    report = json.loads(out.stdout.strip().split("\n")[-1])
    assert report["files"] >= 1 and report["units"] > 0
    for row in report["streams"].values():
        for name in row["files"]:
            parsed = flv_demux.file(open(tmp_path / "rec" / name, "rb").read())
            assert [t["type"] for t in parsed[:2]] == [18, 9] and parsed[1]["packet_type"] == 0 and parsed[2]["key"]
