"""GPU: the H.264 elementary-stream tap (edgpu_tap_*, edgpu_tap.hip) against tests/tap_model.py --
bytes, units, stream rows and counters -- over traces each test builds itself, and a round trip
that does not involve the model.

The shapes are the smallest at which the kernels can go wrong: the scan's rounds are TAP_ROUND
entries, so drains of 1 / R-1 / R / R+1 / 2R / 2R+1 packets, FU-A chains and unit boundaries that
break at the last lane of a round and the first of the next, state carried over every cut of a
129-packet run, every destination byte phase against every length mod 16 with sources at slot
bytes 16, 18, 20, 24, 28 and odd STAP-A offsets, a 64-packet / 64-KiB ring that wraps, and 300
taps (two blocks of the placement scan)."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import tap_traces as tt
from easydarwin_amd import edgpu
from easydarwin_amd.synth import TrackSpec, make_sdp
from tap_model import COUNTERS, DAMAGED, KEY, OPEN_END, PARAMS, START, UNIT_FIELDS, TapModel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = edgpu.TAP_ROUND
H264 = [TrackSpec("video", "H264/90000", 96)]
AV = [TrackSpec("video", "H264/90000", 96), TrackSpec("audio", "MPEG4-GENERIC/44100/2", 97)]
SMALL = dict(max_batch_packets=1 << 15, max_batch_bytes=32 << 20, out_arena_bytes=32 << 20, max_out_packets=1 << 16)
TINY_RING = dict(SMALL, video_ring_packets=64, video_ring_bytes=64 << 10, other_ring_packets=64, other_ring_bytes=64 << 10)


@pytest.fixture(scope="module")
def ctx():
    with edgpu.Context(**SMALL) as c:
        yield c


def add(ctx, tracks=H264, tap=True):
    s = ctx.session_add(make_sdp(tracks))
    ctx.session_ssrc_prefs(s, False, 30)
    if tap:
        ctx.tap_enable(s, 0)
    return s


def ingest(ctx, pkts):
    """pkts: [(session, channel, arrival, bytes)]"""
    ctx.ingest_host(*edgpu.build_batch(pkts))
    ctx.keyframe_index()


def feed(ctx, sess_packets, t0=1000):
    """sess_packets: {session: [bytes]} -> one ingest, arrival t0 + position."""
    ingest(ctx, [(s, 0, t0 + k, p) for s, pk in sess_packets.items() for k, p in enumerate(pk)])


def split(data, units, streams):
    """A drain by (session, track): (bytes, units with stream-relative offsets, counters)."""
    out = {}
    for i, st in enumerate(streams):
        off, n = int(st["offset"]), int(st["bytes"])
        assert off % 16 == 0
        us = units[int(st["unit_first"]):int(st["unit_first"]) + int(st["unit_count"])]
        assert all(int(u["stream"]) == i for u in us)
        rows = [{k: int(u[k]) for k in UNIT_FIELDS} for u in us]
        for r in rows:
            r["offset"] -= off
        out[(int(st["session"]), int(st["track"]))] = (bytes(data[off:off + n]), rows, {k: int(st[k]) for k in COUNTERS})
    # disjoint streams in row order
    ends = [(int(st["offset"]), int(st["offset"]) + int(st["bytes"])) for st in streams]
    assert all(a[1] <= b[0] for a, b in zip(ends, ends[1:]))
    return out


def drain(ctx, flush=False):
    return split(*ctx.tap_drain(flush=flush))


def expect(model, flush=False):
    b, u = model.drain(flush=flush)
    return b, u, dict(model.c)


def same(got, want, what=""):
    gb, gu, gc = got
    wb, wu, wc = want
    assert gc == wc, f"{what}: counters (engine, model) {gc} {wc}"
    assert len(gu) == len(wu), f"{what}: {len(gu)} units, model {len(wu)}"
    for k, (g, w) in enumerate(zip(gu, wu)):
        assert g == w, f"{what}: unit {k} (engine, model) {g} {w}"
    if gb != wb:
        first = next((i for i, (a, b) in enumerate(zip(gb, wb)) if a != b), min(len(gb), len(wb)))
        raise AssertionError(f"{what}: bytes differ at {first} of {len(gb)} / {len(wb)}")


def run_sessions(ctx, traces, steps, flush_last=False, what=""):
    """traces: {name: [bytes]}; steps: {name: [cut, ...]} -- packets [prev cut, cut) are enqueued before
    drain k, the rest before the last one.  Every drain of every session is compared with its model."""
    sess = {n: (add(ctx), TapModel()) for n in traces}
    nsteps = max(len(c) for c in steps.values()) + 1
    for k in range(nsteps):
        batch = {}
        for n, pk in traces.items():
            cuts = [0] + list(steps[n]) + [len(pk)] * (nsteps - len(steps[n]))
            s, m = sess[n]
            part = pk[cuts[k]:cuts[k + 1]]
            batch[s] = part
            for j, p in enumerate(part):
                m.push(p, 1000 * (k + 1) + j)
        feed(ctx, {s: p for s, p in batch.items() if p}, t0=1000 * (k + 1))
        flush = flush_last and k == nsteps - 1
        got = drain(ctx, flush=flush)
        for n, (s, m) in sess.items():
            same(got[(s, 0)], expect(m, flush), f"{what}{n} drain {k}")
    for s, _ in sess.values():
        ctx.tap_disable(s, 0)
    return sess


def single(seq, ts, marker=True, size=30, typ=1):
    return tt.header(seq, ts, marker) + tt.nal(typ, size, fill=seq)


# ---- 1. round boundaries ----

def test_packets_per_drain_around_the_round(ctx):
    traces, steps = {}, {}
    for n in (1, R - 1, R, R + 1, 2 * R, 2 * R + 1):
        traces[f"n={n}"] = [single(65500 + k, 3000 * k, size=20 + k % 50) for k in range(2 * n)]
        steps[f"n={n}"] = [n]
    run_sessions(ctx, traces, steps)


def fu_chain(nfrag, seq0, ts, typ=5, frag=40):
    n = tt.nal(typ, 1 + nfrag * frag)
    pk, _ = tt.packetise([[n]], mtu=frag + 2, seq0=seq0, ts0=ts)
    assert len(pk) == nfrag
    return pk


def test_chain_and_unit_boundaries_at_round_edges(ctx):
    traces = {"whole": fu_chain(2 * R + 10, 10, 500)}
    for pos in (R - 1, R, R + 1, 2 * R - 1, 2 * R):
        chain = fu_chain(2 * R + 10, 10, 500)
        traces[f"lost@{pos}"] = chain[:pos] + chain[pos + 1:]                 # the fragment at lane pos has a gap
        traces[f"type@{pos}"] = chain[:pos] + [chain[pos][:13] + bytes([1]) + chain[pos][14:]] + chain[pos + 1:]
        traces[f"unit@{pos}"] = fu_chain(pos, 10, 500) + fu_chain(R + 5, 10 + pos, 3500, typ=1)
        traces[f"nomarker@{pos}"] = [tt.header(10 + k, 500, False) + p[12:] for k, p in enumerate(fu_chain(pos, 10, 500))] + \
            fu_chain(R + 5, 10 + pos, 3500, typ=1)
    sess = run_sessions(ctx, traces, {n: [] for n in traces})
    c = {n: m.c for n, (_, m) in sess.items()}
    assert c["whole"]["orphans"] == 0 and c[f"lost@{R}"]["orphans"] == 2 * R + 10 - R - 1
    assert c[f"type@{R - 1}"]["orphans"] == 2 * R + 10 - (R - 1) and c[f"unit@{R}"]["damaged_units"] == 0


# ---- 2. every cut, in one call ----

def cut_run():
    """129 packets, 4 access units (57 + 40 + 23 + 10 packets, one of the second lost): a STAP-A, a gap
    inside a chain, a sequence wrap; the last packet has the marker."""
    aus = [[tt.nal(7, 20), tt.nal(8, 6), tt.nal(5, 2100)], [tt.nal(1, 1500)], [tt.nal(6, 9), tt.nal(1, 800)], [tt.nal(1, 371)]]
    pk, reached = tt.packetise(aus, mtu=40, stap=True, seq0=65480, drop=(70,))
    assert "stap" in reached and "drop" in reached and "seq-wrap" in reached
    assert len(pk) == 129 and pk[-1][1] & 0x80
    return pk


def test_state_carried_across_every_cut(ctx):
    pk = cut_run()
    whole = TapModel()
    for k, p in enumerate(pk):
        whole.push(p, k)
    wb, wu = whole.drain()
    assert len(wu) >= 3 and any(u["flags"] & DAMAGED for u in wu)
    sess = [(add(ctx), TapModel()) for _ in range(128)]
    outs = [[b"", []] for _ in sess]
    for half in range(2):
        batch = {}
        for k, (s, m) in enumerate(sess):
            part = pk[:k + 1] if half == 0 else pk[k + 1:]
            batch[s] = part
            for j, p in enumerate(part):
                m.push(p, 1000 * (half + 1) + j)
        feed(ctx, batch, t0=1000 * (half + 1))
        got = drain(ctx)
        for k, (s, m) in enumerate(sess):
            g = got[(s, 0)]
            same(g, expect(m), f"cut {k + 1} drain {half}")
            outs[k][1] += [dict(u, offset=u["offset"] + len(outs[k][0])) for u in g[1]]
            outs[k][0] += g[0]
    for k, (b, u) in enumerate(outs):
        assert b == wb, k
        strip = lambda us: [{f: x[f] for f in UNIT_FIELDS if f != "arrival_ms"} for x in us]
        assert strip(u) == strip(wu), k
    for s, _ in sess:
        ctx.tap_disable(s, 0)


# ---- 3. source and destination phases ----

def phase_trace(L):
    pk, seq, ts = [], 100, 0
    def more(aus, **kw):
        nonlocal pk, seq, ts
        p, _ = tt.packetise(aus, seq0=seq, ts0=ts, **kw)
        pk += p
        seq += len(p)
        ts += 3000 * len(aus)
    more([[tt.nal(1, L)]], mtu=1400)
    for cc in (0, 1, 2, 3):
        more([[tt.nal(1, 37 + L), tt.nal(5, 150 + L)], [tt.nal(1, L + cc)]], mtu=60, cc=cc)
    more([[tt.nal(7, 3), tt.nal(8, 2 + L % 5), tt.nal(6, 4 + L), tt.nal(1, 1)]], mtu=1400, stap=True)
    more([[tt.nal(1, 16 + L % 16)]], mtu=1400, ext=1, pad=3)
    return pk


def test_every_byte_phase_and_nothing_written_outside(ctx):
    traces = {L: phase_trace(L) for L in range(1, 49)}
    sess = {L: (add(ctx), TapModel()) for L in traces}
    feed(ctx, {s: traces[L] for L, (s, _) in sess.items()})
    for L, (s, m) in sess.items():
        for k, p in enumerate(traces[L]):
            m.push(p, 1000 + k)
    cap = 1 << 20
    dev = ctx.device_alloc(cap)
    ctx.copy_to_device(dev.ptr, np.full(cap, 0xA5, dtype=np.uint8))
    n, units, streams = ctx.tap_drain(out=dev)
    data = ctx.copy_to_host(dev.ptr, cap)
    dev.free()
    got = split(data, units, streams)
    phases = set()
    for L, (s, m) in sess.items():
        want = expect(m)
        same(got[(s, 0)], want, f"L={L}")
        phases |= {((u["offset"] + 4) % 16, u["bytes"] % 16) for u in want[1]}
    assert {p for p, _ in phases} == set(range(16)) and {q for _, q in phases} == set(range(16))
    allowed = np.zeros(cap, dtype=bool)
    for st in streams:
        allowed[int(st["offset"]):(int(st["offset"]) + int(st["bytes"]) + 15) // 16 * 16] = True
    assert n <= cap and np.all(data[~allowed] == 0xA5)
    exact = np.zeros(cap, dtype=bool)
    for st in streams:
        exact[int(st["offset"]):int(st["offset"]) + int(st["bytes"])] = True
    assert np.all(data[~exact] == 0xA5)                         # (the kernel writes no padding either)
    for s, _ in sess.values():
        ctx.tap_disable(s, 0)


# ---- 4. ring edges ----

def test_ring_wrap_and_lapped_ring():
    with edgpu.Context(ring_growth=edgpu.FALSE, **TINY_RING) as c:
        s, m = add(c), TapModel()
        seq = 65000
        for tick in range(10):                      # 10 x 40 packets of ~1.4 kB: the meta ring 6 x, the byte ring 8 x
            pk = []
            for f in range(4):
                p, _ = tt.packetise([[tt.nal(5 if f == 0 else 1, 10 * 1380 - 3 * tick - f)]], mtu=1382, seq0=seq,
                                    ts0=3000 * (4 * tick + f))
                assert len(p) == 10
                pk += p
                seq += 10
            feed(c, {s: pk}, t0=1000 * tick)
            for k, p in enumerate(pk):
                m.push(p, 1000 * tick + k)
            same(drain(c)[(s, 0)], expect(m), f"tick {tick}")
        assert m.c["missed"] == 0 and m.c["units"] == 40
        # a single batch that laps the ring: 100 packets into 64 entries leave the last 64
        s2, m2 = add(c), TapModel()
        pk = [single(300 + k, 3000 * (k // 3), marker=k % 3 == 2) for k in range(100)]
        feed(c, {s2: pk})
        for k, p in enumerate(pk):
            m2.push(p, 1000 + k)
        m2.lose(36)
        got = drain(c)
        same(got[(s2, 0)], expect(m2), "lapped ring")
        assert m2.c["missed"] == 36 and got[(s2, 0)][1][0]["flags"] & DAMAGED


# ---- 5. many taps ----

def test_many_taps_in_one_drain():
    with edgpu.Context(video_ring_bytes=4 << 20, **SMALL) as c:
        many_taps(c)


def many_taps(ctx):
    rng = np.random.default_rng(9)
    sess, batch = [], []
    for i in range(300):
        s = add(ctx, AV, tap=False)
        if i == 0:
            with pytest.raises(edgpu.EdgpuError) as ei:
                ctx.tap_enable(s, 1)
            assert ei.value.code == edgpu.BAD_ARGUMENT         # an audio track is refused
        npk = 0 if i % 5 == 0 else 1 if i % 5 == 1 else 3000 if i in (7, 158) else int(rng.integers(2, 90))
        m = TapModel()
        pk = []
        if npk:
            nal_bytes = [int(rng.integers(1, 900)) for _ in range(max(npk // 3, 1))]
            pk, _ = tt.packetise([[tt.nal(1 + k % 5, n)] for k, n in enumerate(nal_bytes)], mtu=300, seq0=i * 77)
            pk = pk[:npk]
        sess.append((s, m, pk))
        batch += [(s, 0, 1000 + k, p) for k, p in enumerate(pk)]
        batch += [(s, 2, 1000, tt.header(5, 5, True) + bytes(40))]             # audio, never tapped
    ingest(ctx, batch)
    tapped = [(s, m, pk) for i, (s, m, pk) in enumerate(sess) if i % 7 != 3]     # some video tracks stay untapped
    drained_before = drain(ctx)
    assert drained_before == {}
    for s, m, pk in tapped:
        ctx.tap_enable(s, 0)
    # the taps start at the next packet: enqueue the traces again
    ingest(ctx, [b for b in batch if b[1] == 0])
    data, units, streams = ctx.tap_drain(flush=True)
    assert len(streams) == len(tapped) > 256
    assert [int(x) for x in streams["session"]] == [s for s, _, _ in tapped]
    got = split(data, units, streams)
    for s, m, pk in tapped:
        for k, p in enumerate(pk):
            m.push(p, 1000 + k)
        same(got[(s, 0)], expect(m, True), f"session {s}")
    for s, _, _ in sess:
        ctx.session_remove(s)
    assert drain(ctx) == {}


# ---- 6. overflow ----

def test_overflow_consumes_nothing():
    with edgpu.Context(**SMALL) as c:
        overflow(c)


def overflow(ctx):
    pk = cut_run()
    sess = [(add(ctx), TapModel()) for _ in range(3)]
    feed(ctx, {s: pk[:40 + 30 * k] for k, (s, _) in enumerate(sess)})
    want = []
    for k, (s, m) in enumerate(sess):
        for j, p in enumerate(pk[:40 + 30 * k]):
            m.push(p, 1000 + j)
        want.append(expect(m))
    need_bytes = sum((len(w[0]) + 15) // 16 * 16 for w in want)
    need_units = sum(len(w[1]) for w in want)
    assert need_units >= 3
    buf = np.full(need_bytes + 64, 0xA5, dtype=np.uint8)
    for short in ("bytes", "units", "streams"):
        units = np.zeros(need_units - (short == "units"), dtype=edgpu.TAP_UNIT_DTYPE)
        streams = np.zeros(3 - (short == "streams"), dtype=edgpu.TAP_STREAM_DTYPE)
        cap = need_bytes - (short == "bytes")
        rc, res = ctx.tap_drain_raw(0, buf.ctypes.data, cap, edgpu.PTR_HOST, units, streams)
        assert rc == edgpu.OUT_OVERFLOW, short
        assert (res.bytes, res.units, res.streams) == (need_bytes, need_units, 3)
        assert np.all(buf == 0xA5)
    units = np.zeros(need_units, dtype=edgpu.TAP_UNIT_DTYPE)
    streams = np.zeros(3, dtype=edgpu.TAP_STREAM_DTYPE)
    rc, res = ctx.tap_drain_raw(0, buf.ctypes.data, need_bytes, edgpu.PTR_HOST, units, streams)
    assert rc == edgpu.OK and (res.bytes, res.units, res.streams) == (need_bytes, need_units, 3)
    got = split(buf, units, streams)
    for (s, _), w in zip(sess, want):
        same(got[(s, 0)], w, "retry")
    assert np.all(buf[need_bytes:] == 0xA5)
    for s, _ in sess:
        ctx.tap_disable(s, 0)


# ---- 7. flush, reset and lifecycle ----

def test_flush_reset_and_lifecycle():
    with edgpu.Context(**SMALL) as c:
        lifecycle(c)


def lifecycle(ctx):
    s, m = add(ctx), TapModel()
    pk = [single(10 + k, 3000 * (k // 2), marker=False) for k in range(5)]
    feed(ctx, {s: pk})
    for k, p in enumerate(pk):
        m.push(p, 1000 + k)
    same(drain(ctx)[(s, 0)], expect(m), "plain")
    g = drain(ctx, flush=True)[(s, 0)]
    same(g, expect(m, True), "flush")
    assert g[1][-1]["flags"] & OPEN_END and g[2]["units"] == 3
    ctx.tap_enable(s, 0)                                        # enabling again resets it
    g = drain(ctx, flush=True)[(s, 0)]
    assert g == (b"", [], dict.fromkeys(COUNTERS, 0))
    feed(ctx, {s: [single(99, 7, typ=5)]})
    g = drain(ctx)[(s, 0)]
    assert g[2]["packets"] == 1 and g[1][0]["flags"] == KEY     # no gap against the state before the reset
    ctx.session_remove(s)
    assert drain(ctx) == {}
    s2 = add(ctx, tap=False)                                    # the reused slot starts clean
    assert s2 == s and drain(ctx) == {}
    ctx.tap_enable(s2, 0)
    feed(ctx, {s2: [single(5, 7)]})
    g = drain(ctx)[(s2, 0)]
    assert g[2] == dict(dict.fromkeys(COUNTERS, 0), packets=1, units=1)
    ctx.tap_disable(s2, 0)
    ctx.tap_disable(s2, 0)
    a = add(ctx, [TrackSpec("video", "MP4V-ES/90000", 96)], tap=False)
    b = add(ctx, [TrackSpec("video", "h264/90000", 96)], tap=False)
    for bad in ((a, 0), (b, 0), (s2, 1), (1 << 20, 0)):
        with pytest.raises(edgpu.EdgpuError) as ei:
            ctx.tap_enable(*bad)
        assert ei.value.code == edgpu.BAD_ARGUMENT


# ---- 8. ingest paths ----

def test_four_ingest_paths_and_device_output(ctx):
    pk = cut_run()
    halves = [pk[:77], pk[77:]]
    m = TapModel()
    want = []
    for h in halves:
        for j, p in enumerate(h):
            m.push(p, 2000 + j)
        want.append(expect(m))

    def drained(s, k, what):
        same(drain(ctx)[(s, 0)], want[k], f"{what} half {k}")

    s = add(ctx)
    for k, h in enumerate(halves):
        ingest(ctx, [(s, 0, 2000 + j, p) for j, p in enumerate(h)])
        drained(s, k, "host")
    ctx.tap_disable(s, 0)
    for kind in ("pinned", "device"):
        s = add(ctx)
        for k, h in enumerate(halves):
            arrays = edgpu.build_batch([(s, 0, 2000 + j, p) for j, p in enumerate(h)])
            bufs = []
            for a in arrays:
                v = np.ascontiguousarray(a).view(np.uint8).ravel()
                if kind == "pinned":
                    b = ctx.host_alloc(max(v.nbytes, 16))
                    b.array[:v.nbytes] = v
                else:
                    b = ctx.device_alloc(max(v.nbytes, 16))
                    ctx.copy_to_device(b.ptr, v)
                bufs.append(b)
            fn = ctx.ingest_pinned if kind == "pinned" else ctx.ingest_device
            fn(bufs[0].ptr, len(arrays[0]), bufs[1].ptr, bufs[2].ptr, len(arrays[2]), bufs[3].ptr, arrays[3].nbytes)
            ctx.keyframe_index()
            drained(s, k, kind)
            for b in bufs:
                b.free()
        ctx.tap_disable(s, 0)
    s = add(ctx)
    for k, h in enumerate(halves):
        frames = [b"$\x00" + len(p).to_bytes(2, "big") + p for p in h]
        reads = np.zeros(len(h), dtype=edgpu.TCP_READ_DTYPE)
        off = 0
        for i, f in enumerate(frames):
            reads[i] = (s, len(f), off, 2000 + i)
            off += len(f)
        res = ctx.ingest_interleaved(reads, b"".join(frames))
        assert int(res["frames"].sum()) == len(h)
        ctx.keyframe_index()
        drained(s, k, "interleaved")
    ctx.tap_disable(s, 0)


# ---- 9. read-only ----

class TapContext(edgpu.Context):
    """Every H.264 track tapped at session add, every tap drained before each fan-out."""

    def __init__(self, tap=True, **cfg):
        super().__init__(**cfg)
        self.tap, self.tapped, self.units, self.bytes = tap, 0, 0, 0

    def session_add(self, sdp, udp_push=False):
        s = super().session_add(sdp, udp_push=udp_push)
        for t in range(self.session_tracks(s) if self.tap else 0):
            try:
                self.tap_enable(s, t)
                self.tapped += 1
            except edgpu.EdgpuError as e:
                assert e.code == edgpu.BAD_ARGUMENT
        return s

    def fanout(self, now_ms):
        if self.tap:
            data, units, streams = self.tap_drain()
            self.units += len(units)
            self.bytes += len(data)
        return super().fanout(now_ms)


def replay_cfg(trace):
    """The context replay() itself would make for the trace's stream prefs."""
    from easydarwin_amd.replay import pref_bool, pref_values
    pv = pref_values(trace.prefs)
    return dict(reflector_buffer_size_sec=int(pv["reflector_buffer_size_sec"]),
                rtp_reflector_threshold_msec=max(1000, int(pv["rtp_reflector_threshold_msec"])),
                reflector_rtp_info_offset_msec=int(pv["reflector_rtp_info_offset_msec"]) or edgpu.FALSE,
                reflector_use_in_packet_receive_time=int(pref_bool(pv["reflector_use_in_packet_receive_time"])),
                reflector_in_packet_max_receive_sec=int(pv["reflector_in_packet_max_receive_sec"]) or edgpu.FALSE)


@pytest.mark.parametrize("name", ["mixed", "backpressure", "leave"])
def test_goldens_unchanged_with_every_track_tapped(name):
    from easydarwin_amd.replay import replay
    from scenarios import SCENARIOS
    import hashlib
    import json
    want = json.load(open(os.path.join(ROOT, "tests", "golden", name + ".json")))["capture_sha256"]
    trace = SCENARIOS[name]()
    with TapContext(tap=False, **replay_cfg(trace)) as c:
        plain, _ = replay(trace, ctx=c)
        assert c.kernel_times(5) == []                          # no tap: nothing recorded
    assert hashlib.sha256(plain).hexdigest() == want
    with TapContext(**replay_cfg(trace)) as c:
        got, _ = replay(trace, ctx=c)
        assert c.tapped and c.units and c.bytes and c.kernel_times(5)
    assert got == plain


# ---- 10. round trip, no model ----

def test_round_trip_without_the_model(ctx):
    rng = np.random.default_rng(4)
    cases = {}
    for name, kw in (("plain", {}), ("stap", dict(stap=True)), ("cc", dict(cc=2)), ("ext+pad", dict(ext=2, pad=5)), ("small", dict(mtu=64))):
        aus = [[tt.nal(7, 24), tt.nal(8, 8), tt.nal(5, int(rng.integers(2000, 6000)))]]
        aus += [[tt.nal(1, int(rng.integers(1, 3000)))] for _ in range(30)]
        pk, _ = tt.packetise(aus, **dict(dict(mtu=1400, seq0=65500), **kw))
        cases[name] = (add(ctx), aus, pk)
    feed(ctx, {s: pk for s, _, pk in cases.values()})
    got = drain(ctx)
    for name, (s, aus, pk) in cases.items():
        b, units, c = got[(s, 0)]
        assert b == tt.annexb(aus), name
        assert [u["bytes"] for u in units] == [sum(4 + len(n) for n in a) for a in aus], name
        assert [u["flags"] for u in units] == [KEY | PARAMS] + [0] * 30, name
        assert c["packets"] == len(pk) and c["damaged_units"] == 0
        ctx.tap_disable(s, 0)


# ---- 11. the tool ----

def test_tap_record_tool(tmp_path):
    import json
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "tap_record.py"), "--sessions", "2", "--seconds", "3",
                          "--out", str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    index = json.load(open(tmp_path / "index.json"))
    assert len(index["files"]) >= 2
    for f in index["files"]:
        data = open(tmp_path / f["file"], "rb").read()
        assert data[:5] == START + b"\x67", f["file"]               # SPS, then PPS and the IDR
        assert START + b"\x68" in data[:64] and START + b"\x65" in data[:96]
        assert f["units"][0]["flags"] & KEY
        assert sum(u["bytes"] for u in f["units"]) == len(data)
        assert all(data[u["offset"]:u["offset"] + 4] == START for u in f["units"] if u["bytes"])
    assert index["drained_units"] >= sum(len(f["units"]) for f in index["files"])
