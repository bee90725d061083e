"""GPU: the AAC audio tap (edgpu_aac_tap_*, edgpu_aac.hip) against tests/aac_model.py -- bytes, frame
rows, stream rows and counters -- over traces each test builds itself, and a round trip through the
ADTS reader that does not involve the model.

The shapes are the smallest at which the kernels can go wrong: the scan's rounds are 64 entries, so
fragment chains that start at entries 62, 63 and 64 and end at 64, 65 and 130; every source phase
against every destination phase mod 16 under both framings; RTP headers the fast path does not
cover; 257 taps (two blocks of the placement scan); a 64-packet / 64-KiB ring that wraps and is
lapped."""
import struct

import numpy as np
import pytest

import aac_traces as at
import adts_reader
import tap_traces as tt
from aac_model import ADTS, COUNTERS, DISCONT, FRAGMENTED, FRAME_FIELDS, HBR, LBR, RAW, AacModel
from easydarwin_amd import edgpu
from easydarwin_amd.synth import TrackSpec, make_sdp
from tap_model import TapModel

pytestmark = pytest.mark.gpu

R = edgpu.AAC_ROUND
AV = [TrackSpec("video", "H264/90000", 96), TrackSpec("audio", "mpeg4-generic/44100/2", 97)]
AUDIO = [TrackSpec("audio", "MPEG4-GENERIC/44100/2", 97)]
SMALL = dict(max_batch_packets=1 << 15, max_batch_bytes=32 << 20, out_arena_bytes=32 << 20, max_out_packets=1 << 16)
TINY_RING = dict(SMALL, video_ring_packets=64, video_ring_bytes=64 << 10, other_ring_packets=64, other_ring_bytes=64 << 10)


def config(mode=HBR, framing=ADTS):
    return edgpu.AacConfig(mode, framing, 2, 4, 2, 0)


@pytest.fixture(scope="module")
def ctx():
    with edgpu.Context(**SMALL) as c:
        yield c


def add(ctx, mode=HBR, framing=ADTS, tap=True):
    """An audio-only session and its model."""
    s = ctx.session_add(make_sdp(AUDIO))
    ctx.session_ssrc_prefs(s, False, 30)
    if tap:
        ctx.aac_tap_enable(s, 0, config(mode, framing))
    return s, AacModel(mode=mode, framing=framing)


def feed(ctx, sess_packets, t0=1000, channel=0):
    """{session: [bytes]} -> one ingest, arrival t0 + position; synchronised before any drain."""
    ctx.ingest_host(*edgpu.build_batch([(s, channel, t0 + k, p) for s, pk in sess_packets.items() for k, p in enumerate(pk)]))
    ctx.keyframe_index()
    ctx.sync()


def split(data, frames, streams):
    out = {}
    for i, st in enumerate(streams):
        off, n = int(st["offset"]), int(st["bytes"])
        assert off % 16 == 0
        fs = frames[int(st["frame_first"]):int(st["frame_first"]) + int(st["frame_count"])]
        assert all(int(f["stream"]) == i for f in fs)
        rows = [{k: int(f[k]) for k in FRAME_FIELDS} for f in fs]
        for r in rows:
            r["offset"] -= off
        out[(int(st["session"]), int(st["track"]))] = (bytes(data[off:off + n]), rows, {k: int(st[k]) for k in COUNTERS})
    ends = [(int(st["offset"]), int(st["offset"]) + int(st["bytes"])) for st in streams]
    assert all(a[1] <= b[0] for a, b in zip(ends, ends[1:]))
    return out


def drain(ctx, flush=False):
    return split(*ctx.aac_tap_drain(flush=flush))


def expect(model, flush=False):
    b, f = model.drain(flush=flush)
    return b, f, dict(model.c)


def same(got, want, what=""):
    gb, gf, gc = got
    wb, wf, wc = want
    assert gc == wc, f"{what}: counters (engine, model) {gc} {wc}"
    assert len(gf) == len(wf), f"{what}: {len(gf)} frames, model {len(wf)}"
    for k, (g, w) in enumerate(zip(gf, wf)):
        assert g == w, f"{what}: frame {k} (engine, model) {g} {w}"
    if gb != wb:
        first = next((i for i, (a, b) in enumerate(zip(gb, wb)) if a != b), min(len(gb), len(wb)))
        raise AssertionError(f"{what}: bytes differ at {first} of {len(gb)} / {len(wb)}")


def run(ctx, cases, flush_last=False):
    """cases: {name: (mode, framing, [packets], [cut, ...])} -- packets [prev cut, cut) are enqueued before
    drain k, the rest before the last one; every drain of every case is compared with its model."""
    sess = {n: add(ctx, c[0], c[1]) for n, c in cases.items()}
    nsteps = max(len(c[3]) for c in cases.values()) + 1
    for k in range(nsteps):
        batch = {}
        for n, (_, _, pk, cuts) in cases.items():
            cuts = [0] + list(cuts) + [len(pk)] * (nsteps - len(cuts))
            s, m = sess[n]
            batch[s] = pk[cuts[k]:cuts[k + 1]]
            for j, p in enumerate(batch[s]):
                m.push(p, 1000 * (k + 1) + j)
        feed(ctx, {s: p for s, p in batch.items() if p}, t0=1000 * (k + 1))
        flush = flush_last and k == nsteps - 1
        got = drain(ctx, flush=flush)
        for n, (s, m) in sess.items():
            same(got[(s, 0)], expect(m, flush), f"{n} drain {k}")
    for s, _ in sess.values():
        ctx.aac_tap_disable(s, 0)
    return {n: m for n, (_, m) in sess.items()}


def hbr(sizes, idx=None):
    idx = idx or [0] * len(sizes)
    return struct.pack(">H", 16 * len(sizes)) + b"".join(struct.pack(">H", (s << 3) | i) for s, i in zip(sizes, idx))


def one(seq, n=20, ts=None, **kw):
    return at.rtp(seq, 1024 * seq if ts is None else ts, True, hbr([n]) + at.frame(n, seq), **kw)


def chain(size, room, seq0, ts=777):
    body = at.frame(size, seq0)
    return [at.rtp(seq0 + k, ts, o + room >= size, hbr([size]) + body[o:o + room]) for k, o in enumerate(range(0, size, room))]


# ---- 1. phases ----

def test_every_source_and_destination_phase_and_nothing_written_outside(ctx):
    lengths = list(range(1, 41)) + list(range(8170, 8185))
    cases = {}
    for framing in (ADTS, RAW):
        for agg in (1, 16):
            frames = [at.frame(n, agg) for n in lengths]
            cases[(framing, agg)] = (HBR, framing, at.packetise(frames, mtu=1400, max_aus=agg, seq0=65500), frames)
    lb = [at.frame(n, 5) for n in range(1, 41)]
    cases[(ADTS, "lbr")] = (LBR, ADTS, at.packetise(lb, hbr=False, mtu=1400, seq0=9), lb)
    cases[(RAW, "lbr")] = (LBR, RAW, at.packetise(lb, hbr=False, mtu=1400, max_aus=3, seq0=9), lb)
    sess = {n: add(ctx, c[0], c[1]) for n, c in cases.items()}
    feed(ctx, {sess[n][0]: c[2] for n, c in cases.items()})
    cap = 1 << 20
    dev = ctx.device_alloc(cap)
    ctx.copy_to_device(dev.ptr, np.full(cap, 0xA5, dtype=np.uint8))
    n, frames, streams = ctx.aac_tap_drain(out=dev)
    data = ctx.copy_to_host(dev.ptr, cap)
    dev.free()
    got = split(data, frames, streams)
    phases = {}
    for name, (mode, framing, pk, src) in cases.items():
        s, m = sess[name]
        for k, p in enumerate(pk):
            m.push(p, 1000 + k)
        want = expect(m)
        same(got[(s, 0)], want, str(name))
        body = [want[0][f["offset"] + (7 if framing == ADTS else 0):f["offset"] + f["bytes"]] for f in want[1]]
        assert body == src, name
        phases.setdefault(framing, set()).update((f["offset"] + (7 if framing == ADTS else 0)) % 16 for f in want[1])
        ctx.aac_tap_disable(s, 0)
    assert phases[ADTS] == set(range(16)) and phases[RAW] == set(range(16))
    exact = np.zeros(cap, dtype=bool)
    for st in streams:
        exact[int(st["offset"]):int(st["offset"]) + int(st["bytes"])] = True
    assert n <= cap and np.all(data[~exact] == 0xA5)            # no byte outside a stream's run, no padding either


def test_csrcs_extension_and_padding_take_the_slow_path(ctx):
    frames = [at.frame(n, 2) for n in range(1, 60)]
    cases = {}
    for name, kw in (("cc1", dict(cc=1)), ("cc3", dict(cc=3)), ("ext0", dict(ext=0)), ("ext2+pad", dict(ext=2, pad=5)),
                     ("cc2+ext1+pad", dict(cc=2, ext=1, pad=1))):
        cases[name] = (HBR, ADTS, at.packetise(frames, mtu=300, max_aus=16, **kw) + at.packetise([at.frame(900)], mtu=200, seq0=100, **kw), [])
        cases[name + " lbr"] = (LBR, RAW, at.packetise(frames, hbr=False, mtu=300, **kw), [])
    run(ctx, cases)


# ---- 2. chains ----

def test_chains_against_the_round(ctx):
    cases = {}
    for first in (R - 2, R - 1, R):
        for last in (R, R + 1, 2 * R + 2):
            nfrag = last - first + 1
            pk = [one(k) for k in range(first)] + chain(10 * nfrag - 3, 10, first) + [one(last + 1 + k) for k in range(3)]
            assert len(pk) == last + 4
            cases[f"{first}..{last}"] = (HBR, ADTS if first % 2 else RAW, pk, [])
    models = run(ctx, cases)
    assert all(m.c["frames"] == len(cases[n][2]) - (int(n.split("..")[1]) - int(n.split("..")[0])) and m.c["orphans"] == 0
               for n, m in models.items())


def test_chain_cut_by_a_drain_waits_and_cut_by_a_flush_orphans(ctx):
    pk = [one(k) for k in range(5)] + chain(95, 10, 5) + [one(15)]
    every = {f"cut {c}": (HBR, ADTS, pk, [c]) for c in range(4, 16)}
    models = run(ctx, every)
    assert all(m.c == dict(dict.fromkeys(COUNTERS, 0), packets=16, frames=7) for m in models.values())
    flushed = run(ctx, {"flush": (HBR, ADTS, pk[:9], [])}, flush_last=True)["flush"]
    assert flushed.c["orphans"] == 4 and flushed.c["frames"] == 5
    # a chain abandoned by a fragment whose own chain then waits: its orphans and DISCONT are not forgotten
    a, b = chain(95, 40, 1, ts=1000), chain(130, 50, 3, ts=2000)
    m = run(ctx, {f"abandoned then cut {c}": (HBR, ADTS, [one(0, ts=5)] + a[:2] + b + [one(6)], [c]) for c in (3, 4, 5)})
    assert all(x.c == dict(dict.fromkeys(COUNTERS, 0), packets=7, orphans=2, frames=3, discontinuities=1) for x in m.values())
    lane = run(ctx, {"abandoned at a round's edge": (HBR, RAW, [one(k) for k in range(R - 2)] + chain(95, 40, R - 2, ts=1)[:2] +
                                                      chain(130, 50, R, ts=2), [R + 1, R + 2])})
    assert lane["abandoned at a round's edge"].c["orphans"] == 2 and lane["abandoned at a round's edge"].c["discontinuities"] == 1
    # after the flush the rest of the chain opens a chain of its own that overruns nothing and never completes
    m = run(ctx, {"gap at the first fragment": (HBR, RAW, [one(1)] + chain(50, 20, 7) + [one(10)], [2, 3])})["gap at the first fragment"]
    assert m.c["discontinuities"] == 1 and m.c["frames"] == 3


def test_chains_broken_and_overrun(ctx):
    c = chain(95, 10, 20)
    cases = {
        "gap": c[:4] + c[5:] + [one(40)],
        "timestamp": c[:4] + chain(95, 10, 24, ts=999)[4:] + [one(40)],
        "size": c[:4] + [at.rtp(24 + k, 777, False, hbr([96]) + bytes(10)) for k in range(3)] + [one(40)],
        "overrun": c[:9] + [at.rtp(29, 777, True, hbr([95]) + bytes(6)), one(30)],
        "restart inside look-alikes": c + [at.rtp(30 + k, 777, False, p[12:]) for k, p in enumerate(c)] + [one(40)],
        "whole frame between": c[:4] + [one(24, ts=5)] + [at.rtp(25 + k, 777, False, p[12:]) for k, p in enumerate(c[4:])],
        "empty pieces": [at.rtp(1, 3, False, hbr([10])), at.rtp(2, 3, False, hbr([10])), at.rtp(3, 3, True, hbr([10]) + bytes(range(10))), one(4)],
        "lbr fragment": [at.rtp(1, 3, True, struct.pack(">HB", 8, 40 << 2) + bytes(10)), at.rtp(2, 4, True, struct.pack(">HB", 8, 4 << 2) + bytes(4))],
    }
    models = run(ctx, {n: (LBR if n.startswith("lbr") else HBR, ADTS, pk, []) for n, pk in cases.items()}, flush_last=True)
    assert models["gap"].c["orphans"] == 9 and models["overrun"].c["malformed"] == 1 and models["overrun"].c["orphans"] == 9
    assert models["restart inside look-alikes"].c["frames"] == 3 and models["lbr fragment"].c["malformed"] == 1


# ---- 3. every malformed / unsupported rule, each followed by a good packet ----

def test_every_drop_rule_sets_discont_on_the_next_frame(ctx):
    bad = {
        "one payload byte": b"\x00",
        "zero bits": b"\x00\x00" + bytes(8),
        "bits not a multiple": struct.pack(">H", 24) + bytes(20),
        "headers past the payload": hbr([4, 4, 4])[:7],
        "17 headers": hbr([1] * 17) + bytes(17),
        "au-index": hbr([4, 4], [1, 0]) + bytes(8),
        "au-index-delta": hbr([4, 4], [0, 2]) + bytes(8),
        "first au empty": hbr([0, 4]) + bytes(4),
        "second au past the end": hbr([4, 9]) + bytes(8),
        "adts too long": hbr([8185]) + bytes(100),
    }
    cases = {}
    for n, pay in bad.items():
        cases[n] = (HBR, ADTS, [one(1), at.rtp(2, 9, True, pay), one(3), one(4)], [])
        cases[n + " slow"] = (HBR, ADTS, [one(1, cc=1), at.rtp(2, 9, True, pay, cc=1), one(3, cc=1), one(4)], [])
    cases["lbr bits"] = (LBR, ADTS, [at.rtp(1, 9, True, struct.pack(">H", 12) + bytes(9)), at.rtp(2, 9, True, struct.pack(">HB", 8, 12) + bytes(3))], [])
    cases["skipped"] = (HBR, ADTS, [one(1), bytes(20), b"\x80" + bytes(11), one(2), one(4)], [])
    models = run(ctx, cases)
    for n in bad:
        c = models[n].c
        assert c["malformed"] + c["unsupported"] == 1 and c["discontinuities"] == 1, n
    assert models["skipped"].c["skipped"] == 2 and models["skipped"].c["discontinuities"] == 1


# ---- 4. overflow ----

def test_overflow_consumes_nothing():
    with edgpu.Context(**SMALL) as c:
        sess = [add(c, HBR, ADTS if k % 2 else RAW) for k in range(3)]
        traces = [at.packetise([at.frame(30 + j + k, k) for j in range(40 + 30 * k)], mtu=200, seq0=k) + chain(500, 120, 1000)[:2]
                  for k in range(3)]
        feed(c, {s: pk for (s, _), pk in zip(sess, traces)})
        want = []
        for (s, m), pk in zip(sess, traces):
            for j, p in enumerate(pk):
                m.push(p, 1000 + j)
            want.append(expect(m))
        need_bytes = sum((len(w[0]) + 15) // 16 * 16 for w in want)
        need_frames = sum(len(w[1]) for w in want)
        buf = np.full(need_bytes + 64, 0xA5, dtype=np.uint8)
        for short in ("bytes", "frames", "streams"):
            frames = np.zeros(need_frames - (short == "frames"), dtype=edgpu.AAC_FRAME_DTYPE)
            streams = np.zeros(3 - (short == "streams"), dtype=edgpu.AAC_STREAM_DTYPE)
            rc, res = c.aac_tap_drain_raw(0, buf.ctypes.data, need_bytes - (short == "bytes"), edgpu.PTR_HOST, frames, streams)
            assert rc == edgpu.OUT_OVERFLOW, short
            assert (res.bytes, res.frames, res.streams) == (need_bytes, need_frames, 3)
            assert np.all(buf == 0xA5) and not frames["bytes"].any() and not streams["bytes"].any()
        frames = np.zeros(need_frames, dtype=edgpu.AAC_FRAME_DTYPE)
        streams = np.zeros(3, dtype=edgpu.AAC_STREAM_DTYPE)
        rc, res = c.aac_tap_drain_raw(0, buf.ctypes.data, need_bytes, edgpu.PTR_HOST, frames, streams)
        assert rc == edgpu.OK and (res.bytes, res.frames, res.streams) == (need_bytes, need_frames, 3)
        got = split(buf, frames, streams)
        for (s, _), w in zip(sess, want):
            same(got[(s, 0)], w, "retry")
        assert np.all(buf[need_bytes:] == 0xA5)


# ---- 5. placement ----

def test_257_taps_cross_the_placement_block():
    with edgpu.Context(**SMALL) as c:
        sess = [add(c, HBR, ADTS if k % 3 else RAW) for k in range(257)]
        traces = [at.packetise([at.frame(1 + (k + 7 * j) % 60, k) for j in range((1 + k % 16) * (2 + k % 2))], max_aus=1 + k % 16, seq0=k)
                  for k in range(257)]
        assert all(len(t) == 2 + k % 2 for k, t in enumerate(traces))
        feed(c, {s: pk for (s, _), pk in zip(sess, traces)})
        data, frames, streams = c.aac_tap_drain()
        assert len(streams) == 257 and [int(x) for x in streams["session"]] == [s for s, _ in sess]
        got = split(data, frames, streams)
        for (s, m), pk in zip(sess, traces):
            for j, p in enumerate(pk):
                m.push(p, 1000 + j)
            same(got[(s, 0)], expect(m), f"session {s}")


# ---- 6. ring edges ----

def test_ring_wrap_lapped_ring_and_growth():
    with edgpu.Context(ring_growth=edgpu.FALSE, **TINY_RING) as c:
        s, m = add(c)
        seq = 65000
        for tick in range(26):                      # 26 x 5 packets of ~1.3 kB: two laps of both rings
            frames = [at.frame(1290 - tick - j, tick) for j in range(4)] + [at.frame(2500 + tick)]
            pk = at.packetise(frames, mtu=1400, seq0=seq, ts0=1024 * 5 * tick)[:5]
            seq += len(pk)
            feed(c, {s: pk}, t0=1000 * tick)
            for k, p in enumerate(pk):
                m.push(p, 1000 * tick + k)
            same(drain(c)[(s, 0)], expect(m), f"tick {tick}")
        assert m.c["missed"] == 0 and m.c["packets"] == 129 and m.c["frames"] >= 100      # the last tick's fragment waits
        s2, m2 = add(c)
        pk = [one(300 + k, 40 + k % 7) for k in range(100)]        # one batch laps the ring: the last 64 are left
        feed(c, {s2: pk})
        for k, p in enumerate(pk):
            m2.push(p, 1000 + k)
        m2.lose(36)
        got = drain(c)
        same(got[(s2, 0)], expect(m2), "lapped ring")
        assert m2.c["missed"] == 36 and got[(s2, 0)][1][0]["flags"] & DISCONT
    with edgpu.Context(**dict(TINY_RING, other_ring_packets=16, other_ring_bytes=16 << 10)) as c:
        s, m = add(c)                                               # enabled on a 16-packet ring, which then grows
        subscriber = c.subscriber_add(s, edgpu.TRANSPORT_UDP)
        seq = 0
        for tick in range(12):
            pk = [one(seq + k, 200 + k) for k in range(12)]
            seq += 12
            feed(c, {s: pk}, t0=100 * tick)
            c.fanout(100 * tick + 50)
            c.sync()
            for k, p in enumerate(pk):
                m.push(p, 100 * tick + k)
            same(drain(c)[(s, 0)], expect(m), f"growing, tick {tick}")
            if c.counters()["ring_grows"]:
                break
        assert c.counters()["ring_grows"] and subscriber is not None
        pk = [one(seq + k, 100 + k) for k in range(30)]             # more entries than the ring had at the enable
        feed(c, {s: pk}, t0=5000)
        for k, p in enumerate(pk):
            m.push(p, 5000 + k)
        got = drain(c)[(s, 0)]
        same(got, expect(m), "after growth")
        assert got[2]["missed"] == 0 and len(got[1]) == 30


# ---- 7. coexistence and lifecycle ----

def test_h264_tap_on_the_same_session_is_undisturbed():
    video, _ = tt.packetise([[tt.nal(7, 20), tt.nal(8, 6), tt.nal(5, 3000)], [tt.nal(1, 700)], [tt.nal(1, 90)]], mtu=500, seq0=5)
    audio = at.packetise([at.frame(100 + k) for k in range(20)], mtu=400) + chain(900, 250, 500)
    results = {}
    for order in ("alone", "video first", "audio first"):
        with edgpu.Context(**SMALL) as c:
            s = c.session_add(make_sdp(AV))
            c.session_ssrc_prefs(s, False, 30)
            c.tap_enable(s, 0)
            with pytest.raises(edgpu.EdgpuError) as e:
                c.aac_tap_enable(s, 0, config())                    # the video track is refused
            assert e.value.code == edgpu.BAD_ARGUMENT
            m = AacModel()
            if order != "alone":
                c.aac_tap_enable(s, 1, config())                    # "mpeg4-generic/...": the name in any case
            c.ingest_host(*edgpu.build_batch([(s, 0, 1000 + k, p) for k, p in enumerate(video)] +
                                             [(s, 2, 1000 + k, p) for k, p in enumerate(audio)]))
            c.keyframe_index()
            c.sync()
            if order == "audio first":
                a = drain(c)
            d, u, st = c.tap_drain()
            if order == "video first":
                a = drain(c)
            assert len(st) == 1 and int(st[0]["offset"]) == 0 and len(d) == (int(st[0]["bytes"]) + 15) // 16 * 16
            results[order] = (bytes(d[:int(st[0]["bytes"])]), u.tobytes(), st.tobytes())    # (the padding is not written)
            if order != "alone":
                for k, p in enumerate(audio):
                    m.push(p, 1000 + k)
                same(a[(s, 1)], expect(m), order)
                assert m.c["frames"] == 21
    vm = TapModel()
    for k, p in enumerate(video):
        vm.push(p, 1000 + k)
    want = vm.drain()[0]
    assert results["alone"][0] == want
    assert results["video first"] == results["alone"] == results["audio first"]


def test_lifecycle():
    with edgpu.Context(**SMALL) as c:
        assert c.aac_tap_drain()[0].size == 0 and c.kernel_times(9) == []      # no tap: nothing recorded
        s, m = add(c)
        feed(c, {s: [one(1), one(2)] + chain(50, 20, 3)[:1]})
        g = drain(c)[(s, 0)]
        assert g[2] == dict(dict.fromkeys(COUNTERS, 0), packets=2, frames=2) and c.kernel_times(9)
        c.aac_tap_enable(s, 0, config(framing=RAW))                 # enabling again resets it
        assert drain(c, flush=True)[(s, 0)] == (b"", [], dict.fromkeys(COUNTERS, 0))
        feed(c, {s: [one(99, 8)]})
        g = drain(c)[(s, 0)]
        assert g[0] == at.frame(8, 99) and g[1][0]["flags"] == 0 and g[2]["packets"] == 1    # no gap against the state before
        assert (s, 0) in c.aac_taps
        c.session_remove(s)
        assert drain(c) == {} and c.aac_taps == {}
        s2, _ = add(c, tap=False)                                   # the reused slot starts clean
        assert s2 == s and drain(c) == {}
        c.aac_tap_enable(s2, 0, config())
        feed(c, {s2: [one(5)]})
        assert drain(c)[(s2, 0)][2] == dict(dict.fromkeys(COUNTERS, 0), packets=1, frames=1)
        c.aac_tap_disable(s2, 0)
        c.aac_tap_disable(s2, 0)
        pcm = c.session_add(make_sdp([TrackSpec("audio", "PCMA/8000", 8), TrackSpec("audio", "MPEG4-GENERICX/44100", 97)]))
        for bad in ((pcm, 0, config()), (pcm, 1, config()), (s2, 1, config()), (1 << 20, 0, config()),
                    (s2, 0, edgpu.AacConfig(3, 0, 2, 4, 2, 0)), (s2, 0, edgpu.AacConfig(HBR, 3, 2, 4, 2, 0)),
                    (s2, 0, edgpu.AacConfig(HBR, 0, 5, 4, 2, 0)), (s2, 0, edgpu.AacConfig(HBR, 0, 0, 4, 2, 0)),
                    (s2, 0, edgpu.AacConfig(HBR, 0, 2, 13, 2, 0)), (s2, 0, edgpu.AacConfig(HBR, 0, 2, 4, 0, 0)),
                    (s2, 0, edgpu.AacConfig(HBR, 0, 2, 4, 8, 0))):
            with pytest.raises(edgpu.EdgpuError) as e:
                c.aac_tap_enable(*bad)
            assert e.value.code == edgpu.BAD_ARGUMENT, bad[:2]
        assert drain(c) == {}


# ---- 8. round trip, no model ----

def test_round_trip_without_the_model(ctx):
    lengths = list(range(1, 8185, 37)) + [8184]
    cases = {}
    for name, kw in (("mtu 1400", dict(mtu=1400)), ("mtu 100", dict(mtu=100)), ("cc", dict(mtu=1400, cc=2)), ("alone", dict(mtu=1400, max_aus=1))):
        frames = [at.frame(n, len(cases)) for n in lengths if kw["mtu"] > 100 or n < 700 or n == 8184]   # (the ring holds 2048 packets)
        s, _ = add(ctx)
        cases[name] = (s, frames, at.packetise(frames, seq0=65000, **kw))
    lb = [at.frame(n, 9) for n in range(1, 64)]
    s, _ = add(ctx, LBR)
    cases["lbr"] = (s, lb, at.packetise(lb, hbr=False, mtu=1400))
    feed(ctx, {s: pk for s, _, pk in cases.values()})
    got = drain(ctx)
    for name, (s, frames, pk) in cases.items():
        b, rows, c = got[(s, 0)]
        assert adts_reader.read(b) == (1, 4, 2, frames), name
        assert b[:4] == bytes.fromhex("FFF15080") if len(frames[0]) < 2048 else True
        assert c == dict(dict.fromkeys(COUNTERS, 0), packets=len(pk), frames=len(frames)), name
        assert [r["rtp_ts"] for r in rows] == [1024 * k for k in range(len(frames))], name
        ctx.aac_tap_disable(s, 0)
