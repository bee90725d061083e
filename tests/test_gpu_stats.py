"""GPU: per-stream reception statistics and the reference bitrate (edgpu_stream_stats_*,
edgpu_stats.hip) against tests/stats_model.py over the packets each test generates itself.

The shapes are the smallest at which k_stream_stats can go wrong: its rounds are 64 packets, so
batches of 1 / 63 / 64 / 65 / 128 / 129, state carried across launches at every cut of a
129-packet run, irregular packets at lanes 0, 1, 31, 63 and at the first lane of the next round
(the entry and exit of the closed-form round), and a 64-packet ring that wraps."""
import os
import struct
import subprocess

import numpy as np
import pytest

from easydarwin_amd import edgpu
from easydarwin_amd.synth import TrackSpec, make_sdp
from stats_model import FIELDS, SessionModel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H264 = [TrackSpec("video", "H264/90000", 96)]
AV = [TrackSpec("video", "H264/90000", 96), TrackSpec("audio", "MPEG4-GENERIC/44100/2", 97)]
SMALL = dict(max_batch_packets=1 << 15, max_batch_bytes=32 << 20, out_arena_bytes=32 << 20, max_out_packets=1 << 16)


def rtp(seq, ts=0, ssrc=0x11223344, size=40, fill=0x41):
    return struct.pack(">BBHII", 0x80, 96, seq & 0xFFFF, ts & 0xFFFFFFFF, ssrc & 0xFFFFFFFF) + bytes([fill]) * (size - 12)


def sr(ssrc, ntp, rtp_ts, pkts, octets, pt=200, size=28):
    b = struct.pack(">BBHIQIII", 0x80, pt, 6, ssrc, ntp, rtp_ts, pkts, octets) + bytes(24)
    return b[:size]


def names(tracks):
    return [t.payload for t in tracks]


def record(row):
    return {k: int(row[k]) for k in FIELDS}


def check(ctx, sess, model, what=""):
    got = [record(r) for r in ctx.stream_stats(sess)]
    want = model.records()
    assert len(got) == len(want)
    for t, (g, w) in enumerate(zip(got, want)):
        diff = {k: (g[k], w[k]) for k in FIELDS if g[k] != w[k]}
        assert not diff, f"{what} session {sess} track {t}: (engine, model) {diff}"


def ingest(ctx, pkts):
    """pkts: [(session, channel, arrival, bytes)]"""
    ctx.ingest_host(*edgpu.build_batch(pkts))
    ctx.keyframe_index()


def add(ctx, tracks, udp_push=False, now=0, ssrc_filter=False):
    s = ctx.session_add(make_sdp(tracks), udp_push=udp_push)
    if not ssrc_filter:
        ctx.session_ssrc_prefs(s, False, 30)
    ctx.stream_stats_enable(s, now)
    return s, SessionModel(names(tracks), udp_push, now)


def in_order(n, seq0=1000, t0=1_000_000, ts0=5000, size=40):
    return [(0, t0 + 40 * i, rtp(seq0 + i, ts0 + 3600 * i, size=size)) for i in range(n)]


@pytest.fixture(scope="module")
def ctx():
    with edgpu.Context(**SMALL) as c:
        yield c


# ---- 1. round boundaries and carry ----

@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 129])
def test_batch_sizes_around_the_round(ctx, n):
    s, m = add(ctx, H264)
    # two batches of n: the second runs the closed-form rounds (the first packet of a stream never does)
    for b in range(2):
        pk = in_order(n, seq0=65536 - 70 + b * n, t0=1_000_000 + 40 * n * b, ts0=3600 * n * b)
        ingest(ctx, [(s, ch, t, d) for ch, t, d in pk])
        for ch, t, d in pk:
            m.push(ch, t, d)
        check(ctx, s, m, f"n={n} batch {b}")
    assert int(ctx.stream_stats(s)[0]["received"]) == 2 * n


def test_state_carried_across_every_cut(ctx):
    pk = in_order(129, seq0=65500)
    rng = np.random.default_rng(3)
    pk = [(ch, t + int(rng.integers(0, 30)), d) for ch, t, d in pk]           # jitter carries too
    sess = [add(ctx, H264) for _ in range(128)]
    ingest(ctx, [(s, ch, t, d) for k, (s, _) in enumerate(sess) for ch, t, d in pk[:k + 1]])
    ingest(ctx, [(s, ch, t, d) for k, (s, _) in enumerate(sess) for ch, t, d in pk[k + 1:]])
    want = SessionModel(names(H264), False, 0)
    for ch, t, d in pk:
        want.push(ch, t, d)
    assert want.records()[0]["jitter_scaled"] > 0
    for s, _ in sess:
        check(ctx, s, want, "cut")


def test_four_ingest_paths_give_equal_records(ctx):
    rng = np.random.default_rng(5)
    pk = [(0, 2_000_000 + 33 * i + int(rng.integers(0, 20)), rtp(65400 + i, 90 * 33 * i, size=int(rng.integers(12, 1400))))
          for i in range(200)]
    pk += [(1, 2_000_000 + 33 * 200, sr(7, 99, 3, 200, 5000))]
    want = SessionModel(names(H264), False, 0)
    for ch, t, d in pk:
        want.push(ch, t, d)
    halves = [pk[:77], pk[77:]]

    # host
    s, _ = add(ctx, H264)
    for h in halves:
        ingest(ctx, [(s, ch, t, d) for ch, t, d in h])
    check(ctx, s, want, "host")
    # pinned and device
    for kind in ("pinned", "device"):
        s, _ = add(ctx, H264)
        for h in halves:
            arrays = edgpu.build_batch([(s, ch, t, d) for ch, t, d in h])
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
            ctx.sync()
            for b in bufs:
                b.free()
        check(ctx, s, want, kind)
    # a TCP byte stream, one read per frame (a frame's arrival is its read's)
    s, _ = add(ctx, H264)
    for h in halves:
        frames = [b"$" + bytes([ch]) + len(d).to_bytes(2, "big") + d for ch, t, d in h]
        reads = np.zeros(len(h), dtype=edgpu.TCP_READ_DTYPE)
        off = 0
        for i, (f, (ch, t, d)) in enumerate(zip(frames, h)):
            reads[i] = (s, len(f), off, t)
            off += len(f)
        res = ctx.ingest_interleaved(reads, b"".join(frames))
        assert int(res["frames"].sum()) == len(h)
        ctx.keyframe_index()
    check(ctx, s, want, "interleaved")


# ---- 2. the sequence machine at lane positions ----

def seq_patterns():
    P = {}
    for p in (0, 1, 31, 63, 64):                    # seq 0 lands at round 1 lane p (p = 64: round 2 lane 0)
        P[f"wrap@{p}"] = [(65536 - (64 + p) + i) & 0xFFFF for i in range(200)]
    base = list(range(100, 300))
    for drop in (5, 63, 64, 127, 128):
        P[f"loss@{drop}"] = base[:drop] + base[drop + 1:]
    for gap in (2999, 3000, 3001):
        P[f"gap{gap}+successor"] = base[:70] + [base[69] + gap + i for i in range(70)]
        P[f"gap{gap}-alone"] = base[:70] + [base[69] + gap] + base[70:140]
    for behind in (1, 99, 100, 101):
        P[f"misorder{behind}"] = list(range(1000, 1150)) + [1149 - behind] + list(range(1150, 1220))
    for at in (10, 63, 64, 65, 127):
        P[f"dup@{at}"] = base[:at] + [base[at - 1]] + base[at:150]
    P["irregular@63"] = base[:64 + 63] + [base[64 + 62]] + base[64 + 63:64 + 130]     # 63 regular, then a duplicate
    P["irregular@0"] = base[:64] + [base[63]] + base[64:64 + 130]                     # a duplicate, then 63 regular
    return P


def test_sequence_machine_at_lane_positions(ctx):
    pats = seq_patterns()
    sess = {}
    batch = []
    for name, seqs in pats.items():
        s, m = add(ctx, H264)
        sess[name] = (s, m)
        for i, q in enumerate(seqs):
            t, d = 3_000_000 + 20 * i, rtp(q, 1800 * i)
            batch.append((s, 0, t, d))
            m.push(0, t, d)
    ingest(ctx, batch)
    for name, (s, m) in sess.items():
        check(ctx, s, m, name)
    r = {n: record(ctx.stream_stats(s)[0]) for n, (s, _) in sess.items()}
    assert all(r[f"wrap@{p}"]["cycles"] == 65536 and r[f"wrap@{p}"]["lost"] == 0 for p in (0, 1, 31, 63, 64))
    assert [r[f"gap{g}+successor"]["restarts"] for g in (2999, 3000, 3001)] == [0, 1, 1]
    assert [r[f"misorder{b}"]["misordered"] for b in (1, 99, 100, 101)] == [1, 1, 0, 0]
    assert r["loss@63"]["lost"] == 1 and r["dup@64"]["lost"] == -1


# ---- 3. jitter ----

@pytest.mark.parametrize("payload", ["H264/90000", "PCMA/8000", "MPEG4-GENERIC/44100/2", "H264"])
def test_jitter_random_arrivals(ctx, payload):
    tracks = [TrackSpec("video", payload, 96)]
    s, m = add(ctx, tracks)
    rng = np.random.default_rng(11)
    t = 1_700_000_000_000                           # arrival_ms * clock_rate passes 2^32 (and 2^48)
    batch = []
    for i in range(300):
        t += int(rng.integers(0, 60))
        # the timestamp wraps at packet 41 (round 0 of the first launch, walked packet by packet) and,
        # after a jump at packet 150, again at packet 180: lane 50 of the second launch's first round,
        # a closed-form round (its 64 packets are regular; only their timestamps are not)
        ts = 0xFFFFFFFF - 40 * 3000 + 3000 * i if i < 150 else 0xFFFFFFFF - 30 * 3000 + 3000 * (i - 150)
        d = rtp(200 + i, ts)
        batch.append((s, 0, t, d))
        m.push(0, t, d)
    ingest(ctx, batch[:130])
    ingest(ctx, batch[130:])
    check(ctx, s, m, payload)
    assert (m.records()[0]["jitter_scaled"] > 0) == ("/" in payload)


# ---- 4. lengths ----

def test_lengths_around_the_rtp_header(ctx):
    s, m = add(ctx, H264)
    batch = []
    for i, n in enumerate(list(range(1, 25)) * 6):
        for d in (rtp(2 * i, 0, size=max(n, 12))[:n], rtp(2 * i + 1, 0, size=1400)):
            batch.append((s, 0, 10 + i, d))
    batch.append((s, 0, 500, rtp(999, 0, size=2061)))
    batch.append((s, 0, 500, rtp(1000, 0, size=3000)))           # clamped to 2060
    for _, ch, t, d in batch:
        m.push(ch, t, d)
    ingest(ctx, batch)
    check(ctx, s, m, "lengths")
    r = record(ctx.stream_stats(s)[0])
    assert r["short_packets"] == 11 * 6 and r["bytes"] == m.tracks[0].bytes


def test_ssrc_filter_hides_a_second_ssrc_and_without_it_the_stream_restarts(ctx):
    trace = [(0, 1000 + 20 * i, rtp(100 + i, 0, ssrc=0xAAAA0001)) for i in range(70)]
    trace += [(0, 2400 + 20 * i, rtp(9000 + i, 0, ssrc=0xBBBB0002)) for i in range(70)]     # 1.4 s later: inside 30 s
    # use_one_SSRC_per_stream: the filter empties the second SSRC's packets
    s, m = add(ctx, H264, ssrc_filter=True)
    ingest(ctx, [(s, ch, t, d) for ch, t, d in trace])
    for ch, t, d in trace:
        m.push(ch, t, d if d[8:12] == trace[0][2][8:12] else b"")
    check(ctx, s, m, "filter on")
    r = record(ctx.stream_stats(s)[0])
    assert (r["packets"], r["ssrc_changes"], r["ssrc"]) == (70, 0, 0xAAAA0001)
    # filter off: every packet arrives, the second SSRC restarts the sequence state
    s, m = add(ctx, H264, ssrc_filter=False)
    ingest(ctx, [(s, ch, t, d) for ch, t, d in trace])
    for ch, t, d in trace:
        m.push(ch, t, d)
    check(ctx, s, m, "filter off")
    r = record(ctx.stream_stats(s)[0])
    assert (r["packets"], r["ssrc_changes"], r["base_seq"], r["received"]) == (140, 1, 9000, 70)


# ---- 5. RTCP ----

def test_sender_reports(ctx):
    s, m = add(ctx, H264)
    rt = [sr(1, 10, 11, 12, 13, size=27), sr(2, 20, 21, 22, 23, size=28), sr(3, 30, 31, 32, 33, size=52),
          sr(4, 40, 41, 42, 43, pt=201)]
    b1 = [(1, 100 + i, d) for i, d in enumerate(rt)]                                      # last SR: the 52-byte one
    fill = [(1, 300 + i, bytes([0x80, 201, 0, 1, 0, 0, 0, i])) for i in range(70)]
    b2 = [(1, 299, sr(5, 50, 51, 52, 53))] + fill                                         # SR first of a batch
    b3 = fill[:30] + [(1, 400, sr(6, 60, 61, 62, 63))] + fill[30:]                        # interior
    b4 = fill + [(1, 500, sr(7, 70, 71, 72, 73))]                                         # last, in round 1
    b5 = fill[:5] + [(1, 600, sr(8, 80, 81, 82, 83)), (1, 601, sr(9, 90, 91, 92, 93))] + fill[:5]    # two in a round
    for k, b in enumerate((b1, b2, b3, b4, b5)):
        ingest(ctx, [(s, ch, t, d) for ch, t, d in b])
        for ch, t, d in b:
            m.push(ch, t, d)
        check(ctx, s, m, f"rtcp batch {k}")
    r = record(ctx.stream_stats(s)[0])
    assert (r["sr_count"], r["sr_ntp"], r["sr_rtp"], r["sr_packets"], r["sr_octets"], r["sr_arrival_ms"]) == (7, 90, 91, 92, 93, 601)


def test_bitrate_counts_rtp_by_port_parity(ctx):
    pk = [(0, 10 + i, rtp(i, 0, size=100)) for i in range(10)] + [(1, 30 + i, sr(1, i, i, i, i)) for i in range(3)]
    got = {}
    for udp in (True, False):
        s, m = add(ctx, H264, udp_push=udp)
        ingest(ctx, [(s, ch, t, d) for ch, t, d in pk])
        for ch, t, d in pk:
            m.push(ch, t, d)
        check(ctx, s, m, f"udp_push={udp}")
        got[udp] = int(ctx.stream_stats(s)[0]["interval_bytes"])
    assert got == {True: 1000, False: 1000 + 3 * 28}


# ---- 6. ring wrap ----

def test_ring_wrap_and_growth():
    small = dict(SMALL, video_ring_packets=64, video_ring_bytes=64 << 10, other_ring_packets=64, other_ring_bytes=64 << 10)
    with edgpu.Context(ring_growth=edgpu.FALSE, **small) as c:
        s, m = add(c, H264)
        c.subscriber_add(s, edgpu.TRANSPORT_UDP)
        seq = 65000
        for tick in range(8):                       # 8 x 32 packets of ~1.4 kB: 4 x the meta ring, 5.6 x the byte ring
            pk = [(0, 1000 + 40 * tick + i, rtp(seq + i, 90 * (40 * tick + i), size=1400 + (i % 7))) for i in range(32)]
            seq += 32
            ingest(c, [(s, ch, t, d) for ch, t, d in pk])
            for ch, t, d in pk:
                m.push(ch, t, d)
            c.fanout(1000 + 40 * tick + 39)
            assert c.stats().status == 0
        check(c, s, m, "wrapping ring")
        assert record(c.stream_stats(s)[0])["missed"] == 0
        # The engine accepts a single batch that laps a ring (the oldest packets are overwritten
        # before anything reads them): 100 small packets into the 64-entry ring leave the last 64,
        # the statistics cover those and count the other 36 as missed.
        s2, m2 = add(c, H264)
        pk = [(0, 5000 + i, rtp(300 + i, 90 * i)) for i in range(100)]
        ingest(c, [(s2, ch, t, d) for ch, t, d in pk])
        for ch, t, d in pk[36:]:
            m2.push(ch, t, d)
        m2.tracks[0].missed = 36
        check(c, s2, m2, "lapped ring")
    with edgpu.Context(**small) as c:               # growth on: the rings grow between two batches
        s, m = add(c, H264)
        c.subscriber_add(s, edgpu.TRANSPORT_UDP)
        grows0 = c.counters()["ring_grows"]
        for tick in range(6):
            pk = [(0, 1000 + 10 * tick + (i % 10), rtp(tick * 40 + i, 900 * tick, size=1000)) for i in range(40)]
            ingest(c, [(s, ch, t, d) for ch, t, d in pk])
            for ch, t, d in pk:
                m.push(ch, t, d)
            c.fanout(1000 + 10 * tick + 9)
            assert c.stats().status == 0
        assert c.counters()["ring_grows"] > grows0
        check(c, s, m, "growing ring")


# ---- 7. many streams ----

def test_many_streams_only_odd_sessions_enabled(ctx):
    pats = list(seq_patterns().values())
    rng = np.random.default_rng(23)
    sess, batch = [], []
    for k in range(64):
        s = ctx.session_add(make_sdp(AV))
        ctx.session_ssrc_prefs(s, False, 30)
        m = None
        if k % 2:
            ctx.stream_stats_enable(s, 0)
            m = SessionModel(names(AV), False, 0)
        sess.append((s, m))
        t = 4_000_000
        for i, q in enumerate(pats[k % len(pats)]):
            t += int(rng.integers(0, 50))
            for ch, d in ((0, rtp(q + k, 3000 * i, ssrc=k + 1, size=60 + k)), (2, rtp(q ^ 0x5555, 1024 * i, ssrc=1000 + k))):
                batch.append((s, ch, t, d))
                if m:
                    m.push(ch, t, d)
            if i % 50 == 0:
                d = sr(k, i, i + 1, i + 2, i + 3)
                batch.append((s, 1, t, d))
                if m:
                    m.push(1, t, d)
    ingest(ctx, batch)
    for k, (s, m) in enumerate(sess):
        if m:
            check(ctx, s, m, f"session {k}")
        else:
            with pytest.raises(edgpu.EdgpuError) as e:
                ctx.stream_stats(s)
            assert e.value.code == edgpu.ERR and "not enabled" in str(e.value)


# ---- 8. bitrate ----

BITRATE_T0 = 1_000_000


def bitrate_script():
    """(time, packets pushed before the tick at that time)"""
    a = [(0, BITRATE_T0 + 10 * i, rtp(i, 900 * i, size=1000)) for i in range(100)] + \
        [(2, BITRATE_T0 + 10 * i, rtp(i, 80 * i, size=172)) for i in range(100)] + \
        [(1, BITRATE_T0 + 500, sr(1, 2, 3, 4, 5))]
    b = [(0, BITRATE_T0 + 40000 + 10 * i, rtp(100 + i, 900 * (4000 + i), size=700)) for i in range(150)]
    return [(BITRATE_T0 + 30000, a), (BITRATE_T0 + 30001, []), (BITRATE_T0 + 30002, []), (BITRATE_T0 + 60001, b),
            (BITRATE_T0 + 60002, [])]


def test_bitrate_samples(ctx):
    av = [TrackSpec("video", "H264/90000", 96), TrackSpec("audio", "PCMA/8000", 8)]
    s, m = add(ctx, av, now=BITRATE_T0)
    seen = []
    for now, pk in bitrate_script():
        if pk:
            ingest(ctx, [(s, ch, t, d) for ch, t, d in pk])
        for ch, t, d in pk:
            m.push(ch, t, d)
        ctx.stream_stats_sample(now)
        m.sample(now)
        check(ctx, s, m, f"sample at {now}")
        rows = ctx.stream_stats(s)
        assert ctx.session_bitrate(s) == int(rows["bitrate"].sum()) == m.bitrate()
        seen.append(ctx.session_bitrate(s))
    # 30000 ms after enable: no sample; 1 ms later: (100 * 1000 + 28) * 8 and 100 * 172 * 8 bits over
    # 30001 ms; 30000 ms after that sample: none again; 1 ms later: 150 * 700 * 8 bits over 30001 ms
    # (and nothing on the audio track)
    assert seen == [0, 26673 + 4586, 26673 + 4586, 26673 + 4586, 27999]
    assert seen[4] == int(np.float32(np.float32(150 * 700 * 8) / np.float32(30001)) * np.float32(1000))


# ---- 9. no behaviour change ----

class StatsContext(edgpu.Context):
    """mode "on": statistics on for every session, a sample call per tick; "touched": every
    session enabled and disabled again, the sample call made all the same; "never": neither.
    Counts the ingests and sample calls made while a session was enabled."""

    def __init__(self, mode="on", **cfg):
        super().__init__(**cfg)
        self.mode, self.enabled, self.stat_launches = mode, set(), 0

    def session_add(self, sdp, udp_push=False):
        s = super().session_add(sdp, udp_push=udp_push)
        if self.mode != "never":
            self.stream_stats_enable(s, 0)
            self.enabled.add(s)
        if self.mode == "touched":
            self.stream_stats_disable(s)
            self.enabled.discard(s)
        return s

    def session_remove(self, session, kill_outputs=False):
        super().session_remove(session, kill_outputs=kill_outputs)
        self.enabled.discard(session)

    def _launched(self):
        self.stat_launches += 1 if self.enabled else 0

    def ingest_host(self, *a):
        super().ingest_host(*a)
        self._launched()

    def ingest_pinned(self, *a):
        super().ingest_pinned(*a)
        self._launched()

    def ingest_interleaved(self, reads, data, device_ptr=None):
        r = super().ingest_interleaved(reads, data, device_ptr)
        if len(reads):
            self._launched()
        return r

    def fanout(self, now_ms):
        if self.mode != "never":
            self.stream_stats_sample(now_ms)
            self._launched()
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


@pytest.mark.parametrize("name", ["mixed", "backpressure"])
def test_goldens_unchanged_with_statistics_enabled(name):
    from easydarwin_amd.replay import replay
    from scenarios import SCENARIOS
    import hashlib
    import json
    # the committed reference capture of the scenario, by its hash (as tests/test_gpu_parity.py)
    want = json.load(open(os.path.join(ROOT, "tests", "golden", name + ".json")))["capture_sha256"]
    trace = SCENARIOS[name]()
    plain, _ = replay(trace)
    assert hashlib.sha256(plain).hexdigest() == want
    cfg = replay_cfg(trace)
    with StatsContext(**cfg) as c:
        got, _ = replay(trace, ctx=c)
        assert any(int(r["packets"]) for s in range(len(trace.sdps)) for r in c.stream_stats(s))
    assert got == plain and hashlib.sha256(got).hexdigest() == want


@pytest.mark.parametrize("name,how", [("mixed", {}), ("mixed", {"pinned": True}), ("anchor", {"interleaved": 1})],
                         ids=["host", "pinned", "interleaved"])
def test_kernel_launches_over_a_replay(name, how):
    """A golden replayed -- `mixed` with host and with pinned ingest (its joins, leaves and session
    ends), `anchor` as RTSP-interleaved byte streams (`mixed` has packets no interleaved frame
    can carry) -- in a context that never touched the statistics, in one where every session was
    enabled and disabled again, and in one with every session enabled: the first two launch the
    same number of kernels, the third exactly one more per ingest and one more per sample call
    made while a session was enabled.  The captures are equal."""
    from easydarwin_amd.replay import replay
    from scenarios import SCENARIOS
    trace = SCENARIOS[name]()
    out = {}
    for mode in ("never", "touched", "on"):
        with StatsContext(mode, **replay_cfg(trace)) as c:
            cap, _ = replay(trace, ctx=c, **how)
            out[mode] = (c.counters()["kernel_launches"], c.stat_launches, cap, c.kernel_times(4))
    assert out["never"][2] == out["touched"][2] == out["on"][2]
    assert out["never"][0] == out["touched"][0] and out["never"][1] == out["touched"][1] == 0
    assert out["never"][3] == out["touched"][3] == []
    assert out["on"][1] >= 2 and out["on"][0] == out["never"][0] + out["on"][1]      # an ingest and a sample at least
    assert out["on"][3] and min(out["on"][3]) >= 0.0


# ---- 10. lifecycle ----

def test_lifecycle(ctx):
    s, m = add(ctx, H264)
    pk = in_order(70)
    ingest(ctx, [(s, ch, t, d) for ch, t, d in pk])
    assert int(ctx.stream_stats(s)[0]["received"]) == 70
    ctx.stream_stats_enable(s, 5)                   # enabling again resets; statistics start at the next packet
    r = record(ctx.stream_stats(s)[0])
    assert (r["packets"], r["received"], r["has_src"], r["last_sample_ms"], r["expected"]) == (0, 0, 0, 5, 0)
    ingest(ctx, [(s, 0, 9_000_000, rtp(7, 0))])
    assert int(ctx.stream_stats(s)[0]["packets"]) == 1
    ctx.stream_stats_disable(s)
    with pytest.raises(edgpu.EdgpuError) as e:
        ctx.stream_stats(s)
    assert e.value.code == edgpu.ERR
    with pytest.raises(edgpu.EdgpuError) as e:
        ctx.session_bitrate(s)
    assert e.value.code == edgpu.ERR
    ctx.stream_stats_enable(s, 6)
    ctx.session_remove(s)
    s2 = ctx.session_add(make_sdp(H264))            # the removed session's id and rows
    assert s2 == s
    with pytest.raises(edgpu.EdgpuError) as e:
        ctx.stream_stats(s2)
    assert e.value.code == edgpu.ERR
    ingest(ctx, [(s2, 0, 9_000_100, rtp(1, 0))])    # disabled: not counted
    ctx.stream_stats_enable(s2, 7)
    r = record(ctx.stream_stats(s2)[0])
    assert (r["packets"], r["bytes"], r["received"], r["interval_bytes"], r["last_sample_ms"]) == (0, 0, 0, 0, 7)
    for call in (lambda: ctx.stream_stats_enable(1 << 20, 0), lambda: ctx.stream_stats_disable(1 << 20),
                 lambda: ctx.stream_stats(1 << 20), lambda: ctx.session_bitrate(1 << 20)):
        with pytest.raises(edgpu.EdgpuError) as e:
            call()
        assert e.value.code == edgpu.BAD_ARGUMENT


def test_adapter_getters_agree_with_the_c_abi():
    """Reflector::EnableStreamStats / GetStreamStats / GetBitRate (tools/adapter_stats) on the
    bitrate case: both report what the model does, ReflectPackets(now) being the sample call."""
    av = [TrackSpec("video", "H264/90000", 96), TrackSpec("audio", "PCMA/8000", 8)]
    m = SessionModel(names(av), False, BITRATE_T0)
    lines = ["S 0 " + make_sdp(av).replace("\r\n", "|"), "O 0", f"E {BITRATE_T0}"]
    want = []
    for now, pk in bitrate_script():
        for ch, t, d in pk:
            lines.append(f"P {ch // 2} {ch & 1} {t} {d.hex()}")
            m.push(ch, t, d)
        lines.append(f"T {now}")
        m.sample(now)
        row = [now, m.bitrate()]
        for r in m.records():
            row += [r["packets"], r["bytes"], r["received"], r["jitter_scaled"], r["bitrate"], r["interval_bytes"], r["last_sample_ms"]]
        want.append(row)
    out = subprocess.run([os.path.join(ROOT, "tools", "adapter_stats")], input="\n".join(lines) + "\n", capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = [ln.split() for ln in out.stdout.splitlines()]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        k = g.index("abi")
        adapter, abi = [int(v) for v in g[2:k]], [int(v) for v in g[k + 1:]]
        assert g[1] == "adapter" and adapter == abi == w[1:], (g, w)
        assert int(g[0]) == w[0]
