"""Directed edge traces for the copy kernels (k_ingest's ring copy, k_fanout4 / k_fanout6): short
deterministic traces that put packets on the kernels' own edges rather than on the reflector's
behaviour.  Every generator returns ``(Trace, claims)``: the claims are the edge conditions the
trace reaches, computed here on the host from the packets it emitted with the engine's ring layout
(a sender's byte ring is a stream of 16-B words; a packet of ``len`` bytes takes
``(len + 4 + 15) / 16`` of them after the 2060-B clamp, edgpu_kernels.hip k_ingest).
tests/test_edge_traces.py asserts every claim and pins the restatement to the compiled reference
on each trace; tests/test_gpu_edges.py runs them through the engine.

Families (ISSUE "directed edge sweeps", docs/PARITY.md):

* A ``lenphase_*``    every RTP length 1..2061 (+ 3000, 65535) once, in a fixed permutation, so every
                      (ring word phase mod 8) x (len mod 16) pair is a slot start;
* B ``chunks_*``      per-tick packet counts around the kernels' CHUNK (16 / 32) multiples, and a
                      joining output whose window starts at every in-chunk position 0..33;
* C ``wrap_*``        A's lengths, twice, through a 64-KiB / 64-packet ring: chunks and single slots
                      straddling the ring end at every word phase;
* D ``neighbours_*``  one tick of >= 4096 work items whose neighbours differ 4x or more in words;
* E ``rewrite_edges`` the rewrite patch's length thresholds (RTP 12, RTCP 8, SR 20), SRs first /
                      last / interior in a chunk, sequence and timestamp carries;
* F ``aktt_near_capacity``  receive-time trailers stripped from most packets, sized so the ring
                      holds the stream at its stripped lengths only.
"""
from __future__ import annotations

import hashlib
import struct

import numpy as np

from easydarwin_amd.synth import SEED_BASE, TrackSpec, make_sdp, rtp_header
from easydarwin_amd.trace import JOIN, PKT, TCP, TICK, UDP, Trace
from scenarios import _aktt_tag, _assemble

MAX_PACKET = 2060                       # ReflectorPacket's buffer (Q11)
PLAIN, PATCHING = "k_fanout6<1024,16,", "k_fanout4<1024,32,"     # (edgpu_fanout_kernel prefixes)
CHUNK = {PLAIN: 16, PATCHING: 32}
SEED = SEED_BASE + 300


def slot_words(n: int) -> int:
    n = min(n, MAX_PACKET)
    return (n + 4 + 15) // 16 if n else 0


def _rng(k: int):
    return np.random.Generator(np.random.PCG64(SEED + k))


def _bytes(rng, n: int) -> bytes:
    return rng.integers(0, 256, size=max(n, 0), dtype=np.uint8).tobytes()


def _rtp(rng, seq: int, ts: int, ssrc: int, n: int, first: bytes = b"") -> bytes:
    """An RTP packet of exactly n bytes (a header cut short below 12), random payload."""
    return (rtp_header(seq, ts, ssrc, 96, False) + first + _bytes(rng, n - 12 - len(first)))[:n]


def kernel_of(tr: Trace, rewrite=None) -> str:
    """The fan-out kernel a trace's ticks run: the patching one as soon as any output is
    RTSP-interleaved or rewritten."""
    tcp = any(ev[0] == JOIN and ev[4] == TCP for ev in tr.events)
    return PATCHING if tcp or rewrite else PLAIN


def sender_ticks(tr: Trace, session: int = 0, channel: int = 0) -> list[list[int]]:
    """The relayed lengths of one sender's packets, per tick."""
    out, cur = [], []
    for ev in tr.events:
        if ev[0] == PKT and ev[2] == session and ev[3] == channel and len(ev[4]):
            cur.append(min(len(ev[4]), MAX_PACKET))
        elif ev[0] == TICK:
            out.append(cur)
            cur = []
    return out


def ring_layout(ticks: list[list[int]], chunk: int, ring_words: int = 0, ring_packets: int = 0) -> dict:
    """Walks a sender's ring as k_ingest fills it and k_plan_final cuts it (outputs that keep up:
    a tick's work items are its new packets in runs of `chunk`)."""
    word = pk = 0
    pairs, first_phase, chunk_wrap_phase = set(), set(), set()
    slot_wraps = pk_splits = wraps = 0
    items = []                                          # words per work item
    for lens in ticks:
        if lens:
            first_phase.add(word % 8)
        for c0 in range(0, len(lens), chunk):
            part = lens[c0:c0 + chunk]
            nw = sum(slot_words(n) for n in part)
            items.append(nw)
            if ring_words and word % ring_words + nw > ring_words:
                chunk_wrap_phase.add(word % ring_words % 8)
                wraps += 1
            if ring_packets and pk % ring_packets + len(part) > ring_packets:
                pk_splits += 1
            for n in part:
                pairs.add((word % 8, n % 16))
                if ring_words and word % ring_words + slot_words(n) > ring_words:
                    slot_wraps += 1
                word += slot_words(n)
                pk += 1
    return {"pairs": pairs, "tick_first_phases": first_phase, "chunk_wrap_phases": chunk_wrap_phase,
            "chunk_wraps": wraps, "slot_wraps": slot_wraps, "packet_ring_chunk_splits": pk_splits,
            "items": items, "words": word, "packets": pk,
            "max_tick_words": max((sum(slot_words(n) for n in t) for t in ticks), default=0),
            "max_tick_packets": max((len(t) for t in ticks), default=0)}


def sweep_lengths(max_len: int = 65535, zero: bool = False) -> list[int]:
    """Family A's lengths: 1..2061 once and the two clamped ones, in a fixed permutation."""
    lens = list(range(1, MAX_PACKET + 2)) + [3000, 65535] + ([0] if zero else [])
    lens = [n for n in lens if n <= max_len]
    return [lens[i] for i in _rng(1).permutation(len(lens))]


def _one_video_session(tr: Trace, name: str = "MP4V-ES/90000"):
    tr.add_session(make_sdp([TrackSpec("video", name, 96)]))


def _paced(lens, caps, gaps, byte_budget):
    """Cuts a length list into ticks: at most caps[k] packets and byte_budget slot bytes in tick k,
    gaps[k] ms after the last."""
    ticks, times, t, i, k = [], [], 0, 0, 0
    while i < len(lens):
        cur, b = [], 0
        while i < len(lens) and len(cur) < caps[k % len(caps)] and b + 16 * slot_words(lens[i]) <= byte_budget:
            b += 16 * slot_words(lens[i])
            cur.append(lens[i])
            i += 1
        t += gaps[k % len(gaps)]
        ticks.append(cur)
        times.append(t)
        k += 1
    return ticks, times


def _sweep_trace(lens, transports, caps, gaps, byte_budget, seed):
    rng = _rng(seed)
    tr = Trace()
    _one_video_session(tr)
    ticks, times = _paced(lens, caps, gaps, byte_budget)
    pk, seq = [], 0
    for cur, t in zip(ticks, times):
        for n in cur:
            pk.append((t, 0, _rtp(rng, 0x7F00 + seq, 3000 * seq, 0x5EED0A01, n)))
            seq += 1
    joins = [(0, 0, 1 + k, tp) for k, tp in enumerate(transports)]
    return _assemble(tr, [pk], 0, 0, joins, tick_times=times)


# ---- A: length x phase ---------------------------------------------------------------------------
A_CAPS = [29, 8, 35, 16, 41, 23, 32, 11]


def lenphase(mixed: bool):
    # (length 0 too: the reference takes the empty packet and relays nothing for it)
    tr = _sweep_trace(sweep_lengths(zero=True), [UDP, TCP] if mixed else [UDP, UDP], A_CAPS, [40], 1 << 30, 2)
    lay = ring_layout(sender_ticks(tr), CHUNK[kernel_of(tr)])
    return tr, {"kernel": kernel_of(tr), "pairs": lay["pairs"], "tick_first_phases": lay["tick_first_phases"],
                "packets": lay["packets"], "lengths": sorted(len(ev[4]) for ev in tr.events if ev[0] == PKT)}


# ---- B: chunk boundaries and in-chunk starts -----------------------------------------------------
B_COUNTS = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65]
B_JOIN_COUNT = 36


def chunks(tcp: bool):
    rng = _rng(3)
    tr = Trace()
    _one_video_session(tr, "H264/90000")
    pk, joins, times = [], [(0, 0, 1, UDP), (0, 0, 2, TCP if tcp else UDP)], []
    seq, t = 0, 0
    claims_joins = []

    def emit(count, key_at):
        nonlocal seq, t
        t += 40
        times.append(t)
        for k in range(count):
            nal = b"\x65" if k == key_at else b"\x41"
            p = _rtp(rng, seq, 3600 * len(times), 0x5EED0B01, int(rng.integers(20, 400)), first=nal)
            pk.append((t, 0, p))
            if k == key_at and times[-1] != 40:
                claims_joins[-1] += (hashlib.sha256(p).hexdigest(),)
            seq += 1

    for n in B_COUNTS:
        emit(n, 0 if n == 1 else -1)                    # the stream's first packet is its first IDR
    for p in range(34):
        sub = 100 + p
        claims_joins.append((sub, p))
        emit(B_JOIN_COUNT, p)
        joins.append((t, 0, sub, TCP if tcp and p % 2 else UDP))
    emit(20, -1)                                        # a tail every joiner relays too
    tr = _assemble(tr, [pk], 0, 0, joins, tick_times=times)
    kern = kernel_of(tr)
    per = sender_ticks(tr)
    return tr, {"kernel": kern, "counts": {(len(c), kern) for c in per},
                "starts": {(p, kern) for _, p, _ in claims_joins},
                "in_chunk_starts": {p % CHUNK[kern] for _, p, _ in claims_joins},
                "joins": claims_joins, "tail": 20}


# ---- C: ring wrap --------------------------------------------------------------------------------
C_RING_BYTES, C_RING_PACKETS = 65536, 64
C_CAPS = [17, 33, 40, 24, 31, 16, 32, 48]
C_GAPS = [20, 50, 30, 40, 25]
C_CFG = dict(video_ring_bytes=C_RING_BYTES, video_ring_packets=C_RING_PACKETS,
             other_ring_bytes=C_RING_BYTES, other_ring_packets=C_RING_PACKETS)


def wrap(mixed: bool, max_len: int = 65535):
    lens = sweep_lengths(max_len)
    tr = _sweep_trace(lens + lens[::-1], [UDP, TCP] if mixed else [UDP, UDP], C_CAPS, C_GAPS, 40 << 10, 4)
    kern = kernel_of(tr)
    lay = ring_layout(sender_ticks(tr), CHUNK[kern], C_RING_BYTES // 16, C_RING_PACKETS)
    keep = ("chunk_wrap_phases", "chunk_wraps", "slot_wraps", "packet_ring_chunk_splits", "max_tick_words",
            "max_tick_packets", "words")
    return tr, dict({k: lay[k] for k in keep}, kernel=kern, ring_words=C_RING_BYTES // 16,
                    max_len=max(len(ev[4]) for ev in tr.events if ev[0] == PKT))


# ---- D: many work items per workgroup, contrasting neighbours -------------------------------------
D_CFG = dict(video_ring_bytes=1 << 17, video_ring_packets=128, other_ring_bytes=4096, other_ring_packets=64)
D_REWRITE = (0x0101, 0x01020304, 0xD00D0001)


def neighbours(patching: bool):
    """Session s's chunk k is of kind (2s + k) % 3: all `big`-byte packets, all 1..20-byte ones, or
    mid sizes.  All-UDP: 1100 sessions x 4 chunks of 16; patching: 2100 sessions x 2 chunks of 32,
    each with a UDP, a TCP and a rewritten UDP player (smaller packets: three times the output)."""
    rng = _rng(5 + patching)
    nsess, nchunks, chunk, big, mid = (2100, 2, 32, 520, (60, 109)) if patching else (1100, 4, 16, MAX_PACKET, (124, 501))
    kind = (2 * np.arange(nsess)[:, None] + np.arange(nchunks)[None, :]) % 3
    kind = np.repeat(kind, chunk, axis=1)                           # [session, packet]
    lens = np.where(kind == 0, big, np.where(kind == 1, rng.integers(1, 21, size=kind.shape),
                                             rng.integers(*mid, size=kind.shape)))
    lens[:, 0] = np.maximum(lens[:, 0], 12)                         # a whole header first (the SSRC latch)
    pool = _bytes(rng, int(lens.sum()))                             # one draw: every payload byte random
    at = 0
    tr = Trace()
    per, joins, rewrite = [], [], {}
    for s in range(nsess):
        _one_video_session(tr)
        pk = []
        for q, n in enumerate(lens[s].tolist()):
            pk.append((1 + q // 16, 0, (rtp_header(q, 90 * q, 0xD0000000 + s, 96, False) + pool[at:at + n])[:n]))
            at += n
        per.append(pk)
        joins.append((0, s, 3 * s + 1, UDP))
        if patching:
            joins += [(0, s, 3 * s + 2, TCP), (0, s, 3 * s + 3, UDP)]
            rewrite[3 * s + 3] = D_REWRITE
    tr = _assemble(tr, per, 0, 0, joins, tick_times=[10])
    items = []                                          # sender-major, chunk-minor (k_plan_final)
    for row in lens.tolist():
        items += ring_layout([row], chunk)["items"]
    contrast = sum(1 for a, b in zip(items, items[1:]) if max(a, b) >= 4 * min(a, b))
    return tr, {"kernel": kernel_of(tr, rewrite), "nwork": len(items), "pairs": len(items) - 1,
                "contrast_pairs": contrast, "rewrite": rewrite}


# ---- E: rewrite thresholds -----------------------------------------------------------------------
E_RTCP_LENS = [4, 7, 8, 12, 19, 20, 28, 52]
E_REWRITE = {1: (0x1234, 0, 0xE0E00001), 2: (0, 0xF0000000, 0xE0E00002),          # session 0: UDP, TCP
             4: (0xFFFF, 0xFFFFFFFF, None), 5: (0x8001, 0x80000001, 0xE0E00005)}  # session 1: UDP, TCP


def _rtcp(rng, pt: int, n: int, ssrc: int) -> bytes:
    """An RTCP packet of n bytes: bytes 8-11 constant (a push over RTSP latches its SSRC filter on
    them, Q12), the rest random -- an SR's RTP timestamp (bytes 16-19) among them."""
    body = struct.pack(">BBHI", 0x80, pt, max(n // 4 - 1, 0), ssrc) + b"\xe5\xe5\x00\x07" + _bytes(rng, n)
    return body[:n]


def rewrite_edges():
    tr = Trace()
    per, joins = [], []
    sr_pos = set()
    for s in range(2):
        rng = _rng(8 + s)
        _one_video_session(tr)
        lens = [1400] + list(range(1, 25)) + [int(x) for x in rng.choice(sweep_lengths()[:400], size=40, replace=False)]
        pk = []
        seq0, ts0 = 0xFFF0, 0xFFFFF000                  # the stream's own seq / ts wrap too
        for i, n in enumerate(lens):
            pk.append((20 + 20 * (i // 13), 0, _rtp(rng, seq0 + i, ts0 + 900 * i, 0x5EED0E00 + s, n)))
        # RTCP: a spread of (PT, length) first, then one tick of 70 with SRs on the chunk edges
        for t in (40, 60):
            for n in E_RTCP_LENS:
                for pt in (200, 201):
                    pk.append((t, 1, _rtcp(rng, pt, n, 0x5EED0E00 + s)))
        for i in range(70):
            edge = i in (0, 15, 16, 31, 32, 63, 64, 69)
            pt = 200 if edge or i % 3 == 0 else 201
            n = (20, 28, 52)[i % 3] if edge else E_RTCP_LENS[(5 * i) % 8]
            pk.append((100, 1, _rtcp(rng, pt, n, 0x5EED0E00 + s)))
            if pt == 200 and n >= 20:
                sr_pos.add(i)                           # (the same positions in both sessions)
        pk.sort(key=lambda p: p[0])
        per.append(pk)
        joins += [(0, s, 3 * s + 1, UDP), (0, s, 3 * s + 2, TCP), (0, s, 3 * s + 3, UDP)]
    tr = _assemble(tr, per, 20, 140, joins)
    rtp_lens = {len(ev[4]) for ev in tr.events if ev[0] == PKT and ev[3] == 0}
    rtcp = {(ev[4][1], len(ev[4])) for ev in tr.events if ev[0] == PKT and ev[3] == 1}
    burst = max(len(t) for t in sender_ticks(tr, 0, 1))
    return tr, {"kernel": kernel_of(tr, E_REWRITE), "rtp_lens": rtp_lens, "rtcp": rtcp, "rtcp_burst": burst,
                "sr_positions": sr_pos, "rewrite": E_REWRITE, "seq0": seq0, "ts0": ts0}


# ---- F: trailer-stripped packets near a ring's capacity ------------------------------------------
F_RING_BYTES, F_RING_PACKETS = 65536, 2048
F_CFG = dict(video_ring_bytes=F_RING_BYTES, video_ring_packets=F_RING_PACKETS,
             other_ring_bytes=4096, other_ring_packets=64)
F_TICK_MS, F_PACKETS = 100, 4400


def aktt_near_capacity():
    """One packet per millisecond, 24..67 bytes, nine in ten with the 12-byte receive-time trailer
    (exact receive times, so the rewritten arrivals are the arrivals); players join at 0 and then
    every ~0.7 s, each starting 1 s back (no key frames): at a joiner's tick the ring must still
    hold the 1001 packets that arrived in its last second."""
    rng = _rng(10)
    tr = Trace()
    tr.prefs = {"reflector_use_in_packet_receive_time": "true"}
    _one_video_session(tr)
    pk, stripped, full = [], [], []
    for i in range(F_PACKETS):
        n = int(rng.integers(24, 68))
        p = _rtp(rng, i, 90 * i, 0x5EED0F01, n)
        tagged = i % 10 != 9
        pk.append((i, 0, _aktt_tag(p, 6_000_000_000 + i) if tagged else p))
        stripped.append(slot_words(n))
        full.append(slot_words(n + 12 if tagged else n))
    joins = [(0, 0, 1, UDP), (0, 0, 2, TCP)] + [(t, 0, 3 + k, TCP if k % 2 else UDP)
                                                 for k, t in enumerate(range(1230, F_PACKETS - 200, 690))]
    tr = _assemble(tr, [pk], F_TICK_MS, F_PACKETS, joins)
    span = 1001                                         # arrivals in [now - 1000, now] at a tick

    def held(words):
        c = np.concatenate([[0], np.cumsum(words)])
        return int(max(c[min(i + span, len(words))] - c[i] for i in range(len(words)))) * 16

    return tr, {"held_stripped": held(stripped), "held_unstripped": held(full), "ring_bytes": F_RING_BYTES,
                "total_stripped": 16 * sum(stripped), "total_unstripped": 16 * sum(full),
                "tagged": sum(1 for i in range(F_PACKETS) if i % 10 != 9), "kernel": kernel_of(tr)}


EDGE_TRACES = {
    "lenphase_mixed": lambda: lenphase(True), "lenphase_udp": lambda: lenphase(False),
    "chunks_udp": lambda: chunks(False), "chunks_tcp": lambda: chunks(True),
    "wrap_udp": lambda: wrap(False), "wrap_mixed": lambda: wrap(True),
    "wrap_udp_2043": lambda: wrap(False, 2043), "wrap_mixed_2043": lambda: wrap(True, 2043),
    "neighbours_udp": lambda: neighbours(False), "neighbours_patch": lambda: neighbours(True),
    "rewrite_edges": rewrite_edges,
    "aktt_near_capacity": aktt_near_capacity,
}

_cache = {}


def edge_trace(name: str):
    """(Trace, claims) of a named edge trace, generated once per process."""
    if name not in _cache:
        _cache[name] = EDGE_TRACES[name]()
    return _cache[name]
