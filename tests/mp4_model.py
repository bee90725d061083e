"""The fragmented-MP4 mux of include/edgpu.h (edgpu_mp4_mux) restated on the CPU: the executable
statement of its rules.  `mux` takes what a tap drain returned (the bytes, the unit rows, the stream
rows) and the caller-held state rows, and returns the output bytes, one sample row per input unit,
the fragment rows and the byte total -- what the engine must give byte for byte.

Units and streams are dicts (or numpy records) with the fields of edgpu_tap_unit / edgpu_tap_stream
the mux reads: offset, bytes, rtp_ts, flags; unit_first, unit_count.

Rules this model fixed where the feature request left them open:
  * the stream's last sample of a call takes last_step *after* the call's own update (so two or
    more samples in a call never fall back to an older step);
  * last_step holds the clamped difference;
  * a fragment's flags are the OR of its sample rows' flags, DAMAGED for a missing leading start
    code included;
  * the row of a unit without bytes keeps its dts and the tap flags, fragment 0xFFFFFFFF, the rest 0;
  * result bytes: the end of the last stream row's run (an empty last row ends at the aligned end
    of the run before it); bytes between runs are not written (`fill` here)."""
KEY, DAMAGED = 1, 4         # EDGPU_TAP_KEY, EDGPU_TAP_DAMAGED
NONE = 0xFFFFFFFF
M64 = (1 << 64) - 1
START = b"\x00\x00\x00\x01"


class Config:
    def __init__(self, max_samples=0, default_duration=0, time_offset=0):
        self.max_samples = max_samples
        self.default_duration = default_duration or 3600
        self.time_offset = time_offset


def new_state():
    return dict(ext_ts=0, origin=0, sequence=0, last_step=0, started=0)


def extend(state, rtp_ts: int) -> int:
    """The unit's extended timestamp; the state moves on (as in the transport-stream mux)."""
    if not state["started"]:
        ext = rtp_ts
        state["started"] = 1
        state["origin"] = ext
    else:
        prev = state["ext_ts"]
        d = (rtp_ts - prev) & 0xFFFFFFFF
        if d & 0x80000000:
            d -= 1 << 32
        ext = (prev + d) & M64
    state["ext_ts"] = ext
    return ext


def start_codes(es: bytes) -> list:
    """Positions of every 00 00 00 01 wholly inside `es` (occurrences cannot overlap)."""
    out, i = [], es.find(START)
    while i >= 0:
        out.append(i)
        i = es.find(START, i + 1)
    return out


def sample_of(es: bytes):
    """-> (sample bytes, damaged): each start code replaced by the length of the NAL after it."""
    sc = start_codes(es)
    out = bytearray(es)
    for j, q in enumerate(sc):
        end = sc[j + 1] if j + 1 < len(sc) else len(es)
        out[q:q + 4] = (end - (q + 4)).to_bytes(4, "big")
    return bytes(out), bool(es) and (not sc or sc[0] != 0)


def be32(v):
    return (v & 0xFFFFFFFF).to_bytes(4, "big")


def fragment_bytes(sequence: int, tfdt: int, samples: list) -> bytes:
    """samples: [(bytes, duration, key)]"""
    n = len(samples)
    trun = be32(20 + 12 * n) + b"trun" + be32(0x000701) + be32(n) + be32(88 + 12 * n + 8)
    for data, dur, key in samples:
        trun += be32(dur) + be32(len(data)) + be32(0x02000000 if key else 0x01010000)
    tfhd = be32(16) + b"tfhd" + be32(0x020000) + be32(1)
    tfdt_box = be32(20) + b"tfdt" + be32(0x01000000) + (tfdt & M64).to_bytes(8, "big")
    traf = tfhd + tfdt_box + trun
    traf = be32(8 + len(traf)) + b"traf" + traf
    mfhd = be32(16) + b"mfhd" + be32(0) + be32(sequence)
    moof = mfhd + traf
    moof = be32(8 + len(moof)) + b"moof" + moof
    assert len(moof) == 88 + 12 * n
    payload = b"".join(s[0] for s in samples)
    return moof + be32(8 + len(payload)) + b"mdat" + payload


def mux(cfg, es, units, streams, states, fill=0):
    """-> (bytes, sample rows, fragment rows, total).  `states` (one dict per stream row) move on."""
    cfg = cfg or Config()
    rows = [dict(offset=0, dts=0, bytes=0, duration=0, flags=0, fragment=0) for _ in units]
    frags = []
    out = bytearray()
    for s, st in enumerate(streams):
        out += bytes([fill]) * (-len(out) % 16)
        first, count = int(st["unit_first"]), int(st["unit_count"])
        state = states[s]
        samples = []                                        # [unit, ext, dts, data, flags]
        for i in range(first, first + count):
            u = units[i]
            off, n, flags = int(u["offset"]), int(u["bytes"]), int(u["flags"])
            ext = extend(state, int(u["rtp_ts"]))
            dts = (ext - state["origin"] + cfg.time_offset) & M64
            if not n:
                rows[i] = dict(offset=0, dts=dts, bytes=0, duration=0, flags=flags, fragment=NONE)
                continue
            data, damaged = sample_of(bytes(es[off:off + n]))
            samples.append([i, ext, dts, data, flags | (DAMAGED if damaged else 0)])
        durs = []
        for a, b in zip(samples, samples[1:]):
            d = (b[1] - a[1]) & M64
            if d & (1 << 63):
                d -= 1 << 64
            d = 0 if d <= 0 else min(d, 0xFFFFFFFF)
            if d > 0:
                state["last_step"] = d
            durs.append(d)
        if samples:
            durs.append(state["last_step"] or cfg.default_duration)
        groups = []
        for k, sm in enumerate(samples):
            if k == 0 or (sm[4] & KEY) or (cfg.max_samples and len(groups[-1]) >= cfg.max_samples):
                groups.append([])
            groups[-1].append(k)
        for g in groups:
            state["sequence"] = (state["sequence"] + 1) & 0xFFFFFFFF
            body = fragment_bytes(state["sequence"], samples[g[0]][2],
                                  [(samples[k][3], durs[k], bool(samples[k][4] & KEY)) for k in g])
            fr = dict(offset=len(out), tfdt=samples[g[0]][2], duration=sum(durs[k] for k in g), bytes=len(body),
                      sequence=state["sequence"], unit_first=samples[g[0]][0], samples=len(g), flags=0, stream=s)
            pos = len(out) + 88 + 12 * len(g) + 8
            for k in g:
                i, _, dts, data, flags = samples[k]
                rows[i] = dict(offset=pos, dts=dts, bytes=len(data), duration=durs[k], flags=flags, fragment=len(frags))
                fr["flags"] |= flags
                pos += len(data)
            frags.append(fr)
            out += body
    return bytes(out), rows, frags, len(out)


def mux_stream(cfg, es_units, state=None):
    """One stream given as [(es bytes, rtp_ts, flags)]: (bytes, sample rows, fragment rows, state)."""
    state = new_state() if state is None else state
    es, units = bytearray(), []
    for b, ts, fl in es_units:
        units.append(dict(offset=len(es), bytes=len(b), rtp_ts=ts & 0xFFFFFFFF, flags=fl))
        es += b
    out, rows, frags, _ = mux(cfg, bytes(es), units, [dict(unit_first=0, unit_count=len(units))], [state])
    return out, rows, frags, state
