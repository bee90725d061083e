"""The FLV mux of include/edgpu.h (edgpu_flv_mux) restated on the CPU: the executable statement of
its rules.  `mux` takes what a tap drain returned (the bytes, the unit rows, the stream rows) and the
caller-held state rows, and returns the output bytes, one tag row per input unit and the byte total
-- what the engine must give byte for byte.  `header` restates edgpu_flv_header's FILE and META
parts and wraps a given AVCDecoderConfigurationRecord into SEQ (the record itself is the engine's).

Units and streams are dicts (or numpy records) with the fields of edgpu_tap_unit / edgpu_tap_stream
the mux reads: offset, bytes, rtp_ts, flags; unit_first, unit_count.

Rules this model fixed where the feature request left them open:
  * the row of a unit without bytes carries its stream row's index too (as a tag's row does); its
    parameter-set fields are 0;
  * parameter sets are looked for only in a unit with both EDGPU_TAP_PARAMS and ES bytes; the eight
    NALs are counted from the unit's first start code, NALs of length 0 included, so bytes before a
    first start code (a DAMAGED unit) are no NAL; a NAL is measured as its length field says (to the
    next start code wholly inside the unit, or the unit's end);
  * the 0xFFFFFA limit holds for every unit given, covered by a stream row or not;
  * a run could reach 2^32 bytes when its units' bytes + 20 per unit (units without bytes too) do;
  * result bytes: the end of the last stream row's run (an empty last row ends at the aligned end
    of the run before it); bytes between runs are not written (`fill` here)."""
import struct

KEY, PARAMS, DAMAGED = 1, 2, 4      # EDGPU_TAP_KEY, EDGPU_TAP_PARAMS, EDGPU_TAP_DAMAGED
M64 = (1 << 64) - 1
START = b"\x00\x00\x00\x01"
FILE, META, SEQ = 1, 2, 4           # EDGPU_FLV_FILE ...
FILE_HEADER = bytes.fromhex("464C5601010000000900000000")
MAX_UNIT = 0xFFFFFA
PARAM_NALS = 8


class Config:
    def __init__(self, time_offset=0):
        self.time_offset = time_offset


def new_state():
    return dict(ext_ts=0, origin=0, started=0)


def extend(state, rtp_ts: int) -> int:
    """The unit's extended timestamp; the state moves on (as in the fragmented-MP4 mux)."""
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
    """-> (sample bytes, damaged, [(NAL offset, NAL length)]): each start code replaced by the length
    of the NAL after it."""
    sc = start_codes(es)
    out = bytearray(es)
    nals = []
    for j, q in enumerate(sc):
        end = sc[j + 1] if j + 1 < len(sc) else len(es)
        out[q:q + 4] = (end - (q + 4)).to_bytes(4, "big")
        nals.append((q + 4, end - (q + 4)))
    return bytes(out), bool(es) and (not sc or sc[0] != 0), nals


def tag_bytes(sample: bytes, timestamp_ms: int, key: bool) -> bytes:
    s = len(sample)
    return (b"\x09" + (s + 5).to_bytes(3, "big") + (timestamp_ms & 0xFFFFFF).to_bytes(3, "big") + bytes([timestamp_ms >> 24])
            + b"\x00\x00\x00" + (b"\x17" if key else b"\x27") + b"\x01\x00\x00\x00" + sample + (s + 16).to_bytes(4, "big"))


def zero_row():
    return dict(offset=0, bytes=0, timestamp_ms=0, flags=0, stream=0, sps_offset=0, sps_bytes=0, pps_offset=0, pps_bytes=0)


def mux(cfg, es, units, streams, states, fill=0):
    """-> (bytes, tag rows, total).  `states` (one dict per stream row) move on."""
    cfg = cfg or Config()
    rows = [zero_row() for _ in units]
    out = bytearray()
    for s, st in enumerate(streams):
        out += bytes([fill]) * (-len(out) % 16)
        first, count = int(st["unit_first"]), int(st["unit_count"])
        state = states[s]
        for i in range(first, first + count):
            u = units[i]
            off, n, flags = int(u["offset"]), int(u["bytes"]), int(u["flags"])
            ext = extend(state, int(u["rtp_ts"]))
            t90 = (ext - state["origin"] + cfg.time_offset) & M64
            ms = (t90 // 90) & 0xFFFFFFFF
            row = zero_row()
            row.update(offset=len(out), timestamp_ms=ms, flags=flags, stream=s)
            if n:
                raw = bytes(es[off:off + n])
                data, damaged, nals = sample_of(raw)
                if damaged:
                    row["flags"] |= DAMAGED
                if flags & PARAMS:
                    for at, ln in nals[:PARAM_NALS]:
                        if not ln:
                            continue
                        kind = raw[at] & 0x1F
                        if kind == 7 and not row["sps_bytes"]:
                            row["sps_offset"], row["sps_bytes"] = 16 + at, ln
                        if kind == 8 and not row["pps_bytes"]:
                            row["pps_offset"], row["pps_bytes"] = 16 + at, ln
                row["bytes"] = n + 20
                out += tag_bytes(data, ms, bool(flags & KEY))
            rows[i] = row
    return bytes(out), rows, len(out)


def bad_argument(units, streams) -> bool:
    """Whether edgpu_flv_mux refuses these rows for their sizes (the index errors are edgpu_ts_mux's)."""
    if any(int(u["bytes"]) > MAX_UNIT for u in units):
        return True
    for st in streams:
        first, count = int(st["unit_first"]), int(st["unit_count"])
        if sum(int(units[i]["bytes"]) for i in range(first, first + count)) + 20 * count >= 1 << 32:
            return True
    return False


def mux_stream(cfg, es_units, state=None):
    """One stream given as [(es bytes, rtp_ts, flags)]: (bytes, tag rows, state)."""
    state = new_state() if state is None else state
    es, units = bytearray(), []
    for b, ts, fl in es_units:
        units.append(dict(offset=len(es), bytes=len(b), rtp_ts=ts & 0xFFFFFFFF, flags=fl))
        es += b
    out, rows, _ = mux(cfg, bytes(es), units, [dict(unit_first=0, unit_count=len(units))], [state])
    return out, rows, state


def header(record: bytes, width: int, height: int, timestamp_ms=0, parts=0) -> bytes:
    """edgpu_flv_header around a given AVCDecoderConfigurationRecord."""
    parts = parts or (FILE | META | SEQ)

    def tag(kind, ms, data):
        return (bytes([kind]) + len(data).to_bytes(3, "big") + (ms & 0xFFFFFF).to_bytes(3, "big") + bytes([ms >> 24]) + bytes(3)
                + data + (11 + len(data)).to_bytes(4, "big"))

    def prop(name, v):
        return len(name).to_bytes(2, "big") + name.encode() + b"\x00" + struct.pack(">d", v)
    out = b""
    if parts & FILE:
        out += FILE_HEADER
    if parts & META:
        out += tag(0x12, 0, b"\x02\x00\x0AonMetaData" + b"\x08\x00\x00\x00\x03" + prop("width", float(width))
                   + prop("height", float(height)) + prop("videocodecid", 7.0) + b"\x00\x00\x09")
    if parts & SEQ:
        out += tag(0x09, timestamp_ms, b"\x17\x00\x00\x00\x00" + record)
    return out
