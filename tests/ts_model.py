"""The MPEG-2 transport-stream mux of include/edgpu.h (edgpu_ts_mux) restated on the CPU: the
executable statement of its rules.  One TsMux per call sequence; `mux` takes what a tap drain
returned (the bytes, the unit rows, the stream rows) and the caller-held state rows, and returns
the packets, one row per input unit and the byte total -- what the engine must give byte for byte.

Units and streams are dicts (or numpy records) with the fields of edgpu_tap_unit / edgpu_tap_stream
the mux reads: offset, bytes, rtp_ts, flags; unit_first, unit_count."""
KEY = 1                     # EDGPU_TAP_KEY
AUD, NOAUD = 1, 2           # EDGPU_TS_AUD, EDGPU_TS_NOAUD
PACKET = 188
M33 = (1 << 33) - 1
M64 = (1 << 64) - 1


def crc32_mpeg2(data: bytes) -> int:
    crc = 0xFFFFFFFF
    for b in data:
        crc ^= b << 24
        for _ in range(8):
            crc = ((crc << 1) ^ 0x04C11DB7) & 0xFFFFFFFF if crc & 0x80000000 else (crc << 1) & 0xFFFFFFFF
    return crc


class Config:
    def __init__(self, pmt_pid=0, video_pid=0, tsid=0, program=0, flags=0, pcr_lead=0, pts_offset=0):
        self.pmt_pid = pmt_pid or 0x1000
        self.video_pid = video_pid or 0x0100
        self.tsid = tsid or 1
        self.program = program or 1
        self.aud = flags == 0 or bool(flags & AUD)
        self.pcr_lead = pcr_lead or 63000
        self.pts_offset = pts_offset


def new_state():
    return dict(ext_ts=0, started=0, cc_pat=0, cc_pmt=0, cc_video=0)


def pat_section(cfg: Config) -> bytes:
    s = bytes([0x00, 0xB0, 0x0D, cfg.tsid >> 8, cfg.tsid & 0xFF, 0xC1, 0x00, 0x00,
               cfg.program >> 8, cfg.program & 0xFF, 0xE0 | (cfg.pmt_pid >> 8), cfg.pmt_pid & 0xFF])
    return s + crc32_mpeg2(s).to_bytes(4, "big")


def pmt_section(cfg: Config) -> bytes:
    v = cfg.video_pid
    s = bytes([0x02, 0xB0, 0x12, cfg.program >> 8, cfg.program & 0xFF, 0xC1, 0x00, 0x00,
               0xE0 | (v >> 8), v & 0xFF, 0xF0, 0x00, 0x1B, 0xE0 | (v >> 8), v & 0xFF, 0xF0, 0x00])
    return s + crc32_mpeg2(s).to_bytes(4, "big")


def psi_packet(pid: int, cc: int, section: bytes) -> bytes:
    p = bytes([0x47, 0x40 | (pid >> 8), pid & 0xFF, 0x10 | (cc & 15), 0x00]) + section
    return p + b"\xFF" * (PACKET - len(p))


def pts_bytes(pts: int) -> bytes:
    return bytes([0x21 | ((pts >> 29) & 0x0E), (pts >> 22) & 0xFF, ((pts >> 14) & 0xFE) | 1,
                  (pts >> 7) & 0xFF, ((pts << 1) & 0xFE) | 1])


def pcr_bytes(base: int) -> bytes:
    return bytes([(base >> 25) & 0xFF, (base >> 17) & 0xFF, (base >> 9) & 0xFF, (base >> 1) & 0xFF,
                  ((base & 1) << 7) | 0x7E, 0x00])


def extend(state, rtp_ts: int) -> int:
    """The unit's extended timestamp; the state moves on."""
    if not state["started"]:
        ext = rtp_ts
        state["started"] = 1
    else:
        prev = state["ext_ts"]
        d = (rtp_ts - prev) & 0xFFFFFFFF
        if d & 0x80000000:
            d -= 1 << 32
        ext = (prev + d) & M64
    state["ext_ts"] = ext
    return ext


def unit_packets(cfg: Config, state, es: bytes, key: bool, ext: int) -> bytes:
    """The packets of one unit with ES bytes, PSI included."""
    out = bytearray()
    if key:
        out += psi_packet(0, state["cc_pat"], pat_section(cfg))
        out += psi_packet(cfg.pmt_pid, state["cc_pmt"], pmt_section(cfg))
        state["cc_pat"] = (state["cc_pat"] + 1) & 15
        state["cc_pmt"] = (state["cc_pmt"] + 1) & 15
    pts = (ext + cfg.pts_offset) & M33
    pes = b"\x00\x00\x01\xE0\x00\x00\x84\x80\x05" + pts_bytes(pts)
    if cfg.aud and (len(es) < 5 or (es[4] & 0x1F) != 9):
        pes += b"\x00\x00\x00\x01\x09\xF0"
    pes += es
    pid = cfg.video_pid
    pos, first = 0, True
    while pos < len(pes):
        left = len(pes) - pos
        cc = state["cc_video"]
        state["cc_video"] = (cc + 1) & 15
        if first:
            n = min(left, 176)
            af = bytes([0x10 | (0x40 if key else 0)]) + pcr_bytes((ext + cfg.pts_offset - cfg.pcr_lead) & M33) + b"\xFF" * (176 - n)
            pkt = bytes([0x47, 0x40 | (pid >> 8), pid & 0xFF, 0x30 | cc, len(af)]) + af
        elif left >= 184:
            n = 184
            pkt = bytes([0x47, pid >> 8, pid & 0xFF, 0x10 | cc])
        else:
            n = left
            al = 183 - n
            pkt = bytes([0x47, pid >> 8, pid & 0xFF, 0x30 | cc, al]) + (b"\x00" + b"\xFF" * (al - 1) if al else b"")
        pkt += pes[pos:pos + n]
        assert len(pkt) == PACKET
        out += pkt
        pos += n
        first = False
    return bytes(out)


def mux(cfg, es, units, streams, states):
    """-> (bytes, rows, total).  `states` (one dict per stream row) move on.  rows: one dict per
    input unit -- offset, bytes, flags, pts, stream; a unit no stream row covers stays zero."""
    cfg = cfg or Config()
    rows = [dict(offset=0, bytes=0, flags=0, pts=0, stream=0) for _ in units]
    out = bytearray()
    for s, st in enumerate(streams):
        first, count = int(st["unit_first"]), int(st["unit_count"])
        for i in range(first, first + count):
            u = units[i]
            off, n, flags = int(u["offset"]), int(u["bytes"]), int(u["flags"])
            ext = extend(states[s], int(u["rtp_ts"]))
            pk = unit_packets(cfg, states[s], bytes(es[off:off + n]), bool(flags & KEY), ext) if n else b""
            rows[i] = dict(offset=len(out), bytes=len(pk), flags=flags, pts=(ext + cfg.pts_offset) & M33, stream=s)
            out += pk
    return bytes(out), rows, len(out)


def mux_stream(cfg, es_units, state=None):
    """One stream given as [(es bytes, rtp_ts, flags)]: (bytes, rows, state)."""
    state = new_state() if state is None else state
    es, units = bytearray(), []
    for b, ts, fl in es_units:
        units.append(dict(offset=len(es), bytes=len(b), rtp_ts=ts & 0xFFFFFFFF, flags=fl))
        es += b
    out, rows, _ = mux(cfg, bytes(es), units, [dict(unit_first=0, unit_count=len(units))], [state])
    return out, rows, state
