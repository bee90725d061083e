"""A transport-stream demultiplexer for the tests, written from ISO/IEC 13818-1 and sharing nothing
with tests/ts_model.py.  `demux` checks every 188-byte packet (sync byte, the PID set, continuity
per PID, adaptation-field lengths, stuffing), parses PAT and PMT with its own CRC-32 and
reassembles the video PES packets.

-> dict(pes=[dict(pts, pcr, rai, payload, packet)], pat=n, pmt=n, program, pmt_pid, video_pid,
        pcr_pid, stream_type, tsid).  `cc` (PID -> last counter) carries continuity across calls."""
import struct


class TsError(AssertionError):
    pass


def _crc(data):
    table = _crc.table
    if table is None:
        table = []
        for i in range(256):
            r = i << 24
            for _ in range(8):
                r = (r << 1) ^ (0x04C11DB7 if r & 0x80000000 else 0)
            table.append(r & 0xFFFFFFFF)
        _crc.table = table
    c = 0xFFFFFFFF
    for b in data:
        c = ((c << 8) & 0xFFFFFFFF) ^ table[(c >> 24) ^ b]
    return c


_crc.table = None


def _need(cond, msg):
    if not cond:
        raise TsError(msg)


def _section(payload, where):
    _need(payload[0] == 0, f"{where}: pointer field {payload[0]}")
    sec = payload[1:]
    length = ((sec[1] & 0x0F) << 8) | sec[2]
    _need(sec[1] & 0x80 and length >= 9 and 3 + length <= len(sec), f"{where}: section length {length}")
    body = sec[:3 + length]
    _need(_crc(body) == 0, f"{where}: CRC")
    _need(all(b == 0xFF for b in sec[3 + length:]), f"{where}: fill")
    _need(body[5] & 1 and (body[5] >> 1) & 31 == 0 and body[6] == 0 and body[7] == 0, f"{where}: version / section numbers")
    return body


def demux(ts, cc=None):
    cc = {} if cc is None else cc
    _need(len(ts) % 188 == 0, f"{len(ts)} bytes are no whole packets")
    info = dict(pes=[], pat=0, pmt=0, program=None, pmt_pid=None, video_pid=None, pcr_pid=None, stream_type=None, tsid=None)
    cur = None
    for k in range(len(ts) // 188):
        p = ts[188 * k:188 * k + 188]
        where = f"packet {k}"
        _need(p[0] == 0x47, f"{where}: sync byte {p[0]:02x}")
        _need(not p[1] & 0x80 and not p[1] & 0x20 and not p[3] & 0xC0, f"{where}: error / priority / scrambling bits")
        pusi, pid, afc, count = bool(p[1] & 0x40), ((p[1] & 0x1F) << 8) | p[2], (p[3] >> 4) & 3, p[3] & 15
        _need(afc in (1, 3), f"{where}: adaptation_field_control {afc}")
        if pid in cc:
            _need(count == (cc[pid] + 1) & 15, f"{where}: continuity of PID {pid:#x}: {count} after {cc[pid]}")
        cc[pid] = count
        pos, pcr, rai = 4, None, False
        if afc == 3:
            al = p[4]
            _need(al <= 182, f"{where}: adaptation field of {al} with payload")
            pos = 5 + al
            if al:
                flags = p[5]
                _need(flags & ~0x50 == 0, f"{where}: adaptation flags {flags:02x}")
                rai = bool(flags & 0x40)
                q = 6
                if flags & 0x10:
                    _need(al >= 7, f"{where}: PCR does not fit")
                    hi, lo = struct.unpack(">IH", p[6:12])
                    pcr = ((hi << 1) | (lo >> 15), lo & 0x1FF)
                    _need(lo & 0x7E00 == 0x7E00, f"{where}: PCR reserved bits")
                    q = 12
                _need(all(b == 0xFF for b in p[q:pos]), f"{where}: stuffing")
        payload = p[pos:]
        _need(len(payload) >= 1, f"{where}: no payload")
        if pid == 0:
            _need(pusi and afc == 1, f"{where}: PAT shape")
            b = _section(payload, where + " PAT")
            _need(b[0] == 0 and len(b) == 16, f"{where}: one-program PAT expected")
            info["tsid"], info["program"] = struct.unpack(">H", b[3:5])[0], struct.unpack(">H", b[8:10])[0]
            info["pmt_pid"] = struct.unpack(">H", b[10:12])[0] & 0x1FFF
            info["pat"] += 1
            continue
        if info["pmt_pid"] is not None and pid == info["pmt_pid"]:
            _need(pusi and afc == 1, f"{where}: PMT shape")
            b = _section(payload, where + " PMT")
            _need(b[0] == 2 and struct.unpack(">H", b[3:5])[0] == info["program"], f"{where}: PMT of another program")
            info["pcr_pid"] = struct.unpack(">H", b[8:10])[0] & 0x1FFF
            _need(struct.unpack(">H", b[10:12])[0] & 0xFFF == 0, f"{where}: program descriptors")
            es = b[12:-4]
            _need(len(es) == 5 and struct.unpack(">H", es[3:5])[0] & 0xFFF == 0, f"{where}: one stream without descriptors expected")
            info["stream_type"], info["video_pid"] = es[0], struct.unpack(">H", es[1:3])[0] & 0x1FFF
            info["pmt"] += 1
            continue
        _need(info["video_pid"] is None or pid == info["video_pid"], f"{where}: PID {pid:#x} is not in the PMT")
        if pusi:
            _need(payload[:3] == b"\x00\x00\x01" and payload[3] == 0xE0, f"{where}: PES start code / stream id")
            _need(payload[4:6] == b"\x00\x00", f"{where}: PES length")
            _need(payload[6] & 0xC0 == 0x80 and payload[6] & 0x04, f"{where}: PES flags {payload[6]:02x}")
            _need(payload[7] == 0x80, f"{where}: PTS only expected")
            hl = payload[8]
            _need(hl == 5, f"{where}: PES header length {hl}")
            t = payload[9:14]
            _need(t[0] >> 4 == 2 and t[0] & 1 and t[2] & 1 and t[4] & 1, f"{where}: PTS markers")
            pts = ((t[0] >> 1) & 7) << 30 | t[1] << 22 | (t[2] >> 1) << 15 | t[3] << 7 | t[4] >> 1
            _need(pcr is not None, f"{where}: the first packet of a PES carries no PCR")
            cur = dict(pts=pts, pcr=pcr, rai=rai, payload=bytearray(payload[14:]), packet=k)
            info["pes"].append(cur)
        else:
            _need(cur is not None, f"{where}: payload before any PES start")
            _need(pcr is None and not rai, f"{where}: PCR / random access inside a PES")
            cur["payload"] += payload
    for e in info["pes"]:
        e["payload"] = bytes(e["payload"])
    return info
