"""The H.264 elementary-stream tap (edgpu_tap_*, edgpu_tap.hip) restated on the CPU: RFC 6184
non-interleaved depacketisation (single NAL unit packets, STAP-A, FU-A) of one track's RTP
sender queue into Annex-B access units.  The kernels must equal this model byte for byte.

A TapModel holds what a tap carries between drains (has_prev / prev_seq, the pending-damage bit,
the cumulative counters) and the queue entries not yet consumed.  `push` appends an entry (a
packet's final bytes, possibly empty); `drain` examines every entry, emits the complete access
units (all of them with flush) and consumes the entries up to the last emitted unit's last
packet.  Entries that left the ring before a drain are taken off the queue by `lose`.
"""
KEY, PARAMS, DAMAGED, NOMARKER, OPEN_END = 1, 2, 4, 8, 16
START = b"\x00\x00\x00\x01"
COUNTERS = ("packets", "skipped", "malformed", "orphans", "unsupported", "missed", "units", "damaged_units")
UNIT_FIELDS = ("offset", "bytes", "rtp_ts", "arrival_ms", "flags", "first_seq", "n_packets", "n_nals")


def parse(d: bytes):
    """(marker, seq, timestamp, payload) of a good packet, else None (rule 1)."""
    n = len(d)
    if n < 12 or d[0] >> 6 != 2:
        return None
    hdr = 12 + 4 * (d[0] & 15)
    if d[0] & 0x10:
        if hdr + 4 > n:
            return None
        hdr += 4 + 4 * ((d[hdr + 2] << 8) | d[hdr + 3])
    end = n
    if d[0] & 0x20:
        pad = d[n - 1]
        if pad == 0 or hdr + pad > n:
            return None
        end = n - pad
    if hdr >= end:
        return None
    return d[1] >> 7, (d[2] << 8) | d[3], int.from_bytes(d[4:8], "big"), d[hdr:end]


class TapModel:
    def __init__(self):
        self.has_prev = False
        self.prev_seq = 0
        self.pending = False
        self.c = dict.fromkeys(COUNTERS, 0)
        self.queue = []             # (bytes, arrival_ms) not yet consumed

    def push(self, data: bytes, arrival_ms: int = 0):
        self.queue.append((bytes(data), arrival_ms))

    def lose(self, n: int):
        """The oldest n waiting entries left the ring before they were examined."""
        del self.queue[:n]
        if n:
            self.c["missed"] += n
            self.pending = True
            self.has_prev = False

    def drain(self, flush: bool = False):
        """-> (bytes, [unit dict]); unit offsets are relative to the returned bytes."""
        out = bytearray()
        units = []
        events = []                 # per entry: counter names it adds to
        has_prev, prev_seq, prev_ts, prev_m = self.has_prev, self.prev_seq, 0, 0
        first = True
        chain = None
        au = None
        last_good = -1              # entry index of the newest good packet
        for i, (d, arrival) in enumerate(self.queue):
            ev = []
            events.append(ev)
            if not d:
                continue
            ev.append("packets")
            p = parse(d)
            if p is None:
                ev.append("skipped")
                continue
            m, seq, ts, pay = p
            gap = has_prev and seq != ((prev_seq + 1) & 0xFFFF)
            start = first or ts != prev_ts or prev_m
            if start:
                if au is not None:
                    if chain is not None:
                        au["flags"] |= DAMAGED
                    if gap and not au["marker"]:
                        au["flags"] |= DAMAGED
                au = dict(offset=len(out), bytes=0, rtp_ts=ts, arrival_ms=arrival, flags=0, first_seq=seq,
                          n_packets=0, n_nals=0, marker=0, last=i, cut=last_good + 1, state=(has_prev, prev_seq))
                if self.pending and not units:
                    au["flags"] |= DAMAGED
                units.append(au)
                chain = None
            au["n_packets"] += 1
            au["marker"] = m
            au["last"] = i
            if gap:
                au["flags"] |= DAMAGED
            t = pay[0] & 0x1F
            dropped = False
            emit = []               # NAL pieces: (new NAL?, bytes)
            if t == 28:
                if len(pay) < 2 or (pay[1] & 0xC0) == 0xC0:
                    ev.append("malformed")
                    dropped = True
                    chain = None
                else:
                    ft, s, e = pay[1] & 0x1F, pay[1] & 0x80, pay[1] & 0x40
                    if s:
                        emit.append((ft, bytes([(pay[0] & 0xE0) | ft]) + pay[2:]))
                        chain = ft
                    elif chain == ft and not gap and not start:
                        emit.append((None, pay[2:]))
                        if e:
                            chain = None
                    else:
                        ev.append("orphans")
                        dropped = True
                        chain = None
            else:
                chain = None
                if 1 <= t <= 23:
                    emit.append((t, pay))
                elif t == 24:
                    o = 1
                    while o < len(pay):
                        size = ((pay[o] << 8) | pay[o + 1]) if o + 2 <= len(pay) else 0
                        if size == 0 or o + 2 + size > len(pay):
                            ev.append("malformed")
                            dropped = True
                            break
                        emit.append((pay[o + 2] & 0x1F, pay[o + 2:o + 2 + size]))
                        o += 2 + size
                else:
                    ev.append("unsupported")
                    dropped = True
            if dropped:
                au["flags"] |= DAMAGED
            for nt, b in emit:
                if nt is not None:
                    out += START
                    au["n_nals"] += 1
                    if nt == 5:
                        au["flags"] |= KEY
                    if nt in (7, 8):
                        au["flags"] |= PARAMS
                out += b
            au["bytes"] = len(out) - au["offset"]
            has_prev, prev_seq, prev_ts, prev_m = True, seq, ts, m
            first = False
            last_good = i
        # the last unit: complete with a marker, emitted open by a flush, else left waiting
        cut = len(self.queue) if flush else 0
        if units:
            a = units[-1]
            if chain is not None:
                a["flags"] |= DAMAGED
            if a["marker"]:
                if not flush:
                    cut = a["last"] + 1
            elif flush:
                a["flags"] |= OPEN_END
            else:
                units.pop()
                cut = a["cut"]
                del out[a["offset"]:]
                has_prev, prev_seq = a["state"]
        for u in units:
            if not u["marker"]:
                u["flags"] |= NOMARKER
        for ev in events[:cut]:
            for k in ev:
                self.c[k] += 1
        self.c["units"] += len(units)
        self.c["damaged_units"] += sum(1 for u in units if u["flags"] & DAMAGED)
        if units:
            self.pending = False
        self.has_prev, self.prev_seq = has_prev, prev_seq
        del self.queue[:cut]
        return bytes(out), [{k: u[k] for k in UNIT_FIELDS} for u in units]


def depacketise(packets, flush=True):
    """One drain over `packets` (bytes each): (bytes, units, counters)."""
    m = TapModel()
    for k, p in enumerate(packets):
        m.push(p, k)
    b, u = m.drain(flush=flush)
    return b, u, dict(m.c)
