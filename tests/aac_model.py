"""The AAC audio tap (edgpu_aac_tap_*, edgpu_aac.hip) restated on the CPU: RFC 3640 AAC-hbr / AAC-lbr
depacketisation of one track's RTP sender queue into AAC frames, raw or behind generated ADTS
headers.  The kernels must equal this model byte for byte.

An AacModel holds what a tap carries between drains (has_prev / prev_seq, the pending-discontinuity
bit, the cumulative counters) and the queue entries not yet consumed.  `push` appends an entry (a
packet's final bytes, possibly empty); `drain` examines every entry, emits every frame that is
complete and consumes the entries before the first fragment of a chain still open (all of them with
flush).  Entries that left the ring before a drain are taken off the queue by `lose`.

Where include/edgpu.h's text leaves a choice, this file makes it:
  * the checks of the AU-header section are made in the order the header lists them, and the
    interleaving check looks at all n headers before any AU is emitted;
  * a bad (`skipped`) packet is absent: it sets no discontinuity and abandons no chain by itself;
  * a fragment of a frame too long for ADTS is dropped packet by packet (`unsupported` each);
  * the fragments of an abandoned chain count in `orphans` at the packet that abandons it; if that
    packet is a fragment whose own chain then waits, they count in the drain that consumes them, and
    the pending discontinuity is carried, so nothing of the abandoned chain is forgotten;
  * an open chain keeps back everything from its first fragment on, empty and bad entries included.
"""
from tap_model import parse

HBR, LBR = 1, 2
ADTS, RAW = 1, 2
MAX_AUS = 16
DISCONT, FRAGMENTED = 1, 2
ADTS_MAX = 8191 - 7
COUNTERS = ("packets", "skipped", "malformed", "orphans", "unsupported", "missed", "frames", "discontinuities")
FRAME_FIELDS = ("offset", "bytes", "rtp_ts", "arrival_ms", "flags", "first_seq", "n_packets", "au_index")


def adts_header(size, object_type, freq_index, channels):
    L = size + 7
    return bytes([0xFF, 0xF1, ((object_type - 1) << 6) | (freq_index << 2) | (channels >> 2),
                  ((channels & 3) << 6) | (L >> 11), (L >> 3) & 0xFF, ((L & 7) << 5) | 0x1F, 0xFC])


def au_headers(pay, h):
    """The AU-header section of a payload: ("malformed" | "unsupported", None) or (None, [AU-size])."""
    if len(pay) < 2:
        return "malformed", None
    bits = (pay[0] << 8) | pay[1]
    if bits == 0 or bits % (8 * h):
        return "malformed", None
    n = bits // (8 * h)
    H = 2 + n * h
    if H > len(pay):
        return "malformed", None
    if n > MAX_AUS:
        return "unsupported", None
    sizes = []
    for k in range(n):
        v = ((pay[2 + 2 * k] << 8) | pay[3 + 2 * k]) if h == 2 else pay[2 + k]
        if v & (7 if h == 2 else 3):
            return "unsupported", None              # AU-index / AU-index-delta: interleaving
        sizes.append(v >> 3 if h == 2 else v >> 2)
    return None, sizes


class AacModel:
    def __init__(self, mode=HBR, framing=ADTS, object_type=2, freq_index=4, channels=2, frame_samples=1024):
        self.h = 2 if mode == HBR else 1
        self.adts = framing != RAW
        self.asc = (object_type, freq_index, channels)
        self.frame_samples = frame_samples or 1024
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

    def frame(self, out, body):
        if self.adts:
            out += adts_header(len(body), *self.asc)
        out += body

    def drain(self, flush: bool = False):
        """-> (bytes, [frame dict]); frame offsets are relative to the returned bytes."""
        out = bytearray()
        frames = []
        events = []                 # per entry: the counter names it adds to
        has_prev, prev_seq, disc = self.has_prev, self.prev_seq, self.pending
        chain = None                # the open chain: ts, size, pieces, n, arrival, seq, entry, state before it
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
            _, seq, ts, pay = p
            before = (has_prev, prev_seq, disc)
            gap = has_prev and seq != ((prev_seq + 1) & 0xFFFF)
            has_prev, prev_seq = True, seq
            if gap:
                disc = True

            def abandon():
                nonlocal chain, disc
                if chain is not None:
                    ev.extend(["orphans"] * chain["n"])
                    disc = True
                    chain = None

            err, sizes = au_headers(pay, self.h)
            if err:
                abandon()
                ev.append(err)
                disc = True
                continue
            H = 2 + len(sizes) * self.h
            if len(sizes) == 1 and sizes[0] > len(pay) - H:         # a fragment
                size, piece = sizes[0], pay[H:]
                if self.h != 2 or (self.adts and size > ADTS_MAX):
                    abandon()
                    ev.append("malformed" if self.h != 2 else "unsupported")
                    disc = True
                    continue
                if chain is not None and not gap and ts == chain["ts"] and size == chain["size"]:
                    if chain["bytes"] + len(piece) > size:
                        abandon()
                        ev.append("malformed")
                        disc = True
                        continue
                else:
                    left = chain["n"] if chain is not None else 0       # it abandons a chain: that much is known
                    abandon()                                           # even if this fragment then waits
                    chain = dict(ts=ts, size=size, pieces=[], bytes=0, n=0, arrival=arrival, seq=seq, entry=i,
                                 before=(before[0], before[1], before[2] or left > 0), left=left)
                chain["pieces"].append(piece)
                chain["bytes"] += len(piece)
                chain["n"] += 1
                if chain["bytes"] == size:
                    frames.append(dict(offset=len(out), bytes=size + (7 if self.adts else 0), rtp_ts=ts, arrival_ms=chain["arrival"],
                                       flags=FRAGMENTED | (DISCONT if disc else 0), first_seq=chain["seq"], n_packets=chain["n"],
                                       au_index=0))
                    self.frame(out, b"".join(chain["pieces"]))
                    disc = False
                    chain = None
                continue
            abandon()
            off = H
            for k, size in enumerate(sizes):
                if size == 0 or off + size > len(pay):
                    ev.append("malformed")
                    disc = True
                    break
                frames.append(dict(offset=len(out), bytes=size + (7 if self.adts else 0),
                                   rtp_ts=(ts + k * self.frame_samples) & 0xFFFFFFFF, arrival_ms=arrival,
                                   flags=DISCONT if disc else 0, first_seq=seq, n_packets=1, au_index=k))
                self.frame(out, pay[off:off + size])
                disc = False
                off += size
        cut = len(self.queue)
        if chain is not None:
            if flush:
                events.append(["orphans"] * chain["n"])
                disc = True
            else:
                cut = chain["entry"]
                has_prev, prev_seq, disc = chain["before"]
                events.append(["orphans"] * chain["left"])
        for ev in events[:cut] + events[len(self.queue):]:
            for k in ev:
                self.c[k] += 1
        self.c["frames"] += len(frames)
        self.c["discontinuities"] += sum(1 for f in frames if f["flags"] & DISCONT)
        self.has_prev, self.prev_seq, self.pending = has_prev, prev_seq, disc
        del self.queue[:cut]
        return bytes(out), frames


def depacketise(packets, flush=True, **cfg):
    """One drain over `packets` (bytes each): (bytes, frames, counters)."""
    m = AacModel(**cfg)
    for k, p in enumerate(packets):
        m.push(p, k)
    b, f = m.drain(flush=flush)
    return b, f, dict(m.c)
