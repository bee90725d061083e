"""An RFC 6184 packetiser of its own for the tap tests (it shares nothing with tests/tap_model.py):
access units given as lists of NAL byte strings become RTP packets -- single NAL unit packets,
STAP-A for runs of small NALs, FU-A above the MTU -- with optional CSRCs, a header extension and
padding, and optional faults.  `packetise` also reports which edge conditions the trace reached, so
a test can assert that a trace meant to reach an edge does."""
import struct

START = b"\x00\x00\x00\x01"


def header(seq, ts, marker, cc=0, ext=None, pad=0, pt=96, ssrc=0x0A0B0C0D, version=2):
    b0 = (version << 6) | (0x20 if pad else 0) | (0x10 if ext is not None else 0) | cc
    h = struct.pack(">BBHII", b0, (0x80 if marker else 0) | pt, seq & 0xFFFF, ts & 0xFFFFFFFF, ssrc)
    h += b"".join(struct.pack(">I", 0xC0000000 + k) for k in range(cc))
    if ext is not None:
        h += struct.pack(">HH", 0xBEDE, ext) + bytes([0xE0 + (k & 15) for k in range(4 * ext)])
    return h


def padding(pad):
    return bytes(pad - 1) + bytes([pad]) if pad else b""


def packetise(aus, mtu=1400, seq0=100, ts0=9000, ts_step=3000, stap=False, cc=0, ext=None, pad=0,
              markers=True, drop=(), swap=(), dup=()):
    """aus: [[NAL bytes, ...], ...] -> (packets, reached).  `mtu` bounds the RTP payload.  drop /
    dup: packet positions removed / sent twice; swap: positions exchanged with their successor."""
    reached = set()
    pk = []
    seq = seq0
    for a, nals in enumerate(aus):
        ts = ts0 + a * ts_step
        groups = []
        i = 0
        while i < len(nals):
            n = nals[i]
            if stap and len(n) + 3 <= mtu and i + 1 < len(nals) and 1 + 2 + len(n) + 2 + len(nals[i + 1]) <= mtu:
                body = b""
                while i < len(nals) and 1 + len(body) + 2 + len(nals[i]) <= mtu:
                    body += struct.pack(">H", len(nals[i])) + nals[i]
                    i += 1
                groups.append([bytes([(n[0] & 0x60) | 24]) + body])
                reached.add("stap")
                continue
            if len(n) <= mtu:
                groups.append([n])
                reached.add("single")
            else:
                ind, typ = (n[0] & 0xE0) | 28, n[0] & 0x1F
                body, frag = n[1:], mtu - 2
                parts = [body[o:o + frag] for o in range(0, len(body), frag)]
                groups.append([bytes([ind, (0x80 if k == 0 else 0) | (0x40 if k == len(parts) - 1 else 0) | typ]) + p
                               for k, p in enumerate(parts)])
                reached.add("fu")
                if len(parts) > 2:
                    reached.add("fu-middle")
            i += 1
        payloads = [p for g in groups for p in g]
        for k, p in enumerate(payloads):
            last = k == len(payloads) - 1
            pk.append(header(seq, ts, markers and last, cc, ext, pad) + p + padding(pad))
            seq += 1
    if cc:
        reached.add("cc")
    if ext is not None:
        reached.add("ext")
    if pad:
        reached.add("pad")
    if any(struct.unpack(">H", p[2:4])[0] == 0 for p in pk[1:]):
        reached.add("seq-wrap")
    for k in sorted(swap):
        pk[k], pk[k + 1] = pk[k + 1], pk[k]
        reached.add("swap")
    out = []
    for k, p in enumerate(pk):
        if k in drop:
            reached.add("drop")
            continue
        out.append(p)
        if k in dup:
            out.append(p)
            reached.add("dup")
    return out, reached


def annexb(aus):
    return b"".join(START + n for nals in aus for n in nals)


def nal(typ, size, fill=None, nri=3):
    """A NAL of `size` bytes: header (type `typ`) and a byte pattern that depends on the position."""
    body = bytes(((fill if fill is not None else typ * 7) + 3 * k) & 0xFF for k in range(size - 1))
    return bytes([(nri << 5) | typ]) + body
