"""An RFC 3640 packetiser for the audio-tap tests, written from the RFC alone: it shares no code with
tests/aac_model.py.  AAC-hbr (13-bit AU-size, 3-bit AU-index / AU-index-delta) and AAC-lbr (6 + 2
bits); consecutive frames are aggregated, up to `max_aus` per packet, while the payload stays within
`mtu`; a frame that does not fit a packet alone is fragmented (AAC-hbr only), every fragment under
one AU header that states the whole frame's size, the marker on the last."""
import struct


def rtp(seq, ts, marker, payload, pt=97, ssrc=0x0A0B0C0D, cc=0, ext=None, pad=0):
    """One RTP packet: `cc` CSRCs, an extension of `ext` 32-bit words (None: no X bit), `pad` padding bytes."""
    b0 = 0x80 | cc | (0x10 if ext is not None else 0) | (0x20 if pad else 0)
    out = struct.pack(">BBHII", b0, (0x80 if marker else 0) | pt, seq & 0xFFFF, ts & 0xFFFFFFFF, ssrc)
    out += b"".join(struct.pack(">I", 0xC0000000 + k) for k in range(cc))
    if ext is not None:
        out += struct.pack(">HH", 0xBEDE, ext) + bytes(range(1, 4 * ext + 1))
    out += payload
    if pad:
        out += bytes(pad - 1) + bytes([pad])
    return out


def section(sizes, hbr=True):
    """AU-headers-length and the AU headers of frames of these sizes, all AU-index(-delta) 0."""
    if hbr:
        return struct.pack(">H", 16 * len(sizes)) + b"".join(struct.pack(">H", s << 3) for s in sizes)
    return struct.pack(">H", 8 * len(sizes)) + bytes(s << 2 for s in sizes)


def packetise(frames, hbr=True, mtu=1400, max_aus=16, seq0=0, ts0=0, samples=1024, **hdr):
    """frames: [bytes] -> [RTP packet bytes].  Frame k has timestamp ts0 + k * samples."""
    h = 2 if hbr else 1
    packets, seq, k = [], seq0, 0
    while k < len(frames):
        ts = ts0 + k * samples
        if 2 + h + len(frames[k]) > mtu:
            assert hbr, "AAC-lbr cannot fragment"
            body, room = frames[k], mtu - 2 - h
            assert room > 0
            for at in range(0, len(body), room):
                piece = body[at:at + room]
                packets.append(rtp(seq, ts, at + room >= len(body), section([len(body)]) + piece, **hdr))
                seq += 1
            k += 1
            continue
        group = [frames[k]]
        while (k + len(group) < len(frames) and len(group) < max_aus and
               2 + h * (len(group) + 1) + sum(map(len, group)) + len(frames[k + len(group)]) <= mtu):
            group.append(frames[k + len(group)])
        packets.append(rtp(seq, ts, True, section([len(f) for f in group], hbr) + b"".join(group), **hdr))
        seq += 1
        k += len(group)
    return packets


def frame(n, seed=0):
    """A frame body of n bytes that no other (n, seed) shares."""
    return bytes((seed * 131 + n * 7 + 13 * j + (j >> 8)) & 0xFF for j in range(n))
