"""An independent fragmented-MP4 reader written from ISO/IEC 14496-12 / -15 (it knows nothing of
tests/mp4_model.py): walks the boxes, requires every size to nest exactly, data_offset to land on the
mdat payload, the sample sizes to tile the payload and the length-prefixed NALs to tile each sample,
and turns the samples back into Annex-B."""
import struct

CONTAINERS = {b"moov", b"trak", b"mdia", b"minf", b"dinf", b"stbl", b"mvex", b"moof", b"traf"}


class DemuxError(AssertionError):
    pass


def need(cond, msg):
    if not cond:
        raise DemuxError(msg)


def boxes(data: bytes, start=0, end=None):
    """[(type, payload start, payload end)] of the boxes that tile data[start:end] exactly."""
    end = len(data) if end is None else end
    out, pos = [], start
    while pos < end:
        need(end - pos >= 8, f"box header cut at {pos}")
        size, typ = struct.unpack_from(">I4s", data, pos)
        need(size >= 8 and pos + size <= end, f"box {typ} at {pos}: size {size} does not nest in {end}")
        out.append((typ, pos + 8, pos + size))
        pos += size
    need(pos == end, "boxes do not tile their parent")
    return out


def tree(data: bytes, start=0, end=None):
    """{type: [(payload start, payload end, children)]} recursively for the container boxes."""
    out = {}
    for typ, a, b in boxes(data, start, end):
        out.setdefault(typ, []).append((a, b, tree(data, a, b) if typ in CONTAINERS else None))
    return out


def one(t, typ):
    need(typ in t and len(t[typ]) == 1, f"expected exactly one {typ}")
    return t[typ][0]


def annexb(sample: bytes) -> bytes:
    """Length-prefixed NALs, which must tile the sample, as start-code-prefixed ones."""
    out, pos = bytearray(), 0
    while pos < len(sample):
        need(len(sample) - pos >= 4, "NAL length cut")
        n = struct.unpack_from(">I", sample, pos)[0]
        need(pos + 4 + n <= len(sample), "NAL runs past its sample")
        out += b"\x00\x00\x00\x01" + sample[pos + 4:pos + 4 + n]
        pos += 4 + n
    return bytes(out)


def fragments(data: bytes, prefixed=True):
    """The moof + mdat pairs that tile `data`: a list of dicts -- offset, bytes, sequence, tfdt and
    samples [(duration, flags, sample bytes, Annex-B bytes)].  `prefixed` False skips the NAL check
    (a sample whose unit lacked a leading start code is not a sequence of NALs)."""
    top = boxes(data)
    need(len(top) % 2 == 0, "fragments are moof + mdat pairs")
    out = []
    for (t1, a1, b1), (t2, a2, b2) in zip(top[0::2], top[1::2]):
        need(t1 == b"moof" and t2 == b"mdat", f"expected moof, mdat; got {t1}, {t2}")
        moof_start = a1 - 8
        t = tree(data, a1, b1)
        a, b, _ = one(t, b"mfhd")
        need(b - a == 8, "mfhd size")
        vf, seq = struct.unpack_from(">II", data, a)
        need(vf == 0, "mfhd version / flags")
        _, _, traf = one(t, b"traf")
        need(sorted(traf) == [b"tfdt", b"tfhd", b"trun"], "traf children")
        a, b, _ = one(traf, b"tfhd")
        need(b - a == 8 and struct.unpack_from(">II", data, a) == (0x020000, 1), "tfhd: default-base-is-moof, track 1")
        a, b, _ = one(traf, b"tfdt")
        need(b - a == 12 and struct.unpack_from(">I", data, a)[0] == 0x01000000, "tfdt version 1")
        tfdt = struct.unpack_from(">Q", data, a + 4)[0]
        a, b, _ = one(traf, b"trun")
        vf, n, data_offset = struct.unpack_from(">IIi", data, a)
        need(vf == 0x000701, "trun flags")
        need(b - a == 12 + 12 * n, "trun size")
        need(moof_start + data_offset == a2, "data_offset does not land on the mdat payload")
        pos, samples = a2, []
        for k in range(n):
            dur, size, fl = struct.unpack_from(">III", data, a + 12 + 12 * k)
            need(pos + size <= b2, "samples run past the mdat")
            raw = data[pos:pos + size]
            samples.append((dur, fl, raw, annexb(raw) if prefixed else None))
            pos += size
        need(pos == b2, "the sample sizes do not tile the mdat payload")
        out.append(dict(offset=moof_start, bytes=b2 - moof_start, sequence=seq, tfdt=tfdt, samples=samples))
    return out


def init_segment(data: bytes):
    """ftyp + moov -> dict(timescale, width, height, tkhd_width, tkhd_height, sps, pps, avcc_ext, brand)."""
    top = tree(data)
    need(list(t for t, _, _ in boxes(data)) == [b"ftyp", b"moov"], "an init segment is ftyp + moov")
    a, b, _ = one(top, b"ftyp")
    brand = data[a:a + 4]
    _, _, moov = one(top, b"moov")
    a, b, _ = one(moov, b"mvhd")
    need(b - a == 100 and data[a] == 0, "mvhd version 0")
    mv_timescale = struct.unpack_from(">I", data, a + 12)[0]
    _, _, mvex = one(moov, b"mvex")
    a, b, _ = one(mvex, b"trex")
    need(b - a == 24 and struct.unpack_from(">II", data, a + 4) == (1, 1), "trex: track 1, description 1")
    _, _, trak = one(moov, b"trak")
    a, b, _ = one(trak, b"tkhd")
    need(b - a == 84 and struct.unpack_from(">I", data, a + 12)[0] == 1, "tkhd: track 1")
    tw, th = struct.unpack_from(">II", data, a + 76)
    _, _, mdia = one(trak, b"mdia")
    a, b, _ = one(mdia, b"mdhd")
    need(b - a == 24, "mdhd size")
    timescale = struct.unpack_from(">I", data, a + 12)[0]
    need(timescale == mv_timescale, "mvhd and mdhd timescales differ")
    a, b, _ = one(mdia, b"hdlr")
    need(data[a + 8:a + 12] == b"vide", "hdlr vide")
    _, _, minf = one(mdia, b"minf")
    one(minf, b"vmhd")
    _, _, dinf = one(minf, b"dinf")
    one(dinf, b"dref")
    _, _, stbl = one(minf, b"stbl")
    for typ, size in ((b"stts", 8), (b"stsc", 8), (b"stsz", 12), (b"stco", 8)):
        a, b, _ = one(stbl, typ)
        need(b - a == size and not any(data[a:b]), f"{typ} must be empty")
    a, b, _ = one(stbl, b"stsd")
    need(struct.unpack_from(">II", data, a) == (0, 1), "stsd: one entry")
    (typ, ea, eb), = boxes(data, a + 8, b)
    need(typ == b"avc1", "avc1 sample entry")
    need(struct.unpack_from(">H", data, ea + 6)[0] == 1, "data reference index")
    w, h = struct.unpack_from(">HH", data, ea + 24)
    (typ, ca, cb), = boxes(data, ea + 78, eb)
    need(typ == b"avcC" and data[ca] == 1 and data[ca + 4] == 0xFF and data[ca + 5] == 0xE1, "avcC: version 1, 4-byte lengths, one SPS")
    n = struct.unpack_from(">H", data, ca + 6)[0]
    sps = data[ca + 8:ca + 8 + n]
    need(data[ca + 1:ca + 4] == sps[1:4], "avcC profile / compatibility / level")
    p = ca + 8 + n
    need(data[p] == 1, "one PPS")
    m = struct.unpack_from(">H", data, p + 1)[0]
    pps = data[p + 3:p + 3 + m]
    ext = data[p + 3 + m:cb]
    return dict(timescale=timescale, width=w, height=h, tkhd_width=tw / 65536, tkhd_height=th / 65536,
                sps=bytes(sps), pps=bytes(pps), avcc_ext=bytes(ext), brand=bytes(brand))
