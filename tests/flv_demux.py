"""A strict FLV reader of its own for the FLV mux tests, written from the FLV file-format
specification (Adobe Flash Video File Format Specification 10.1, annex E) -- it shares nothing with
tests/flv_model.py.  Everything the mux and edgpu_flv_header promise about the container is checked
here, and a violation raises DemuxError:

  * the file header: "FLV", version 1, flags 01 (video only), DataOffset 9, PreviousTagSize0 == 0;
  * every tag: type 9 (video) or 18 (script data), the reserved and filter bits clear, stream id 0,
    DataSize within the data, and the PreviousTagSize after it == 11 + DataSize;
  * the timestamp reassembled from its 24 low bits and the extension byte;
  * a video tag: codec 7 (AVC), frame type 1 or 2, packet type 0 (sequence header) or 1 (NALUs),
    composition time 0; a sequence header must be a key frame;
  * packet type 1: 4-byte NAL lengths that tile the rest of the tag exactly;
  * packet type 0: an AVCDecoderConfigurationRecord with version 1, 4-byte lengths, one SPS and one
    PPS that fit, and an extension of 0 or 4 bytes;
  * script data: the AMF0 string "onMetaData" and an ECMA array of number properties with its end
    marker, filling the tag exactly."""
import struct


class DemuxError(Exception):
    pass


def need(cond, what):
    if not cond:
        raise DemuxError(what)


def be(b):
    return int.from_bytes(b, "big")


def annexb(nals):
    return b"".join(b"\x00\x00\x00\x01" + n for n in nals)


def config_record(rec: bytes) -> dict:
    need(len(rec) >= 7 and rec[0] == 1, "AVCDecoderConfigurationRecord: version")
    need(rec[4] == 0xFF, "AVCDecoderConfigurationRecord: lengthSizeMinusOne must be 3, reserved bits set")
    need(rec[5] == 0xE1, "AVCDecoderConfigurationRecord: one SPS, reserved bits set")
    n = be(rec[6:8])
    need(8 + n + 3 <= len(rec), "AVCDecoderConfigurationRecord: the SPS does not fit")
    sps = rec[8:8 + n]
    pos = 8 + n
    need(rec[pos] == 1, "AVCDecoderConfigurationRecord: one PPS")
    m = be(rec[pos + 1:pos + 3])
    need(pos + 3 + m <= len(rec), "AVCDecoderConfigurationRecord: the PPS does not fit")
    pps = rec[pos + 3:pos + 3 + m]
    ext = rec[pos + 3 + m:]
    need(len(ext) in (0, 4), "AVCDecoderConfigurationRecord: trailing bytes")
    need(n >= 4 and sps[0] & 0x1F == 7 and m >= 1 and pps[0] & 0x1F == 8, "AVCDecoderConfigurationRecord: NAL types")
    need(rec[1:4] == sps[1:4], "AVCDecoderConfigurationRecord: profile, compatibility, level")
    return dict(sps=sps, pps=pps, ext=ext, record=rec)


def script_data(d: bytes) -> dict:
    need(d[:13] == b"\x02\x00\x0AonMetaData", "script data: the name")
    need(d[13] == 8, "script data: an ECMA array")
    count, pos, props = be(d[14:18]), 18, {}
    while d[pos:pos + 3] != b"\x00\x00\x09":
        need(pos + 2 <= len(d), "script data: no end marker")
        n = be(d[pos:pos + 2])
        name = d[pos + 2:pos + 2 + n].decode("ascii")
        pos += 2 + n
        need(pos + 9 <= len(d) and d[pos] == 0, "script data: a number")
        props[name] = struct.unpack(">d", d[pos + 1:pos + 9])[0]
        pos += 9
    need(pos + 3 == len(d), "script data: bytes after the end marker")
    need(len(props) == count, "script data: the array's count")
    return props


def tags(data: bytes, pos=0) -> list:
    """The tags from `pos` to the end of `data`: dicts with offset, bytes, type, timestamp and, for
    video, key, packet_type and nals (type 1) or config (type 0); for script data, meta."""
    out = []
    data = bytes(data)
    while pos < len(data):
        need(pos + 15 <= len(data), f"a truncated tag at {pos}")
        t = data[pos]
        need(t in (9, 18), f"tag type {t:#x} at {pos}")
        size = be(data[pos + 1:pos + 4])
        ts = be(data[pos + 4:pos + 7]) | data[pos + 7] << 24
        need(data[pos + 8:pos + 11] == b"\x00\x00\x00", f"stream id at {pos}")
        end = pos + 11 + size
        need(end + 4 <= len(data), f"DataSize {size} of the tag at {pos} leaves the data")
        need(be(data[end:end + 4]) == 11 + size, f"PreviousTagSize after the tag at {pos}")
        d = data[pos + 11:end]
        tag = dict(offset=pos, bytes=size + 15, type=t, timestamp=ts)
        if t == 18:
            need(ts == 0, "script data: timestamp")
            tag["meta"] = script_data(d)
        else:
            need(size >= 5, f"a video tag of {size} data bytes at {pos}")
            need(d[0] & 0x0F == 7, f"codec id at {pos}")
            need(d[0] >> 4 in (1, 2), f"frame type at {pos}")
            need(d[1] in (0, 1), f"AVC packet type at {pos}")
            need(d[2:5] == b"\x00\x00\x00", f"composition time at {pos}")
            tag["key"], tag["packet_type"] = d[0] >> 4 == 1, d[1]
            if d[1] == 0:
                need(tag["key"], "a sequence header that is no key frame")
                tag["config"] = config_record(d[5:])
            else:
                nals, p = [], 5
                while p < len(d):
                    need(p + 4 <= len(d), f"a truncated NAL length in the tag at {pos}")
                    n = be(d[p:p + 4])
                    need(p + 4 + n <= len(d), f"NAL length {n} leaves the tag at {pos}")
                    nals.append(d[p + 4:p + 4 + n])
                    p += 4 + n
                tag["nals"] = nals
        out.append(tag)
        pos = end + 4
    return out


def file(data: bytes) -> list:
    """The tags of a whole file, after its header."""
    data = bytes(data)
    need(data[:3] == b"FLV" and data[3] == 1, "signature and version")
    need(data[4] == 1, "type flags: video only")
    need(be(data[5:9]) == 9, "DataOffset")
    need(data[9:13] == b"\x00\x00\x00\x00", "PreviousTagSize0")
    return tags(data, 13)
