"""FLV recording and live joining over the tags of Context.tap_drain_flv (host only).

Both classes take (bytes, tags, streams) per drain.  A tag row says where its tag is, whether it is
a key frame and where the SPS and the PPS lie in it, so nothing here parses a tag.

A Recorder keeps, per (session, track), files `<session>_<track>_<n>.flv`:
  * tags before a stream's first key tag that reports an SPS and a PPS are dropped;
  * a file begins with the file header, onMetaData and the AVC sequence header (edgpu.flv_header),
    then the stream's tags as they come; whenever the reported SPS or PPS bytes change, a new
    sequence header at that tag's timestamp precedes the tag;
  * a new file starts at the first key tag whose timestamp is at least `seconds` after the file's
    first (the rule of mp4.Recorder: it cuts on key frames);
  * `header` builds those bytes: edgpu.flv_header unless another callable (sps, pps, timestamp_ms,
    parts) is given.

A LiveStream is what an HTTP-FLV or RTMP front end keeps per stream: `push` each drain's tags,
`join()` gives a new viewer (bytes, cursor) -- the file header, onMetaData, the sequence header and
every tag since the latest key tag -- and `tags_since(cursor)` what followed.  It holds the current
GOP (and, until the next push, what the last push brought of the GOP before, so that a viewer who
asks after every push misses nothing); an older cursor resumes at the latest key tag.
"""
from __future__ import annotations

import os

KEY, PARAMS, DAMAGED = 1, 2, 4      # EDGPU_TAP_KEY, EDGPU_TAP_PARAMS, EDGPU_TAP_DAMAGED
FILE, META, SEQ = 1, 2, 4           # EDGPU_FLV_FILE, EDGPU_FLV_META, EDGPU_FLV_SEQ


def _default_header(sps, pps, timestamp_ms=0, parts=0):
    from . import edgpu
    return edgpu.flv_header(sps, pps, timestamp_ms, parts)


def parameter_sets(data, tag) -> tuple:
    """The SPS and the PPS a tag row reports: (sps, pps), each None when absent."""
    base = int(tag["offset"])

    def cut(off, n):
        return bytes(data[base + int(off):base + int(off) + int(n)]) if int(n) else None
    return cut(tag["sps_offset"], tag["sps_bytes"]), cut(tag["pps_offset"], tag["pps_bytes"])


def _stream_tags(tags, streams):
    """((session, track), tag row) of every tag with bytes, in output order."""
    for t in tags:
        if int(t["bytes"]):
            st = streams[int(t["stream"])]
            yield (int(st["session"]), int(st["track"])), t


class _Params:
    """The parameter sets in force for one stream, and whether a tag changes them."""

    def __init__(self):
        self.sps = self.pps = None

    def update(self, data, tag) -> bool:
        """True when the tag reports an SPS or a PPS that differs from the one in force."""
        if not int(tag["flags"]) & PARAMS:
            return False
        sps, pps = parameter_sets(data, tag)
        changed = (sps is not None and sps != self.sps) or (pps is not None and pps != self.pps)
        self.sps, self.pps = sps if sps is not None else self.sps, pps if pps is not None else self.pps
        return changed

    @property
    def known(self):
        return self.sps is not None and self.pps is not None


class _File:
    def __init__(self):
        self.file = None
        self.name = None
        self.n = 0
        self.first = 0
        self.params = _Params()
        self.started = False
        self.done = []              # (name, tags)
        self.tags = 0


class Recorder:
    def __init__(self, out_dir: str, seconds: float = 300.0, header=None):
        self.out_dir, self.seconds, self.header = out_dir, float(seconds), header or _default_header
        self.streams = {}
        os.makedirs(out_dir, exist_ok=True)

    def push(self, data, tags, streams):
        data = memoryview(data)
        for key, t in _stream_tags(tags, streams):
            self._tag(key, data, t)

    def _tag(self, key, data, t):
        s = self.streams.setdefault(key, _File())
        is_key = bool(int(t["flags"]) & KEY)
        ms = int(t["timestamp_ms"])
        if not s.started and not is_key:
            return
        changed = s.params.update(data, t)
        if not s.started:
            if not s.params.known:
                return
            s.started = True
        if s.file is not None and is_key and ms - s.first >= self.seconds * 1000:
            self._close(s)
        if s.file is None:
            if not is_key:
                return
            name = "%d_%d_%d.flv" % (key[0], key[1], s.n)
            s.file, s.first, s.tags, s.name = open(os.path.join(self.out_dir, name), "wb"), ms, 0, name
            s.file.write(self.header(s.params.sps, s.params.pps, ms, 0))
        elif changed:
            s.file.write(self.header(s.params.sps, s.params.pps, ms, SEQ))
        s.file.write(data[int(t["offset"]):int(t["offset"]) + int(t["bytes"])])
        s.tags += 1

    def _close(self, s):
        s.file.close()
        s.file = None
        s.done.append((s.name, s.tags))
        s.n += 1

    def close(self):
        for s in self.streams.values():
            if s.file is not None:
                self._close(s)

    def summary(self) -> dict:
        return {"%d_%d" % k: dict(files=[n for n, _ in s.done], tags=sum(c for _, c in s.done)) for k, s in self.streams.items()}


class LiveStream:
    """One stream's current GOP.  `push` takes a whole drain and keeps the tags of `key` = (session, track).
    The tail of the GOP before stays until the next push, so that a viewer who asks tags_since after
    every push misses nothing when a drain holds a key tag."""

    def __init__(self, key, header=None):
        self.key, self.header = tuple(key), header or _default_header
        self.params = _Params()
        self.buf = []               # per tag: (the sequence header before it when it changed a parameter set, or b"", its bytes)
        self.key_at = 0             # of the latest key tag in buf
        self.first = 0              # cursor of buf[0]: tags dropped so far
        self.start_ms = 0           # of the latest key tag
        self.start_params = None    # (sps, pps) in force at it

    def push(self, data, tags, streams):
        data = memoryview(data)
        del self.buf[:self.key_at]                          # what the last push left of the GOP before
        self.first, self.key_at = self.first + self.key_at, 0
        for key, t in _stream_tags(tags, streams):
            if key != self.key:
                continue
            is_key = bool(int(t["flags"]) & KEY)
            if not self.buf and not is_key:
                continue
            changed = self.params.update(data, t)
            if not self.params.known:
                continue
            body = bytes(data[int(t["offset"]):int(t["offset"]) + int(t["bytes"])])
            ms = int(t["timestamp_ms"])
            if is_key:
                self.key_at = len(self.buf)
                self.start_ms, self.start_params = ms, (self.params.sps, self.params.pps)
            seq = self.header(self.params.sps, self.params.pps, ms, SEQ) if changed and self.buf else b""
            self.buf.append((seq, body))

    @property
    def ready(self) -> bool:
        return bool(self.buf)

    @property
    def gop(self) -> list:
        """The tags since the latest key tag."""
        return self.buf[self.key_at:]

    def _from_key(self, parts):
        """The header parts at the latest key tag, then that tag and what followed it."""
        gop = self.gop
        head = self.header(self.start_params[0], self.start_params[1], self.start_ms, parts)
        return head + gop[0][1] + b"".join(seq + body for seq, body in gop[1:])

    def join(self):
        """-> (bytes, cursor): everything a new viewer needs up to now; None before the first key tag."""
        if not self.buf:
            return None
        return self._from_key(0), self.first + len(self.buf)

    def tags_since(self, cursor: int):
        """-> (bytes, cursor): the tags pushed since `cursor`.  A cursor that fell out of the buffer
        resumes at the latest key tag, behind a sequence header."""
        end = self.first + len(self.buf)
        if cursor >= end:
            return b"", end
        if cursor < self.first:
            return self._from_key(SEQ), end
        return b"".join(seq + body for seq, body in self.buf[cursor - self.first:]), end
