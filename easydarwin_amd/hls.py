"""HLS segmenter over the transport stream of Context.tap_drain_ts (host only).

A Segmenter takes (ts_bytes, ts_units, streams) per drain and keeps, per (session, track), a
directory `<session>_<track>/` with `seg<n>.ts` files and an `index.m3u8` playlist:

  * units before a stream's first KEY unit are dropped (a segment starts with PAT, PMT and a
    random-access point);
  * a new segment is cut at the first KEY unit whose PTS is at least `segment` seconds after the
    segment's first (PTS differences are unwrapped at 33 bits);
  * a segment's EXTINF is the PTS difference between its first unit and the next segment's first;
    the last segment, closed by close(), ends one unit interval (the last PTS step seen) after its
    last unit;
  * a segment that holds a DAMAGED unit is preceded by #EXT-X-DISCONTINUITY (unless it is the
    stream's first);
  * the playlist is rewritten at each cut with the last `window` segments (0 keeps all) and closed
    with #EXT-X-ENDLIST by close().  EXT-X-TARGETDURATION is the ceiling of the longest segment so
    far.  Files of segments that left the window are kept.
"""
from __future__ import annotations

import math
import os

KEY, DAMAGED = 1, 4             # EDGPU_TAP_KEY, EDGPU_TAP_DAMAGED
CLOCK = 90000
_M33 = 1 << 33


class _Stream:
    def __init__(self, path):
        self.path = path
        self.file = None
        self.n = 0                  # number of the open segment
        self.first = 0              # unwrapped PTS of its first unit
        self.last = None            # unwrapped PTS of the last unit written
        self.step = 0               # the last PTS step
        self.damaged = False
        self.done = []              # (n, seconds, discontinuity)
        self.longest = 0.0


class Segmenter:
    def __init__(self, out_dir: str, segment: float = 2.0, window: int = 0):
        self.out_dir, self.segment, self.window = out_dir, float(segment), int(window)
        self.streams = {}

    def push(self, ts_bytes, ts_units, streams):
        data = memoryview(ts_bytes)
        for row in streams:
            key = (int(row["session"]), int(row["track"]))
            first, count = int(row["unit_first"]), int(row["unit_count"])
            for u in ts_units[first:first + count]:
                self._unit(key, data[int(u["offset"]):int(u["offset"]) + int(u["bytes"])], int(u["pts"]), int(u["flags"]))

    def _unit(self, key, packets, pts, flags):
        s = self.streams.get(key)
        if s is None:
            if not (flags & KEY) or not len(packets):
                return
            s = self.streams[key] = _Stream(os.path.join(self.out_dir, "%d_%d" % key))
            os.makedirs(s.path, exist_ok=True)
        if s.last is None:
            up = pts
        else:
            d = (pts - s.last) % _M33
            up = s.last + (d - _M33 if d >= _M33 // 2 else d)
        if s.file is None:
            self._open(s, up)
        elif (flags & KEY) and len(packets) and up - s.first >= self.segment * CLOCK:
            self._cut(s, up)
            self._open(s, up)
            self._playlist(s, False)
        if s.last is not None:
            s.step = up - s.last
        s.last = up
        s.damaged |= bool(flags & DAMAGED)
        s.file.write(packets)

    def _open(self, s, up):
        s.file = open(os.path.join(s.path, "seg%d.ts" % s.n), "wb")
        s.first, s.damaged = up, False

    def _cut(self, s, end):
        s.file.close()
        s.file = None
        secs = max(end - s.first, 0) / CLOCK
        s.done.append((s.n, secs, s.damaged and s.n > 0))
        s.longest = max(s.longest, secs)
        s.n += 1

    def _playlist(self, s, end):
        rows = s.done[-self.window:] if self.window else s.done
        lines = ["#EXTM3U", "#EXT-X-VERSION:3", "#EXT-X-TARGETDURATION:%d" % max(1, math.ceil(s.longest)),
                 "#EXT-X-MEDIA-SEQUENCE:%d" % (rows[0][0] if rows else 0)]
        for n, secs, disc in rows:
            if disc:
                lines.append("#EXT-X-DISCONTINUITY")
            lines += ["#EXTINF:%.3f," % secs, "seg%d.ts" % n]
        if end:
            lines.append("#EXT-X-ENDLIST")
        tmp = os.path.join(s.path, "index.m3u8.tmp")
        with open(tmp, "w") as f:
            f.write("\n".join(lines) + "\n")
        os.replace(tmp, os.path.join(s.path, "index.m3u8"))

    def close(self):
        for s in self.streams.values():
            if s.file is not None:
                self._cut(s, s.last + max(s.step, 0))
            self._playlist(s, True)

    def summary(self) -> dict:
        return {"%d_%d" % k: dict(segments=len(s.done), seconds=round(sum(r[1] for r in s.done), 3)) for k, s in self.streams.items()}


class _Fmp4Stream(_Stream):
    def __init__(self, path):
        super().__init__(path)
        self.summed = 0             # durations of the open segment's fragments


class Fmp4Segmenter(Segmenter):
    """HLS with fragmented-MP4 segments over Context.tap_drain_mp4: per (session, track) a directory
    with `init.mp4` (edgpu.mp4_init of the first SPS / PPS found in a key fragment), `seg<n>.m4s`
    files of whole fragments and an `index.m3u8` of version 7 with #EXT-X-MAP.

    Fragments before a stream's first key fragment with parameter sets are dropped; a segment is cut
    at the first key fragment whose tfdt is at least `segment` seconds after the segment's first; a
    segment's EXTINF is the tfdt difference to the next segment's first fragment, the last segment's
    the sum of its fragments' durations.  The discontinuity, window and target-duration rules are
    Segmenter's: closing a segment (_cut) and summary() are inherited, and only the playlist's text
    is written here, since Segmenter itself stays as it is."""

    def __init__(self, out_dir: str, segment: float = 2.0, window: int = 0, init=None):
        from . import mp4
        super().__init__(out_dir, segment, window)
        self.init = init or mp4._default_init

    def push(self, data, samples, frags, streams):
        from . import mp4
        data = memoryview(data)
        for f in frags:
            st = streams[int(f["stream"])]
            key = (int(st["session"]), int(st["track"]))
            flags, tfdt = int(f["flags"]), int(f["tfdt"])
            s = self.streams.get(key)
            if s is None:
                if not flags & KEY:
                    continue
                sps, pps = mp4.fragment_parameter_sets(data, samples, f)
                if sps is None or pps is None:
                    continue
                s = self.streams[key] = _Fmp4Stream(os.path.join(self.out_dir, "%d_%d" % key))
                os.makedirs(s.path, exist_ok=True)
                with open(os.path.join(s.path, "init.mp4"), "wb") as fh:
                    fh.write(self.init(sps, pps))
            if s.file is None:
                self._open(s, tfdt)
            elif (flags & KEY) and tfdt - s.first >= self.segment * CLOCK:
                self._cut(s, tfdt)
                self._open(s, tfdt)
                self._playlist(s, False)
            s.last = tfdt
            s.summed += int(f["duration"])
            s.damaged |= bool(flags & DAMAGED)
            s.file.write(data[int(f["offset"]):int(f["offset"]) + int(f["bytes"])])

    def _open(self, s, tfdt):
        s.file = open(os.path.join(s.path, "seg%d.m4s" % s.n), "wb")
        s.first, s.damaged, s.summed = tfdt, False, 0

    def _playlist(self, s, end):
        rows = s.done[-self.window:] if self.window else s.done
        lines = ["#EXTM3U", "#EXT-X-VERSION:7", "#EXT-X-TARGETDURATION:%d" % max(1, math.ceil(s.longest)),
                 "#EXT-X-MEDIA-SEQUENCE:%d" % (rows[0][0] if rows else 0), '#EXT-X-MAP:URI="init.mp4"']
        for n, secs, disc in rows:
            if disc:
                lines.append("#EXT-X-DISCONTINUITY")
            lines += ["#EXTINF:%.3f," % secs, "seg%d.m4s" % n]
        if end:
            lines.append("#EXT-X-ENDLIST")
        tmp = os.path.join(s.path, "index.m3u8.tmp")
        with open(tmp, "w") as f:
            f.write("\n".join(lines) + "\n")
        os.replace(tmp, os.path.join(s.path, "index.m3u8"))

    def close(self):
        for s in self.streams.values():
            if s.file is not None:
                self._cut(s, s.first + s.summed)
            self._playlist(s, True)
