"""Fragmented-MP4 recording over the fragments of Context.tap_drain_mp4 (host only).

A Recorder takes (bytes, samples, frags, streams) per drain and keeps, per (session, track), files
`<session>_<track>_<n>.mp4`: the initialisation segment of edgpu.mp4_init (from the first SPS and PPS
found in a key fragment's first sample), then the stream's fragments as they come -- a file that is
valid after every fragment, with nothing to finalise.

  * fragments before a stream's first key fragment that carries an SPS and a PPS are dropped;
  * a new file starts at the first key fragment whose tfdt is at least `seconds` after the file's
    first (the reference recorder's rule: it cuts on key frames);
  * `init` builds the initialisation segment: edgpu.mp4_init unless another callable is given.
"""
from __future__ import annotations

import os

KEY, PARAMS, DAMAGED = 1, 2, 4      # EDGPU_TAP_KEY, EDGPU_TAP_PARAMS, EDGPU_TAP_DAMAGED
CLOCK = 90000


def parameter_sets(sample) -> tuple:
    """The first SPS and the first PPS among the length-prefixed NALs of one sample: (sps, pps),
    each None when absent."""
    data, pos, sps, pps = bytes(sample), 0, None, None
    while pos + 4 <= len(data) and (sps is None or pps is None):
        n = int.from_bytes(data[pos:pos + 4], "big")
        nal = data[pos + 4:pos + 4 + n]
        if nal and (nal[0] & 0x1F) == 7 and sps is None:
            sps = nal
        if nal and (nal[0] & 0x1F) == 8 and pps is None:
            pps = nal
        pos += 4 + n
    return sps, pps


def fragment_parameter_sets(data, samples, frag) -> tuple:
    """parameter_sets of the fragment's first sample."""
    row = samples[int(frag["unit_first"])]
    return parameter_sets(data[int(row["offset"]):int(row["offset"]) + int(row["bytes"])])


def _default_init(sps, pps):
    from . import edgpu
    return edgpu.mp4_init(sps, pps)


class _File:
    def __init__(self):
        self.file = None
        self.name = None
        self.n = 0
        self.first = 0
        self.init = None
        self.done = []              # (name, fragments)
        self.frags = 0


class Recorder:
    def __init__(self, out_dir: str, seconds: float = 300.0, init=None):
        self.out_dir, self.seconds, self.init = out_dir, float(seconds), init or _default_init
        self.streams = {}
        os.makedirs(out_dir, exist_ok=True)

    def push(self, data, samples, frags, streams):
        data = memoryview(data)
        for f in frags:
            st = streams[int(f["stream"])]
            self._fragment((int(st["session"]), int(st["track"])), data, samples, f)

    def _fragment(self, key, data, samples, f):
        s = self.streams.setdefault(key, _File())
        key_frag = bool(int(f["flags"]) & KEY)
        if s.init is None:
            if not key_frag:
                return
            sps, pps = fragment_parameter_sets(data, samples, f)
            if sps is None or pps is None:
                return
            s.init = self.init(sps, pps)
        tfdt = int(f["tfdt"])
        if s.file is not None and key_frag and tfdt - s.first >= self.seconds * CLOCK:
            self._close(s)
        if s.file is None:
            if not key_frag:
                return
            name = "%d_%d_%d.mp4" % (key[0], key[1], s.n)
            s.file, s.first, s.frags, s.name = open(os.path.join(self.out_dir, name), "wb"), tfdt, 0, name
            s.file.write(s.init)
        s.file.write(data[int(f["offset"]):int(f["offset"]) + int(f["bytes"])])
        s.frags += 1

    def _close(self, s):
        s.file.close()
        s.file = None
        s.done.append((s.name, s.frags))
        s.n += 1

    def close(self):
        for s in self.streams.values():
            if s.file is not None:
                self._close(s)

    def summary(self) -> dict:
        return {"%d_%d" % k: dict(files=[n for n, _ in s.done], fragments=sum(c for _, c in s.done)) for k, s in self.streams.items()}
