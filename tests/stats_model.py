"""Plain-Python restatement of the per-stream statistics (include/edgpu.h, "Per-stream reception
statistics"): RFC 3550 A.1 update_seq without probation, the A.8 jitter filter, the RTCP sender
report capture and ReflectorStream::UpdateBitRate in numpy.float32.

A model is fed (channel, arrival_ms, final bytes) tuples in queue order -- "final" meaning what the
engine keeps of the packet: clamped to 2060 bytes, emptied by the SSRC filter, its receive-time
trailer stripped.  Empty packets are skipped everywhere.  Nothing here comes from the engine.
"""
import numpy as np

MAX_PACKET = 2060
MAX_DROPOUT = 3000
MAX_MISORDER = 100
SEQ_MOD = 1 << 16
BITRATE_INTERVAL_MS = 30000
M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF

# fields of a record the GPU tests compare with the engine's edgpu_stream_stats
FIELDS = ("clock_rate", "packets", "bytes", "missed", "short_packets", "has_src", "ssrc", "ssrc_changes",
          "base_seq", "max_seq", "cycles", "bad_seq", "received", "misordered", "restarts", "expected", "lost",
          "jitter", "jitter_scaled", "has_transit", "transit", "rtcp_packets", "rtcp_bytes", "rtcp_missed",
          "sr_count", "sr_rtp", "sr_ntp", "sr_packets", "sr_octets", "sr_arrival_ms",
          "interval_bytes", "bitrate", "last_sample_ms")


def clock_rate_of(name) -> int:
    """The decimal digits after the first '/' of an rtpmap name; 0 without a '/' or digits."""
    if isinstance(name, bytes):
        name = name.decode("latin-1")
    p = name.find("/")
    if p < 0:
        return 0
    v = 0
    for c in name[p + 1:]:
        if not ("0" <= c <= "9"):
            break
        v = v * 10 + int(c)
        if v > M32:
            return 0
    return v


def clamp(data: bytes) -> bytes:
    return data[:MAX_PACKET]


class StreamModel:
    def __init__(self, clock_rate: int, udp_push: bool, enable_ms: int):
        self.clock_rate = clock_rate
        self.udp_push = udp_push
        self.packets = self.bytes = self.missed = self.short_packets = 0
        self.has_src = self.ssrc = self.ssrc_changes = 0
        self.base_seq = self.max_seq = self.cycles = self.bad_seq = 0
        self.received = self.misordered = self.restarts = 0
        self.has_transit = self.transit = self.jitter_scaled = 0
        self.rtcp_packets = self.rtcp_bytes = self.rtcp_missed = 0
        self.sr_count = self.sr_rtp = self.sr_ntp = self.sr_packets = self.sr_octets = self.sr_arrival_ms = 0
        self.interval_bytes = self.bitrate = 0
        self.last_sample_ms = enable_ms

    def _init_seq(self, seq):
        self.base_seq = self.max_seq = seq
        self.bad_seq = SEQ_MOD
        self.cycles = 0
        self.received = 0

    def push(self, kind: int, arrival_ms: int, data: bytes):
        """kind 0: the track's RTP sender (even channel), 1: its RTCP sender."""
        n = len(data)
        if n == 0:
            return
        if kind == 0 or not self.udp_push:          # RTP by port parity
            self.interval_bytes = (self.interval_bytes + n) & M32
        if kind == 1:
            self.rtcp_packets += 1
            self.rtcp_bytes += n
            if n >= 28 and data[1] == 200:
                self.sr_count += 1
                self.sr_ntp = int.from_bytes(data[8:16], "big")
                self.sr_rtp = int.from_bytes(data[16:20], "big")
                self.sr_packets = int.from_bytes(data[20:24], "big")
                self.sr_octets = int.from_bytes(data[24:28], "big")
                self.sr_arrival_ms = arrival_ms
            return
        self.packets += 1
        self.bytes += n
        if n < 12:
            self.short_packets += 1
            return
        seq = int.from_bytes(data[2:4], "big")
        ts = int.from_bytes(data[4:8], "big")
        ssrc = int.from_bytes(data[8:12], "big")
        if not self.has_src or ssrc != self.ssrc:
            if self.has_src:
                self.ssrc_changes += 1
            self._init_seq(seq)
            self.has_transit = 0
            self.jitter_scaled = 0
            self.has_src = 1
            self.ssrc = ssrc
        udelta = (seq - self.max_seq) & 0xFFFF
        accepted = True
        if udelta < MAX_DROPOUT:
            if seq < self.max_seq:
                self.cycles = (self.cycles + SEQ_MOD) & M32
            self.max_seq = seq
        elif udelta <= SEQ_MOD - MAX_MISORDER:
            if seq == self.bad_seq:
                self._init_seq(seq)
                self.restarts += 1
            else:
                self.bad_seq = (seq + 1) & 0xFFFF
                accepted = False
        else:
            self.misordered += 1
        if not accepted:
            return
        self.received = (self.received + 1) & M32
        if self.clock_rate:
            arrival_rtp = ((((arrival_ms & M64) * self.clock_rate) & M64) // 1000) & M32
            transit = (arrival_rtp - ts) & M32
            if self.has_transit:
                d = (transit - self.transit) & M32
                if d >= 1 << 31:
                    d = (1 << 32) - d
                self.jitter_scaled = (self.jitter_scaled + d - ((self.jitter_scaled + 8) >> 4)) & M32
            self.transit = transit
            self.has_transit = 1

    def sample(self, now: int):
        """ReflectorStream::UpdateBitRate (ReflectorStream.h:542-557) in float32."""
        if self.last_sample_ms + BITRATE_INTERVAL_MS < now:
            bits = (self.interval_bytes * 8) & M32
            bps = np.float32(bits) / np.float32(now - self.last_sample_ms)
            bps = np.float32(bps * np.float32(1000))
            self.bitrate = int(bps)
            self.interval_bytes = 0
            self.last_sample_ms = now

    @property
    def expected(self):
        return (self.cycles + self.max_seq - self.base_seq + 1) & M32 if self.has_src else 0

    def record(self) -> dict:
        r = {k: getattr(self, k) for k in FIELDS if k not in ("lost", "jitter")}
        r["lost"] = self.expected - self.received
        r["jitter"] = self.jitter_scaled >> 4
        return r


class SessionModel:
    """One model per track; `names` are the tracks' rtpmap names."""

    def __init__(self, names, udp_push: bool, enable_ms: int):
        self.tracks = [StreamModel(clock_rate_of(n), udp_push, enable_ms) for n in names]

    def push(self, channel: int, arrival_ms: int, data: bytes):
        t = channel // 2
        if t < len(self.tracks):
            self.tracks[t].push(channel & 1, arrival_ms, clamp(data))

    def sample(self, now: int):
        for t in self.tracks:
            t.sample(now)

    def bitrate(self) -> int:
        return sum(t.bitrate for t in self.tracks) & M32

    def records(self) -> list:
        return [t.record() for t in self.tracks]
