// edgpu_stats.hip -- per-stream reception statistics and the reference's per-stream bitrate,
// computed on the GPU from the rings k_ingest has just filled (gfx950).
//
//   k_stream_stats    one wave64 per stream (track).  The wave walks the track's RTP sender over
//                     the queue indices [StatDev.head, SenderDev.head) in rounds of 64 packets,
//                     then its RTCP sender.  A lane loads one PktMeta (32 B) and, for a packet of
//                     12 bytes or more, the slot's first 16-B word (slot bytes 4..15 are RTP bytes
//                     0..11); the next round's loads are issued before this round's serial part.
//                     Counts, the sequence delta to the previous packet and the transit time are
//                     per lane; only the recurrences are serial: RFC 3550 A.1 update_seq (no
//                     probation) and the A.8 jitter filter.  A round whose 64 packets all carry
//                     the current SSRC with consecutive sequence numbers advances max_seq, cycles
//                     and received in closed form and steps only the jitter filter.  A stream's
//                     row has this one writer, so there are no atomics; the state lives in
//                     registers (wave-uniform) and lane 0 writes it back once per launch.  The
//                     kernel reads rings and SenderDev rows and writes StatDev rows only; every
//                     ring index is masked.
//   k_stream_bitrate  one lane per stream: ReflectorStream::UpdateBitRate (ReflectorStream.h:
//                     542-557), bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "edgpu.h"
#include "edgpu_device.h"
#include "edgpu_params.h"
#include "edgpu_bytes.h"
#include "edgpu_wave.h"
#include "edgpu_rings.h"

namespace edgpu {
namespace {

constexpr uint32_t kRtpSeqMod = 1u << 16;       // RFC 3550 A.1
constexpr uint32_t kMaxDropout = 3000;
constexpr uint32_t kMaxMisorder = 100;
constexpr uint32_t kRtpHeader = 12;             // a packet shorter than this has no seq / ts / SSRC
constexpr uint32_t kSrBytes = 28;               // RTCP header + SSRC + sender info
constexpr uint32_t kRtcpSr = 200;
constexpr int64_t kBitRateAvgIntervalMs = 30000;    // ReflectorStream::kBitRateAvgIntervalInMilSecs

}  // namespace

__global__ __launch_bounds__(64) void k_stream_stats(StatsParams P) {
    const uint32_t s = blockIdx.x;
    if (s >= P.nstreams) return;
    StatDev& S = P.stats[s];
    if (!uni(S.enabled)) return;
    const uint32_t snd = uni(S.sender);
    if (snd + 1 >= P.nsenders) return;
    const SenderDev& D0 = P.senders[snd];
    const SenderDev& D1 = P.senders[snd + 1];
    const uint64_t head0 = uni(D0.head), head1 = uni(D1.head);
    const uint64_t from0 = uni(S.head), from1 = uni(S.rtcp_head);
    if (from0 >= head0 && from1 >= head1) return;          // nothing new
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t interval = 0;                                  // bytes this launch adds to interval_bytes

    if (from0 < head0) {
        Rings R{reinterpret_cast<const u32x4*>(D0.meta), reinterpret_cast<const u32x4*>(D0.ring),
                uni(D0.pk_mask), uni(D0.word_mask)};
        const uint64_t start = uni(intact_from(D0, R, from0, head0));
        const uint32_t clock = uni(S.clock_rate);
        // wave-uniform state
        uint32_t has_src = uni(S.has_src), ssrc = uni(S.ssrc), ssrc_changes = uni(S.ssrc_changes);
        uint32_t base_seq = uni(S.base_seq), max_seq = uni(S.max_seq), cycles = uni(S.cycles), bad_seq = uni(S.bad_seq);
        uint32_t received = uni(S.received), misordered = uni(S.misordered), restarts = uni(S.restarts);
        uint32_t has_transit = uni(S.has_transit), last_transit = uni(S.transit), jitter = uni(S.jitter);
        // per-lane sums, reduced once
        uint32_t n_pk = 0, n_short = 0;
        uint64_t n_by = 0;

        u32x4 a0, a1, b0, b1;
        load_meta(R, start + lane, head0, a0, a1);
        load_meta(R, start + 64 + lane, head0, b0, b1);
        u32x4 w = load_word(R, a0, a1, kRtpHeader, 0);
        for (uint64_t base = start; base < head0; base += 64) {
            // the next round's slot word and the meta of the round after it, ahead of the serial part
            const u32x4 wn = load_word(R, b0, b1, kRtpHeader, 0);
            u32x4 c0, c1;
            load_meta(R, base + 128 + lane, head0, c0, c1);

            const uint32_t len = meta_len(a1);
            const bool rtp = len >= kRtpHeader;
            n_pk += len ? 1u : 0u;
            n_by += len;
            n_short += (len && !rtp) ? 1u : 0u;
            const uint32_t seq = __builtin_bswap32(w.y) & 0xFFFFu;
            const uint32_t ts = __builtin_bswap32(w.z);
            const uint32_t src = __builtin_bswap32(w.w);
            const uint64_t arrival = (uint64_t)a1.x | ((uint64_t)a1.y << 32);
            const uint32_t transit = clock ? (uint32_t)((arrival * clock) / 1000u) - ts : 0u;
            const unsigned long long m_rtp = __ballot(rtp);
            if (m_rtp) {
                uint32_t prev_seq = __shfl_up(seq, 1, 64), prev_tr = __shfl_up(transit, 1, 64);
                if (lane == 0) { prev_seq = max_seq; prev_tr = last_transit; }
                const bool next = rtp && src == ssrc && seq == ((prev_seq + 1) & 0xFFFFu);
                if (has_src && __ballot(next) == ~0ull) {
                    // 64 packets of the current SSRC, each one above the one before it: every udelta
                    // is 1, a wrap is the packet whose seq is 0
                    cycles += kRtpSeqMod * (uint32_t)__popcll(__ballot(seq == 0));
                    max_seq = lane_of(seq, 63);
                    received += 64;
                    if (clock) {
                        const int32_t diff = (int32_t)(transit - prev_tr);
                        const uint32_t d = diff < 0 ? 0u - (uint32_t)diff : (uint32_t)diff;
                        for (uint32_t l = has_transit ? 0u : 1u; l < 64; l++)
                            jitter += lane_of(d, l) - ((jitter + 8) >> 4);
                        last_transit = lane_of(transit, 63);
                        has_transit = 1;
                    }
                } else {
                    for (unsigned long long m = m_rtp; m; m &= m - 1) {
                        const uint32_t l = (uint32_t)__ffsll((long long)m) - 1;
                        const uint32_t q = lane_of(seq, l), sc = lane_of(src, l);
                        if (!has_src || sc != ssrc) {
                            if (has_src) ssrc_changes++;
                            base_seq = max_seq = q; bad_seq = kRtpSeqMod; cycles = 0; received = 0;
                            has_transit = 0; jitter = 0; has_src = 1; ssrc = sc;
                        }
                        const uint32_t udelta = (q - max_seq) & 0xFFFFu;
                        bool accepted = true;
                        if (udelta < kMaxDropout) {
                            if (q < max_seq) cycles += kRtpSeqMod;
                            max_seq = q;
                        } else if (udelta <= kRtpSeqMod - kMaxMisorder) {
                            if (q == bad_seq) {
                                base_seq = max_seq = q; bad_seq = kRtpSeqMod; cycles = 0; received = 0;
                                restarts++;
                            } else {
                                bad_seq = (q + 1) & 0xFFFFu;
                                accepted = false;
                            }
                        } else {
                            misordered++;
                        }
                        if (accepted) {
                            received++;
                            if (clock) {
                                const uint32_t tr = lane_of(transit, l);
                                if (has_transit) {
                                    const int32_t diff = (int32_t)(tr - last_transit);
                                    jitter += (diff < 0 ? 0u - (uint32_t)diff : (uint32_t)diff) - ((jitter + 8) >> 4);
                                }
                                last_transit = tr;
                                has_transit = 1;
                            }
                        }
                    }
                }
            }
            a0 = b0; a1 = b1; b0 = c0; b1 = c1; w = wn;
        }
        const uint64_t by = wave_sum(n_by);
        const uint32_t pk = wave_sum(n_pk), sh = wave_sum(n_short);
        interval += (uint32_t)by;
        if (lane == 0) {
            S.head = head0;
            S.packets += pk; S.bytes += by; S.short_packets += sh;
            S.missed += start - from0;
            S.has_src = has_src; S.ssrc = ssrc; S.ssrc_changes = ssrc_changes;
            S.base_seq = base_seq; S.max_seq = max_seq; S.cycles = cycles; S.bad_seq = bad_seq;
            S.received = received; S.misordered = misordered; S.restarts = restarts;
            S.has_transit = has_transit; S.transit = last_transit; S.jitter = jitter;
        }
    }

    if (from1 < head1) {
        Rings R{reinterpret_cast<const u32x4*>(D1.meta), reinterpret_cast<const u32x4*>(D1.ring),
                uni(D1.pk_mask), uni(D1.word_mask)};
        const uint64_t start = uni(intact_from(D1, R, from1, head1));
        uint32_t sr_count = 0, sr_rtp = 0, sr_packets = 0, sr_octets = 0, sr_lo = 0, sr_hi = 0, sr_alo = 0, sr_ahi = 0;
        uint32_t n_pk = 0;
        uint64_t n_by = 0;
        u32x4 a0, a1, b0, b1;
        load_meta(R, start + lane, head1, a0, a1);
        load_meta(R, start + 64 + lane, head1, b0, b1);
        u32x4 w0 = load_word(R, a0, a1, kSrBytes, 0), w1 = load_word(R, a0, a1, kSrBytes, 1);
        for (uint64_t base = start; base < head1; base += 64) {
            const u32x4 wn0 = load_word(R, b0, b1, kSrBytes, 0), wn1 = load_word(R, b0, b1, kSrBytes, 1);
            u32x4 c0, c1;
            load_meta(R, base + 128 + lane, head1, c0, c1);
            const uint32_t len = meta_len(a1);
            n_pk += len ? 1u : 0u;
            n_by += len;
            // slot byte 5 is RTCP byte 1, the packet type
            const unsigned long long m_sr = __ballot(len >= kSrBytes && ((w0.y >> 8) & 0xFFu) == kRtcpSr);
            if (m_sr) {                                     // the round's last sender report wins
                const uint32_t l = 63u - (uint32_t)__clzll((long long)m_sr);
                sr_count += (uint32_t)__popcll(m_sr);
                sr_hi = __builtin_bswap32(lane_of(w0.w, l));        // RTCP bytes 8-11
                sr_lo = __builtin_bswap32(lane_of(w1.x, l));        // 12-15
                sr_rtp = __builtin_bswap32(lane_of(w1.y, l));       // 16-19
                sr_packets = __builtin_bswap32(lane_of(w1.z, l));   // 20-23
                sr_octets = __builtin_bswap32(lane_of(w1.w, l));    // 24-27
                sr_alo = lane_of(a1.x, l);
                sr_ahi = lane_of(a1.y, l);
            }
            a0 = b0; a1 = b1; b0 = c0; b1 = c1; w0 = wn0; w1 = wn1;
        }
        const uint64_t by = wave_sum(n_by);
        const uint32_t pk = wave_sum(n_pk);
        if (!(uni(D1.flags) & kSndRtcpPort)) interval += (uint32_t)by;      // RTP by port parity (Q12)
        if (lane == 0) {
            S.rtcp_head = head1;
            S.rtcp_packets += pk; S.rtcp_bytes += by;
            S.rtcp_missed += start - from1;
            if (sr_count) {
                S.sr_count += sr_count;
                S.sr_ntp = ((uint64_t)sr_hi << 32) | sr_lo;
                S.sr_rtp = sr_rtp; S.sr_packets = sr_packets; S.sr_octets = sr_octets;
                S.sr_arrival_ms = (int64_t)(((uint64_t)sr_ahi << 32) | sr_alo);
            }
        }
    }
    if (lane == 0 && interval) S.interval_bytes += interval;
}

// ReflectorStream::UpdateBitRate (ReflectorStream.h:542-557): the division and the scaling are two
// fp32 operations, each rounded; intervalBytes * 8 wraps in 32 bits as the reference's does.
__global__ __launch_bounds__(64) void k_stream_bitrate(StatsParams P) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= P.nstreams) return;
    StatDev& S = P.stats[s];
    if (!S.enabled) return;
    const int64_t last = S.last_sample_ms;
    if (last + kBitRateAvgIntervalMs < P.now) {
        const uint32_t bits = S.interval_bytes * 8u;
        float bps = __fdiv_rn((float)bits, (float)(P.now - last));
        bps = __fmul_rn(bps, 1000.f);
        S.bitrate = (uint32_t)bps;
        S.interval_bytes = 0;
        S.last_sample_ms = P.now;
    }
}

hipError_t launch_stream_stats(const StatsParams& p, hipStream_t st) {
    if (p.nstreams) EDGPU_LAUNCH(k_stream_stats, dim3(p.nstreams), dim3(64), 0, st, p);
    return hipGetLastError();
}
hipError_t launch_stream_bitrate(const StatsParams& p, hipStream_t st) {
    if (p.nstreams) EDGPU_LAUNCH(k_stream_bitrate, dim3((p.nstreams + 63) / 64), dim3(64), 0, st, p);
    return hipGetLastError();
}

}  // namespace edgpu
