// edgpu_mp4.hip -- the fragmented-MP4 mux of tapped H.264 access units (gfx950).  The rules are
// stated in include/edgpu.h (edgpu_mp4_mux) and restated on the CPU in tests/mp4_model.py.  One call
// is six kernels:
//
//   k_mp4_mark     the bitmap of the ES's start codes and each 2-KiB chunk's first one
//   k_mp4_resolve  for every start code the distance from its end to the next one (both are
//                  edgpu_scode.h, shared with the FLV mux)
//   k_mp4_plan     one wave64 per stream row, its units in rounds of 64: the extended timestamp, the
//                  sample ranks, the fragment starts (first sample, key units, max_samples), each
//                  sample's place in its fragment, the durations (the lane of a sample writes the
//                  duration of the sample before it) and the new state row, with the carries in
//                  wave-uniform registers.  A lane that starts a fragment leaves an Mp4FragRec: the
//                  stream's sums before it, which close the fragment before it.
//   k_mp4_place    one workgroup sums the streams' bytes (runs are 16-B aligned) and fragments in
//                  blocks of 256 and alone decides whether the call commits.
//   k_mp4_rows     flat: the fragment rows (differences of neighbouring Mp4FragRecs), the sample rows
//                  and the streams' sample lists, in staging.
//   k_mp4_pack     flat over the output's 16-B words.  A word that lies inside one sample and touches
//                  no start code is one 16-B store funnelled from two aligned 16-B loads; any other
//                  word (box headers, trun rows, NAL lengths, sample and stream edges) is assembled
//                  byte by byte.  Every byte of a run is written once, nothing outside the runs.
//
// No atomics, no LDS outside the placement scan, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "edgpu.h"
#include "edgpu_device.h"
#include "edgpu_params.h"
#include "edgpu_bytes.h"
#include "edgpu_wave.h"
#include "edgpu_scode.h"

namespace edgpu {
namespace {

constexpr uint32_t kMp4PlaceThreads = 256;
}  // namespace

__global__ __launch_bounds__(256) void k_mp4_mark(Mp4Params P) { scode_mark(P.sc); }

__global__ __launch_bounds__(256) void k_mp4_resolve(Mp4Params P) { scode_resolve(P.sc); }

__global__ __launch_bounds__(64) void k_mp4_plan(Mp4Params P) {
    const uint32_t s = blockIdx.x;
    if (s >= P.n_streams) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t first = uni(P.ranges[s].first), count = uni(P.ranges[s].count), slot0 = uni(P.ranges[s].slot);
    const edgpu_mp4_state st = P.states[s];
    const uint32_t started = uni(st.started);
    uint64_t c_ext = uni(started ? st.ext_ts : (uint64_t)0);
    uint64_t origin = uni(st.origin);
    if (!started && count) origin = uni(P.units[first].rtp_ts);
    const uint32_t maxs = P.max_samples;
    uint32_t c_rank = 0, c_bytes = 0, c_nfrag = 0, c_seg1 = 0, c_fragb1 = 0, c_or = 0;
    uint32_t c_prev_unit = 0, c_has_prev = 0, c_step = uni(st.last_step);
    uint64_t c_dsum = 0, c_prev_ext = 0;
    for (uint32_t base = 0; base < count; base += 64) {
        const uint32_t i = base + lane;
        const bool valid = i < count;
        uint64_t off = 0;
        uint32_t bytes = 0, ts = 0, flags = 0;
        if (valid) {
            const edgpu_tap_unit u = P.units[first + i];
            off = u.offset; bytes = u.bytes; ts = u.rtp_ts; flags = u.flags;
        }
        const bool hasb = bytes != 0;
        const uint32_t has = hasb ? 1u : 0u;
        if (hasb && !(bytes >= 4 && ((P.sc.bitmap[off >> 5] >> (off & 31u)) & 1u))) flags |= EDGPU_TAP_DAMAGED;
        // the extended timestamp, as the transport-stream mux extends it
        uint32_t prev_ts = __shfl_up(ts, 1, 64);
        if (lane == 0) prev_ts = (uint32_t)c_ext;
        uint64_t d = valid ? (uint64_t)(int64_t)(int32_t)(ts - prev_ts) : 0ull;
        if (valid && i == 0 && !started) d = ts;
        const uint64_t in_d = wave_incl(d, lane);
        const uint64_t ext = c_ext + in_d;
        const uint64_t dts = ext - origin + P.time_offset;
        // ranks, bytes, fragment starts
        const uint32_t in_has = wave_incl(has, lane), in_b = wave_incl(bytes, lane);
        const uint32_t r = c_rank + in_has - has;
        const uint32_t bex = c_bytes + in_b - bytes;
        const bool key = hasb && (flags & EDGPU_TAP_KEY);
        const bool segstart = hasb && (key || r == 0);
        const uint32_t in_seg = wave_incl_max(segstart ? r + 1 : 0u, lane);
        const uint32_t seg1 = in_seg > c_seg1 ? in_seg : c_seg1;          // rank + 1 of the last key (or first) sample
        const uint32_t pos = hasb ? r - (seg1 - 1) : 0u;
        const bool fragstart = hasb && (maxs ? pos % maxs == 0 : pos == 0);
        const uint32_t in_fs = wave_incl(fragstart ? 1u : 0u, lane);
        const uint32_t fi = c_nfrag + in_fs - 1;                           // of a sample: its fragment, within the stream
        const uint32_t in_fb = wave_incl_max(fragstart ? bex + 1 : 0u, lane);
        const uint32_t fragb1 = in_fb > c_fragb1 ? in_fb : c_fragb1;
        // OR of the flags within the fragment so far: a segmented scan, heads at the fragment starts
        uint32_t ov = hasb ? flags : 0u, of = fragstart ? 1u : 0u;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t uv = __shfl_up(ov, o, 64), uf = __shfl_up(of, o, 64);
            if (lane >= (uint32_t)o) { if (!of) ov |= uv; of |= uf; }
        }
        if (!of) ov |= c_or;
        uint32_t prev_or = __shfl_up(ov, 1, 64);
        if (lane == 0) prev_or = c_or;
        // the sample before this one: its duration is known here
        uint32_t pl = __shfl_up(wave_incl_max(hasb ? lane + 1 : 0u, lane), 1, 64);
        if (lane == 0) pl = 0;
        const uint64_t pext_w = shfl64(ext, pl ? pl - 1 : 0u);
        const bool hp = hasb && (pl || c_has_prev);
        const uint64_t pext = pl ? pext_w : c_prev_ext;
        const uint32_t punit = pl ? first + base + pl - 1 : c_prev_unit;
        uint32_t dp = 0;
        bool positive = false;
        if (hp) {
            const int64_t diff = (int64_t)(ext - pext);
            positive = diff > 0;
            dp = diff <= 0 ? 0u : diff > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)diff;
            P.recs[punit].duration = dp;
        }
        const uint64_t in_dp = wave_incl((uint64_t)dp, lane);
        if (valid) {
            Mp4Rec* r_ = &P.recs[first + i];                // every field but `duration`: the next sample's lane writes that
            r_->dts = dts;
            r_->slot = hasb ? slot0 + fi : kMp4None;
            r_->poff = hasb ? bex - (fragb1 - 1) : 0u;
            r_->rank = r;
            r_->flags = flags | ((hasb ? 2u : 1u) << 30);
            r_->_pad = 0;
            if (!hasb) r_->duration = 0;
        }
        if (fragstart) {
            Mp4FragRec f;
            f.tfdt = dts;
            f.dsum = c_dsum + in_dp;
            f.unit_first = first + i;
            f.rank = r;
            f.bex = bex;
            f.prev_or = prev_or;
            P.frecs[slot0 + fi] = f;
        }
        // carries
        c_ext += lane_of(in_d, 63);
        c_rank += lane_of(in_has, 63);
        c_bytes += lane_of(in_b, 63);
        c_nfrag += lane_of(in_fs, 63);
        c_dsum += lane_of(in_dp, 63);
        c_seg1 = lane_of(seg1, 63);
        c_fragb1 = lane_of(fragb1, 63);
        c_or = lane_of(ov, 63);
        const uint64_t pb = __ballot(positive);
        if (pb) c_step = lane_of(dp, 63u - (uint32_t)__builtin_clzll(pb));
        const uint64_t hb = __ballot(hasb);
        if (hb) {
            const uint32_t hl = 63u - (uint32_t)__builtin_clzll(hb);
            c_prev_ext = lane_of(ext, hl);
            c_prev_unit = first + base + hl;
            c_has_prev = 1;
        }
    }
    if (lane == 0) {
        uint32_t ld = 0;
        if (c_has_prev) {
            ld = c_step ? c_step : P.default_duration;
            P.recs[c_prev_unit].duration = ld;
        }
        Mp4FragRec f;
        f.tfdt = 0;
        f.dsum = c_dsum + ld;
        f.unit_first = 0;
        f.rank = c_rank;
        f.bex = c_bytes;
        f.prev_or = c_or;
        P.frecs[slot0 + c_nfrag] = f;
        edgpu_mp4_state n = st;
        if (count) {
            n.ext_ts = c_ext;
            n.origin = origin;
            n.sequence = st.sequence + c_nfrag;
            n.last_step = c_step;
            n.started = 1;
        }
        P.new_states[s] = n;
        Mp4StreamRec sr;
        sr.bytes = 96ull * c_nfrag + 12ull * c_rank + c_bytes;
        sr.base = 0;
        sr.nfrags = c_nfrag;
        sr.fbase = 0;
        P.srecs[s] = sr;
    }
}

__global__ __launch_bounds__(256) void k_mp4_place(Mp4Params P) {
    __shared__ uint64_t scratch[kMp4PlaceThreads / 64];
    const uint32_t t = threadIdx.x;
    uint64_t cb = 0, cf = 0;
    for (uint32_t b = 0; b < P.n_streams; b += kMp4PlaceThreads) {
        const uint32_t i = b + t;
        const uint64_t vf = i < P.n_streams ? P.srecs[i].nfrags : 0ull;
        uint64_t tb, tf;
        const uint64_t base = cb + place_round(P.srecs, P.n_streams, i, scratch, tb);
        const uint64_t fbase = cf + block_exclusive_scan<uint64_t>(vf, scratch, tf);
        if (i < P.n_streams) {
            P.srecs[i].base = base;
            P.srecs[i].fbase = fbase > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)fbase;
        }
        cb += tb;
        cf += tf;
    }
    if (t == 0) {
        const uint64_t total = place_total(P.srecs, P.n_streams, cb);
        Mp4Place pl;
        pl.bytes = total;
        pl.frags = cf > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)cf;
        pl.commit = (total <= P.out_cap && cf <= P.frag_cap) ? 1u : 0u;
        *P.place = pl;
    }
}

namespace {

// The stream row whose Mp4FragRecs hold slot `j`
__device__ __forceinline__ uint32_t m_stream_of_slot(const Mp4Params& P, uint32_t j) {
    uint32_t lo = 0, hi = P.n_streams;                      // ranges[lo].slot <= j < ranges[hi].slot
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (P.ranges[mid].slot <= j) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace

__global__ __launch_bounds__(256) void k_mp4_rows(Mp4Params P) {
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = gid; j < P.n_slots; j += nthreads) {
        const uint32_t s = m_stream_of_slot(P, (uint32_t)j);
        const uint32_t fi = (uint32_t)j - P.ranges[s].slot;
        const Mp4StreamRec sr = P.srecs[s];
        if (fi >= sr.nfrags) continue;
        const Mp4FragRec a = P.frecs[j], b = P.frecs[j + 1];
        const uint32_t n = b.rank - a.rank;
        edgpu_mp4_frag f;
        f.offset = sr.base + 96ull * fi + 12ull * a.rank + a.bex;
        f.tfdt = a.tfdt;
        f.duration = b.dsum - a.dsum;
        f.bytes = 96u + 12u * n + (b.bex - a.bex);
        f.sequence = P.states[s].sequence + fi + 1;
        f.unit_first = a.unit_first;
        f.samples = n;
        f.flags = b.prev_or;
        f.stream = s;
        P.frags[(uint64_t)sr.fbase + fi] = f;               // staging holds n_units rows: in range whatever the verdict
    }
    for (uint64_t i = gid; i < P.n_units; i += nthreads) {
        const Mp4Rec r = P.recs[i];
        const uint32_t kind = r.flags >> 30;
        edgpu_mp4_sample o;
        o.offset = 0; o.dts = 0; o.bytes = 0; o.duration = 0; o.flags = 0; o.fragment = 0;
        if (kind == 1) {
            o.dts = r.dts;
            o.flags = r.flags & 0x3FFFFFFFu;
            o.fragment = kMp4None;
        } else if (kind == 2) {
            const uint32_t s = m_stream_of_slot(P, r.slot);
            const Mp4Range rg = P.ranges[s];
            const Mp4StreamRec sr = P.srecs[s];
            const uint32_t fi = r.slot - rg.slot;
            const Mp4FragRec a = P.frecs[r.slot], b = P.frecs[r.slot + 1];
            const uint32_t n = b.rank - a.rank;
            const uint64_t rel = 96ull * fi + 12ull * a.rank + a.bex + 96u + 12ull * n + r.poff;
            o.offset = sr.base + rel;
            o.dts = r.dts;
            o.bytes = P.units[i].bytes;
            o.duration = r.duration;
            o.flags = r.flags & 0x3FFFFFFFu;
            o.fragment = sr.fbase + fi;
            Mp4Samp sm;
            sm.off = rel; sm.unit = (uint32_t)i; sm._pad = 0;
            P.samps[rg.first + r.rank] = sm;
        }
        P.rows[i] = o;
    }
}

namespace {

// What k_mp4_pack knows about the fragment and the sample its current byte is in
struct Mp4Cur {
    uint64_t foff;          // of the fragment, relative to the stream's run
    uint32_t fbytes, n, hdr;    // hdr = 96 + 12 n: moof and the mdat header
    uint32_t seq;
    uint64_t tfdt;
    uint64_t samp0;         // of its first sample in the sample list
    // the sample
    uint32_t k;             // within the fragment; kMp4None: not looked up
    uint64_t s_off;         // relative to the stream's run
    uint64_t s_src;         // of its unit in the ES
    uint32_t s_bytes;
};

__device__ __forceinline__ void m_load_frag(const Mp4Params& P, Mp4Cur& c, const Mp4StreamRec& sr, const Mp4Range& rg, uint32_t f) {
    const edgpu_mp4_frag fr = P.frags[f];
    c.foff = fr.offset - sr.base;
    c.fbytes = fr.bytes;
    c.n = fr.samples;
    c.hdr = 96u + 12u * fr.samples;
    c.seq = fr.sequence;
    c.tfdt = fr.tfdt;
    c.samp0 = (uint64_t)rg.first + P.frecs[rg.slot + (f - sr.fbase)].rank;
    c.k = kMp4None;
}

__device__ __forceinline__ void m_load_sample(const Mp4Params& P, Mp4Cur& c, uint32_t k) {
    const Mp4Samp sm = P.samps[c.samp0 + k];
    const edgpu_tap_unit u = P.units[sm.unit];
    c.k = k;
    c.s_off = sm.off;
    c.s_src = u.offset;
    c.s_bytes = u.bytes;
}

// The sample of the fragment that holds byte `rel` of the stream's run (rel is in the mdat payload)
__device__ __forceinline__ void m_find_sample(const Mp4Params& P, Mp4Cur& c, uint64_t rel) {
    uint32_t lo = 0, hi = c.n;                              // samps[lo].off <= rel < samps[hi].off
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (P.samps[c.samp0 + mid].off <= rel) lo = mid; else hi = mid;
    }
    m_load_sample(P, c, lo);
}

// Big-endian dword `j` of the fragment's moof and mdat header
__device__ __forceinline__ uint32_t m_hdr_word(const Mp4Params& P, const Mp4Cur& c, uint32_t j) {
    const uint32_t H = c.hdr - 8;
    if (j >= 22 && j < 22 + 3 * c.n) {
        const uint32_t k = (j - 22) / 3, e = (j - 22) - 3 * k;
        const edgpu_mp4_sample* row = &P.rows[P.samps[c.samp0 + k].unit];
        return e == 0 ? row->duration : e == 1 ? row->bytes : (row->flags & EDGPU_TAP_KEY) ? 0x02000000u : 0x01010000u;
    }
    if (j == 22 + 3 * c.n) return c.fbytes - H;             // mdat: 8 + the samples
    if (j == 23 + 3 * c.n) return 0x6D646174u;
    switch (j) {
        case 0: return H;
        case 1: return 0x6D6F6F66u;                         // moof
        case 2: case 8: return 16u;
        case 3: return 0x6D666864u;                         // mfhd
        case 5: return c.seq;
        case 6: return H - 24;
        case 7: return 0x74726166u;                         // traf
        case 9: return 0x74666864u;                         // tfhd
        case 10: return 0x00020000u;
        case 11: return 1u;
        case 12: return 20u;
        case 13: return 0x74666474u;                        // tfdt
        case 14: return 0x01000000u;
        case 15: return (uint32_t)(c.tfdt >> 32);
        case 16: return (uint32_t)c.tfdt;
        case 17: return 20u + 12u * c.n;
        case 18: return 0x7472756Eu;                        // trun
        case 19: return 0x00000701u;
        case 20: return c.n;
        case 21: return c.hdr;
        default: return 0u;                                 // 4
    }
}

}  // namespace

__global__ __launch_bounds__(256) void k_mp4_pack(Mp4Params P) {
    const Mp4Place pl = *P.place;
    if (!pl.commit) return;
    const uint64_t nwords = (pl.bytes + 15) >> 4;
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t w = gid; w < nwords; w += nthreads) {
        const uint64_t o = w << 4;
        const uint32_t lo = run_of_byte(P.srecs, P.n_streams, o);
        const Mp4StreamRec sr = P.srecs[lo];
        const uint64_t rel = o - sr.base;
        if (rel >= sr.bytes) continue;
        const Mp4Range rg = P.ranges[lo];
        uint32_t fl = sr.fbase, fh = sr.fbase + sr.nfrags;  // frags[fl].offset <= o < frags[fh].offset
        while (fh - fl > 1) {
            const uint32_t mid = (fl + fh) >> 1;
            if (P.frags[mid].offset <= o) fl = mid; else fh = mid;
        }
        Mp4Cur c;
        m_load_frag(P, c, sr, rg, fl);
        uint32_t x = (uint32_t)(rel - c.foff);              // of the word in the fragment
        if (x >= c.hdr && x + 16 <= c.fbytes) {
            m_find_sample(P, c, rel);
            const uint64_t t = rel - c.s_off;
            if (t + 16 <= c.s_bytes) {
                const uint64_t sp = c.s_src + t;
                if (scode_clear16(P.sc, sp)) {
                    *reinterpret_cast<u32x4*>(P.out + o) = load16_funnel(P.sc.es + sp);
                    continue;
                }
            }
        }
        // generated bytes, NAL lengths and edges: byte by byte
        const uint32_t nv = sr.bytes - rel >= 16 ? 16u : (uint32_t)(sr.bytes - rel);
        uint32_t d0 = 0, d1 = 0, d2 = 0, d3 = 0;
        uint32_t f = fl;
#pragma unroll 1
        for (uint32_t i = 0; i < nv; i++) {
            if (x >= c.fbytes) {                            // into the stream's next fragment
                f++;
                m_load_frag(P, c, sr, rg, f);
                x = 0;
            }
            uint32_t v;
            if (x < c.hdr) {
                v = (m_hdr_word(P, c, x >> 2) >> (8 * (3 - (x & 3u)))) & 0xFFu;
            } else {
                const uint64_t r2 = c.foff + x;
                if (c.k == kMp4None) m_find_sample(P, c, r2);
                else if (r2 >= c.s_off + c.s_bytes) m_load_sample(P, c, c.k + 1);
                v = scode_sample_byte(P.sc, c.s_src, c.s_bytes, (uint32_t)(r2 - c.s_off));
            }
            v <<= 8 * (i & 3u);
            const uint32_t dw = i >> 2;
            if (dw == 0) d0 |= v; else if (dw == 1) d1 |= v; else if (dw == 2) d2 |= v; else d3 |= v;
            x++;
        }
        if (nv == 16) {
            *reinterpret_cast<u32x4*>(P.out + o) = u32x4{d0, d1, d2, d3};
        } else {
            uint32_t* q = reinterpret_cast<uint32_t*>(P.out + o);
            if (nv >= 4) q[0] = d0;
            if (nv >= 8) q[1] = d1;
            if (nv >= 12) q[2] = d2;
            const uint32_t full = nv & ~3u;
            const uint32_t last = full == 0 ? d0 : full == 4 ? d1 : full == 8 ? d2 : d3;
            for (uint32_t i = full; i < nv; i++) P.out[o + i] = (uint8_t)(last >> (8 * (i - full)));
        }
    }
}

hipError_t launch_mp4_mux(const Mp4Params& p, uint32_t flat_blocks, hipStream_t st) {
    if (p.sc.nchunks) {
        const uint32_t mb = (uint32_t)((p.sc.nchunks + 3) / 4 < flat_blocks ? (p.sc.nchunks + 3) / 4 : flat_blocks);
        EDGPU_LAUNCH(k_mp4_mark, dim3(mb), dim3(256), 0, st, p);
        EDGPU_LAUNCH(k_mp4_resolve, dim3(mb), dim3(256), 0, st, p);
    }
    EDGPU_LAUNCH(k_mp4_plan, dim3(p.n_streams), dim3(64), 0, st, p);
    EDGPU_LAUNCH(k_mp4_place, dim3(1), dim3(kMp4PlaceThreads), 0, st, p);
    EDGPU_LAUNCH(k_mp4_rows, dim3(flat_blocks), dim3(256), 0, st, p);
    EDGPU_LAUNCH(k_mp4_pack, dim3(flat_blocks), dim3(256), 0, st, p);
    return hipGetLastError();
}

}  // namespace edgpu
