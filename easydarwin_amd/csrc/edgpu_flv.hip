// edgpu_flv.hip -- the FLV mux of tapped H.264 access units (gfx950).  The rules are stated in
// include/edgpu.h (edgpu_flv_mux) and restated on the CPU in tests/flv_model.py.  One call is five
// kernels:
//
//   k_flv_mark     the bitmap of the ES's start codes and each 2-KiB chunk's first one
//   k_flv_resolve  for every start code the distance from its end to the next one (both are
//                  edgpu_scode.h, shared with the fragmented-MP4 mux)
//   k_flv_plan     one wave64 per stream row, its units in rounds of 64: the extended timestamp as
//                  the fragmented-MP4 plan extends it, the millisecond stamp, the tag sizes and
//                  their prefix sums, and the new state row, with the carries in wave-uniform
//                  registers.  The lane of a PARAMS unit walks at most 8 hops of the distance table
//                  for the first SPS and the first PPS.
//   k_flv_place    one workgroup sums the streams' bytes (runs are 16-B aligned) in blocks of 256
//                  and alone decides whether the call commits.
//   k_flv_pack     flat over the output's 16-B words.  A word that lies inside one sample and touches
//                  no start code is one 16-B store funnelled from two aligned 16-B loads; any other
//                  word (tag header and trailer, NAL lengths, unit and run edges) is assembled byte
//                  by byte.  Every byte of a run is written once, nothing outside the runs.  Then
//                  flat over the units: the tag rows.
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

constexpr uint32_t kFlvPlaceThreads = 256;
constexpr uint32_t kFlvHead = 16;           // tag header (11) and the AVC video header (5)
constexpr uint32_t kFlvOver = 20;           // ... and PreviousTagSize
constexpr uint32_t kFlvParamNals = 8;       // NALs of a PARAMS unit examined for its parameter sets

// The first start code at or after ES byte `pos` that lies wholly below `end`, or `end`
__device__ __forceinline__ uint64_t f_first_code(const ScodeView& V, uint64_t pos, uint64_t end) {
    if (pos + 4 > end) return end;
    uint64_t w = pos >> 5;
    uint64_t q = end;
    const uint32_t b0 = V.bitmap[w] & (0xFFFFFFFFu << (uint32_t)(pos & 31u));
    if (b0) {
        q = (w << 5) + (uint32_t)__builtin_ctz(b0);
    } else {
        const uint64_t c = w / kScodeChunkWords;
        const uint64_t cend = (c + 1) * kScodeChunkWords < V.nwords ? (c + 1) * kScodeChunkWords : V.nwords;
        for (w++; w < cend && (w << 5) < end; w++) {        // the rest of this chunk, word by word
            const uint32_t b = V.bitmap[w];
            if (b) { q = (w << 5) + (uint32_t)__builtin_ctz(b); break; }
        }
        if (q == end)
            for (uint64_t cc = c + 1; cc < V.nchunks && cc * kScodeChunkBytes < end; cc++) {
                const uint32_t v = V.chunk_first[cc];
                if (v != kScodeNone) { q = cc * kScodeChunkBytes + v; break; }
            }
    }
    return q + 4 <= end ? q : end;
}

}  // namespace

__global__ __launch_bounds__(256) void k_flv_mark(FlvParams P) { scode_mark(P.sc); }

__global__ __launch_bounds__(256) void k_flv_resolve(FlvParams P) { scode_resolve(P.sc); }

__global__ __launch_bounds__(64) void k_flv_plan(FlvParams P) {
    const uint32_t s = blockIdx.x;
    if (s >= P.n_streams) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t first = uni(P.ranges[s].first), count = uni(P.ranges[s].count);
    const edgpu_flv_state st = P.states[s];
    const uint32_t started = uni(st.started);
    uint64_t c_ext = uni(started ? st.ext_ts : (uint64_t)0);
    uint64_t origin = uni(st.origin);
    if (!started && count) origin = uni(P.units[first].rtp_ts);
    uint32_t c_bytes = 0;
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
        const bool lead = hasb && bytes >= 4 && ((P.sc.bitmap[off >> 5] >> (off & 31u)) & 1u);
        if (hasb && !lead) flags |= EDGPU_TAP_DAMAGED;
        // the extended timestamp, as the fragmented-MP4 mux extends it
        uint32_t prev_ts = __shfl_up(ts, 1, 64);
        if (lane == 0) prev_ts = (uint32_t)c_ext;
        uint64_t d = valid ? (uint64_t)(int64_t)(int32_t)(ts - prev_ts) : 0ull;
        if (valid && i == 0 && !started) d = ts;
        const uint64_t in_d = wave_incl(d, lane);
        const uint64_t ext = c_ext + in_d;
        const uint64_t t90 = ext - origin + P.time_offset;
        const uint32_t size = hasb ? bytes + kFlvOver : 0u;
        const uint32_t in_b = wave_incl(size, lane);
        if (valid) {
            FlvRec r;
            r.pre = c_bytes + in_b - size;
            r.ts_ms = (uint32_t)(t90 / 90u);
            r.flags = flags | ((hasb ? 2u : 1u) << 30);
            r.stream = s;
            r.sps_offset = 0; r.sps_bytes = 0; r.pps_offset = 0; r.pps_bytes = 0;
            if (hasb && (flags & EDGPU_TAP_PARAMS)) {
                const uint64_t end = off + bytes;
                uint64_t q = lead ? off : f_first_code(P.sc, off, end);
                for (uint32_t hop = 0; hop < kFlvParamNals && q < end; hop++) {
                    const uint64_t q2 = q + 4 + P.sc.lens[q >> 2];
                    const uint64_t nal_end = q2 + 4 <= end ? q2 : end;      // a start code cut by the unit's end is data
                    const uint32_t len = (uint32_t)(nal_end - (q + 4));
                    if (len) {
                        const uint32_t type = P.sc.es[q + 4] & 0x1Fu;
                        const uint32_t at = kFlvHead + (uint32_t)(q + 4 - off);
                        if (type == 7 && !r.sps_bytes) { r.sps_offset = at; r.sps_bytes = len; }
                        if (type == 8 && !r.pps_bytes) { r.pps_offset = at; r.pps_bytes = len; }
                    }
                    q = nal_end;
                }
            }
            P.recs[first + i] = r;
        }
        c_ext += lane_of(in_d, 63);
        c_bytes += lane_of(in_b, 63);
    }
    if (lane == 0) {
        edgpu_flv_state n = st;
        if (count) {
            n.ext_ts = c_ext;
            n.origin = origin;
            n.started = 1;
        }
        P.new_states[s] = n;
        FlvStreamRec sr;
        sr.bytes = c_bytes;
        sr.base = 0;
        P.srecs[s] = sr;
    }
}

__global__ __launch_bounds__(256) void k_flv_place(FlvParams P) {
    __shared__ uint64_t scratch[kFlvPlaceThreads / 64];
    const uint32_t t = threadIdx.x;
    uint64_t cb = 0;
    for (uint32_t b = 0; b < P.n_streams; b += kFlvPlaceThreads) {
        const uint32_t i = b + t;
        uint64_t tb;
        const uint64_t base = cb + place_round(P.srecs, P.n_streams, i, scratch, tb);
        if (i < P.n_streams) P.srecs[i].base = base;
        cb += tb;
    }
    if (t == 0) {
        const uint64_t total = place_total(P.srecs, P.n_streams, cb);
        FlvPlace pl;
        pl.bytes = total;
        pl.commit = total <= P.out_cap ? 1u : 0u;
        pl._pad = 0;
        *P.place = pl;
    }
}

namespace {

// The tag k_flv_pack's current byte is in
struct FlvCur {
    uint32_t unit;          // its unit
    uint32_t pre;           // of the tag, relative to the stream's run
    uint32_t bytes;         // of the unit: the tag has bytes + 20
    uint32_t ts_ms, key;
    uint64_t src;           // of the unit in the ES
};

__device__ __forceinline__ void f_load(const FlvParams& P, FlvCur& c, uint32_t unit) {
    const FlvRec r = P.recs[unit];
    const edgpu_tap_unit u = P.units[unit];
    c.unit = unit;
    c.pre = r.pre;
    c.bytes = u.bytes;
    c.ts_ms = r.ts_ms;
    c.key = r.flags & EDGPU_TAP_KEY;
    c.src = u.offset;
}

// Byte `x` of the current tag
__device__ __forceinline__ uint32_t f_tag_byte(const FlvParams& P, const FlvCur& c, uint32_t x) {
    if (x >= kFlvHead) {
        if (x < kFlvHead + c.bytes) return scode_sample_byte(P.sc, c.src, c.bytes, x - kFlvHead);
        return ((c.bytes + kFlvHead) >> (8 * (3 - (x - kFlvHead - c.bytes)))) & 0xFFu;     // PreviousTagSize
    }
    switch (x) {
        case 0: return 0x09u;
        case 1: case 2: case 3: return ((c.bytes + 5u) >> (8 * (3 - x))) & 0xFFu;          // DataSize
        case 4: case 5: case 6: return (c.ts_ms >> (8 * (6 - x))) & 0xFFu;
        case 7: return c.ts_ms >> 24;
        case 11: return c.key ? 0x17u : 0x27u;
        case 12: return 0x01u;
        default: return 0u;                                 // stream id, composition time
    }
}

}  // namespace

__global__ __launch_bounds__(256) void k_flv_pack(FlvParams P) {
    const FlvPlace pl = *P.place;
    if (!pl.commit) return;
    const uint64_t nwords = (pl.bytes + 15) >> 4;
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t w = gid; w < nwords; w += nthreads) {
        const uint64_t o = w << 4;
        const uint32_t lo = run_of_byte(P.srecs, P.n_streams, o);
        const FlvStreamRec sr = P.srecs[lo];
        const uint64_t rel64 = o - sr.base;
        if (rel64 >= sr.bytes) continue;
        const uint32_t rel = (uint32_t)rel64;               // a run is below 2^32 bytes
        const FlvRange rg = P.ranges[lo];
        uint32_t ul = rg.first, uh = rg.first + rg.count;   // recs[ul].pre <= rel < recs[uh].pre: a unit with bytes
        while (uh - ul > 1) {
            const uint32_t mid = (ul + uh) >> 1;
            if (P.recs[mid].pre <= rel) ul = mid; else uh = mid;
        }
        FlvCur c;
        f_load(P, c, ul);
        uint32_t x = rel - c.pre;                           // of the word in the tag
        if (x >= kFlvHead && x + 16 <= kFlvHead + c.bytes) {
            const uint64_t sp = c.src + (x - kFlvHead);
            if (scode_clear16(P.sc, sp)) {
                *reinterpret_cast<u32x4*>(P.out + o) = load16_funnel(P.sc.es + sp);
                continue;
            }
        }
        // generated bytes, NAL lengths and edges: byte by byte
        const uint32_t nv = sr.bytes - rel >= 16 ? 16u : (uint32_t)(sr.bytes - rel);
        const uint32_t uend = rg.first + rg.count;
        uint32_t d0 = 0, d1 = 0, d2 = 0, d3 = 0;
#pragma unroll 1
        for (uint32_t i = 0; i < nv; i++) {
            if (x >= c.bytes + kFlvOver) {                  // into the stream's next tag: units without bytes have none
                uint32_t n = c.unit + 1;
                while (n + 1 < uend && P.units[n].bytes == 0) n++;
                f_load(P, c, n);
                x = 0;
            }
            const uint32_t v = f_tag_byte(P, c, x) << (8 * (i & 3u));
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
    for (uint64_t i = gid; i < P.n_units; i += nthreads) {
        const FlvRec r = P.recs[i];
        const uint32_t kind = r.flags >> 30;
        edgpu_flv_tag t;
        t.offset = 0; t.bytes = 0; t.timestamp_ms = 0; t.flags = 0; t.stream = 0;
        t.sps_offset = 0; t.sps_bytes = 0; t.pps_offset = 0; t.pps_bytes = 0;
        if (kind) {
            t.offset = P.srecs[r.stream].base + r.pre;
            t.bytes = kind == 2 ? P.units[i].bytes + kFlvOver : 0u;
            t.timestamp_ms = r.ts_ms;
            t.flags = r.flags & 0x3FFFFFFFu;
            t.stream = r.stream;
            t.sps_offset = r.sps_offset; t.sps_bytes = r.sps_bytes;
            t.pps_offset = r.pps_offset; t.pps_bytes = r.pps_bytes;
        }
        P.rows[i] = t;
    }
}

hipError_t launch_flv_mux(const FlvParams& p, uint32_t flat_blocks, hipStream_t st) {
    if (p.sc.nchunks) {
        const uint32_t mb = (uint32_t)((p.sc.nchunks + 3) / 4 < flat_blocks ? (p.sc.nchunks + 3) / 4 : flat_blocks);
        EDGPU_LAUNCH(k_flv_mark, dim3(mb), dim3(256), 0, st, p);
        EDGPU_LAUNCH(k_flv_resolve, dim3(mb), dim3(256), 0, st, p);
    }
    EDGPU_LAUNCH(k_flv_plan, dim3(p.n_streams), dim3(64), 0, st, p);
    EDGPU_LAUNCH(k_flv_place, dim3(1), dim3(kFlvPlaceThreads), 0, st, p);
    EDGPU_LAUNCH(k_flv_pack, dim3(flat_blocks), dim3(256), 0, st, p);
    return hipGetLastError();
}

}  // namespace edgpu
