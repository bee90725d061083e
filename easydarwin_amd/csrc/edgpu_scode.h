// edgpu_scode.h -- the start codes of an Annex-B elementary stream, shared by the muxers that turn
// them into NAL lengths (edgpu_mp4.hip, edgpu_flv.hip; device code): the bitmap of every 00 00 00 01
// and the table of the distance from each to the next, the reads both muxers make of them, and (at
// the end) the pieces their pack and placement kernels have in common.
//
//   scode_mark     flat over the ES, a lane per 32 bytes (two aligned 16-B loads and the dword after
//                  them): one word of the bitmap -- bit b of word w says 00 00 00 01 begins at ES byte
//                  32 w + b.  A wave is a chunk of 2 KiB; it also leaves the chunk's first start code.
//                  The bitmap knows nothing of units: a start code that straddles a unit's end is told
//                  apart where it is used.
//   scode_resolve  flat over the bitmap, a wave per chunk: for every start code the distance from
//                  its end to the next one, into a table indexed by position / 4 (start codes are at
//                  least 4 bytes apart).  The next one is in the lane's own word, in a later word of
//                  the wave (one ballot), or -- for the chunk's last start code only -- in a later
//                  chunk: the wave reads the chunks' first start codes 64 at a time, 128 KiB of ES
//                  per step, so the search for a NAL of L bytes is L / 128 Ki + 1 steps and the
//                  searches of a whole ES together read each chunk entry about once.
//
// Both are bodies of kernels of 256 threads (four waves), every lane active.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "edgpu_params.h"
#include "edgpu_bytes.h"
#include "edgpu_wave.h"

namespace edgpu {

// Bits [lo, lo + 32) of the bitmap
__device__ __forceinline__ uint32_t scode_bits(const ScodeView& V, uint64_t lo) {
    const uint64_t w = lo >> 5;
    const uint32_t sh = (uint32_t)(lo & 31u);
    const uint32_t a = w < V.nwords ? V.bitmap[w] : 0u;
    const uint32_t b = (sh && w + 1 < V.nwords) ? V.bitmap[w + 1] : 0u;
    return (uint32_t)(((((uint64_t)b) << 32) | a) >> sh);
}

__device__ __forceinline__ void scode_mark(const ScodeView& V) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * 4;
    for (uint64_t c = wave; c < V.nchunks; c += nwaves) {
        const uint64_t w = c * kScodeChunkWords + lane;
        const uint64_t pos = w << 5;
        uint32_t bits = 0;
        if (pos < V.es_bytes) {
            const uint64_t left = V.es_bytes - pos;         // bytes at or past the ES end read as 0: they complete no start code
            const u32x4* src = reinterpret_cast<const u32x4*>(V.es + pos);
            u32x4 v0 = src[0];
            u32x4 v1 = left > 16 ? src[1] : u32x4{0u, 0u, 0u, 0u};
            uint32_t nx = left > 32 ? *reinterpret_cast<const uint32_t*>(V.es + pos + 32) : 0u;
            if (left < 16) v0 = keep16(v0, (int)left);
            else if (left < 32) v1 = keep16(v1, (int)left - 16);
            else if (left < 36) nx &= (1u << (8 * ((uint32_t)left - 32))) - 1u;
            const uint32_t d[9] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, nx};
#pragma unroll
            for (uint32_t j = 0; j < 8; j++) {
                const uint32_t lo = d[j], hi = d[j + 1];
                if (lo == 0x01000000u) bits |= 1u << (4 * j);
                if (__builtin_amdgcn_alignbyte(hi, lo, 1) == 0x01000000u) bits |= 2u << (4 * j);
                if (__builtin_amdgcn_alignbyte(hi, lo, 2) == 0x01000000u) bits |= 4u << (4 * j);
                if (__builtin_amdgcn_alignbyte(hi, lo, 3) == 0x01000000u) bits |= 8u << (4 * j);
            }
        }
        if (w < V.nwords) V.bitmap[w] = bits;
        const uint64_t ball = __ballot(bits != 0);
        if (ball == 0) {
            if (lane == 0) V.chunk_first[c] = kScodeNone;
        } else if (lane == (uint32_t)__builtin_ctzll(ball)) {
            V.chunk_first[c] = lane * 32u + (uint32_t)__builtin_ctz(bits);
        }
    }
}

__device__ __forceinline__ void scode_resolve(const ScodeView& V) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * 4;
    for (uint64_t c = wave; c < V.nchunks; c += nwaves) {
        const uint64_t w = c * kScodeChunkWords + lane;
        const uint32_t bits = w < V.nwords ? V.bitmap[w] : 0u;
        const uint64_t ball = __ballot(bits != 0);
        if (ball == 0) continue;                            // wave-uniform
        // the next word of this wave that holds a start code
        const uint64_t above = lane == 63 ? 0ull : ball & ~((2ull << lane) - 1ull);
        const uint32_t nl = above ? (uint32_t)__builtin_ctzll(above) : 0u;
        const uint32_t fb = bits ? (uint32_t)__builtin_ctz(bits) : 0u;
        const uint32_t nfb = (uint32_t)__shfl((int)fb, (int)nl, 64);
        // the chunk's last start code looks at the later chunks, 64 per step
        uint64_t far = V.es_bytes;
        for (uint64_t cc = c + 1; cc < V.nchunks; cc += 64) {
            const uint32_t v = cc + lane < V.nchunks ? V.chunk_first[cc + lane] : kScodeNone;
            const uint64_t b2 = __ballot(v != kScodeNone);
            if (b2) {
                const uint32_t l2 = (uint32_t)__builtin_ctzll(b2);
                far = (cc + l2) * kScodeChunkBytes + lane_of(v, l2);
                break;
            }
        }
        const uint64_t after = above ? (c * kScodeChunkWords + nl) * 32ull + nfb : far;
        uint32_t rem = bits;
        while (rem) {
            const uint32_t i = (uint32_t)__builtin_ctz(rem);
            rem &= rem - 1;
            const uint64_t q = (w << 5) + i;
            const uint64_t nxt = rem ? (w << 5) + (uint32_t)__builtin_ctz(rem) : after;
            const uint64_t dist = nxt - (q + 4);
            V.lens[q >> 2] = dist > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)dist;
        }
    }
}

// Whether no start code touches the 16 bytes at ES byte `sp`: one that begins in [sp - 3, sp + 15] would
__device__ __forceinline__ bool scode_clear16(const ScodeView& V, uint64_t sp) {
    const uint64_t b0 = sp >= 3 ? sp - 3 : 0;
    const uint32_t nb = (uint32_t)(sp + 16 - b0);
    return (scode_bits(V, b0) & ((1u << nb) - 1u)) == 0;
}

// Byte `t` of the sample made of the unit [src, src + bytes) of the ES: a byte of a NAL length where
// a start code was, else the ES byte
__device__ __forceinline__ uint32_t scode_sample_byte(const ScodeView& V, uint64_t src, uint32_t bytes, uint32_t t) {
    const uint64_t a = src, end = src + bytes, sp = a + t;
    const uint64_t lo = sp >= 3 ? sp - 3 : 0;
    const uint32_t v = scode_bits(V, lo);
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        if (sp < lo + j) continue;
        const uint64_t q = sp - j;
        if (q < a || q + 4 > end || !((v >> (uint32_t)(q - lo)) & 1u)) continue;
        const uint64_t q2 = q + 4 + V.lens[q >> 2];
        const uint64_t nal_end = q2 + 4 <= end ? q2 : end;  // a start code cut by the unit's end is data
        const uint32_t len = (uint32_t)(nal_end - (q + 4));
        return (len >> (8 * (3 - j))) & 0xFFu;
    }
    return V.es[sp];
}

// ---- What k_mp4_pack / k_flv_pack and k_mp4_place / k_flv_place share.  SRec is the mux's stream
// record: `bytes` and `base` of the stream's run in the output; runs begin 16-B aligned. ----

// The run that holds output byte `o`: srecs[lo].base <= o < srecs[lo + 1].base
template <typename SRec>
__device__ __forceinline__ uint32_t run_of_byte(const SRec* srecs, uint32_t n_streams, uint64_t o) {
    uint32_t lo = 0, hi = n_streams;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (srecs[mid].base <= o) lo = mid; else hi = mid;
    }
    return lo;
}

// The 16 bytes at `src`, of any alignment: two aligned 16-B loads, funnelled.  The pack's fast path
// for a word inside one sample that scode_clear16 passes: one aligned 16-B store of this.
__device__ __forceinline__ u32x4 load16_funnel(const uint8_t* src) {
    const uintptr_t a = (uintptr_t)src;
    const uint32_t sh = (uint32_t)(a & 15u);
    const u32x4* sw = reinterpret_cast<const u32x4*>(a & ~(uintptr_t)15);
    const u32x4 l = sw[0];
    const u32x4 h = sh ? sw[1] : l;
    return funnel16(l, h, sh);
}

// One round of the placement scan (every thread of the workgroup, stream `i` each): the aligned
// bytes of the round's runs before stream i's; `round_total`: of all the round's runs
template <typename SRec>
__device__ __forceinline__ uint64_t place_round(const SRec* srecs, uint32_t n_streams, uint32_t i, uint64_t* scratch, uint64_t& round_total) {
    const uint64_t bytes = i < n_streams ? srecs[i].bytes : 0ull;
    return block_exclusive_scan<uint64_t>((bytes + 15) & ~15ull, scratch, round_total);
}

// The output's bytes from the rounds' sum `cb`.  The last run is not padded: its base + bytes is the
// sum of every run less the last one's padding
template <typename SRec>
__device__ __forceinline__ uint64_t place_total(const SRec* srecs, uint32_t n_streams, uint64_t cb) {
    const uint64_t last = n_streams ? srecs[n_streams - 1].bytes : 0ull;
    return cb - (((last + 15) & ~15ull) - last);
}

}  // namespace edgpu
