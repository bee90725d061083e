// edgpu_wave.h -- wave64 and workgroup primitives shared by every kernel file (device code):
// uniform and lane reads, wave scans and sums, workgroup scans and reductions.  A new kernel takes
// these from here, not from a copy of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace edgpu {

// The value of the first active lane, as a scalar.  `v` must already be the same in every active lane.
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t uni(uint64_t v) { return ((uint64_t)uni((uint32_t)(v >> 32)) << 32) | uni((uint32_t)v); }

// Lane `l`'s value, as a scalar.  `l` (0..63) is wave-uniform; the lane need not be active.
__device__ __forceinline__ uint32_t lane_of(uint32_t v, uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l); }
__device__ __forceinline__ uint64_t lane_of(uint64_t v, uint32_t l) {
    return ((uint64_t)lane_of((uint32_t)(v >> 32), l) << 32) | lane_of((uint32_t)v, l);
}

// Lane `l`'s value, `l` (0..63) chosen per lane; an inactive source lane gives 0.
__device__ __forceinline__ uint64_t shfl64(uint64_t v, uint32_t l) {
    return ((uint64_t)(uint32_t)__shfl((int)(v >> 32), (int)l, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)v, (int)l, 64);
}

// Inclusive scans across the wave (sum, maximum); `lane` is the caller's lane, 0..63.  Every lane active.
__device__ __forceinline__ uint32_t wave_incl(uint32_t v, uint32_t lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(v, o, 64);
        if (lane >= (uint32_t)o) v += u;
    }
    return v;
}
__device__ __forceinline__ uint64_t wave_incl(uint64_t v, uint32_t lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t lo = __shfl_up((uint32_t)v, o, 64), hi = __shfl_up((uint32_t)(v >> 32), o, 64);
        if (lane >= (uint32_t)o) v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_incl_max(uint32_t v, uint32_t lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(v, o, 64);
        if (lane >= (uint32_t)o) v = v > u ? v : u;
    }
    return v;
}

// The wave's sum, in every lane.  Every lane active.
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Inclusive scan of a 64-bit value across the wave, in registers: DPP row shifts (1, 2, 4, 8)
// give each row of 16 lanes its own prefix, then every lane adds the totals of the rows before its
// own (lanes 15, 31, 47, read as scalars).  Call with every lane active.
template <int CTRL>
__device__ __forceinline__ uint64_t dpp_u64(uint64_t x) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)x, CTRL, 0xF, 0xF, true);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(x >> 32), CTRL, 0xF, 0xF, true);
    return (uint64_t)hi << 32 | lo;
}
__device__ __forceinline__ uint64_t wave_inclusive_scan_u64(uint64_t x) {
    x += dpp_u64<0x111>(x);                 // row_shr:1 (a row's first lanes read 0)
    x += dpp_u64<0x112>(x);                 // row_shr:2
    x += dpp_u64<0x114>(x);                 // row_shr:4
    x += dpp_u64<0x118>(x);                 // row_shr:8
    const uint64_t r0 = lane_of(x, 15), r1 = lane_of(x, 31), r2 = lane_of(x, 47);
    const int row = (threadIdx.x & 63) >> 4;
    return x + (row >= 1 ? r0 : 0ull) + (row >= 2 ? r1 : 0ull) + (row >= 3 ? r2 : 0ull);
}

// Exclusive scan over a workgroup of NW waves of 64 (256 threads by default); `total` gets the sum of
// all.  Every thread of the block calls it; `scratch` (LDS) holds NW entries and may be reused right after.
template <typename T, int NW = 4>
__device__ __forceinline__ T block_exclusive_scan(T v, T* scratch, T& total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const T x = wave_incl(v, (uint32_t)lane);
    if (lane == 63) scratch[wid] = x;
    __syncthreads();
    T base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) {
        T t = scratch[w];
        if (w < wid) base += t;
        tot += t;
    }
    __syncthreads();
    total = tot;
    return base + x - v;
}

// Inclusive scan over a workgroup of up to 1024 threads: shuffles inside each wave, then the
// wave totals (wsum, one per wave) through LDS.  Every thread of the block must call it.
template <typename T>
__device__ __forceinline__ T wave_block_inclusive_scan(T v, T* wsum) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    v = wave_incl(v, (uint32_t)lane);
    if (lane == 63) wsum[w] = v;
    __syncthreads();
    T base = 0;
    for (int i = 0; i < w; i++) base += wsum[i];
    __syncthreads();                                  // wsum may be reused by the next call
    return v + base;
}

// Reduction over a workgroup of NW waves of 64 (every thread gets the result).  Every thread of the
// block calls it; `scratch` holds NW entries and may be reused right after.
struct OpSum { template <typename T> __device__ T operator()(T a, T b) const { return a + b; } };
struct OpMax { template <typename T> __device__ T operator()(T a, T b) const { return a > b ? a : b; } };
struct OpMin { template <typename T> __device__ T operator()(T a, T b) const { return a < b ? a : b; } };
template <typename T, typename Op, int NW = 4>
__device__ __forceinline__ T block_reduce(T v, T* scratch) {
    const Op op;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, (T)__shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    T r = scratch[0];
#pragma unroll
    for (int w = 1; w < NW; w++) r = op(r, scratch[w]);
    __syncthreads();
    return r;
}

}  // namespace edgpu
