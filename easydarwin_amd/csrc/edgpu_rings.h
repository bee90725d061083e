// edgpu_rings.h -- one sender's two rings as the kernels that walk them read them (device code): what
// is still intact, a packet's PktMeta, the words and bytes of its slot.  Every index is masked.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "edgpu_device.h"
#include "edgpu_bytes.h"

namespace edgpu {

struct Rings {
    const u32x4* meta;          // PktMeta as two 16-B words
    const u32x4* ring;
    uint32_t pk_mask, word_mask;
};

// The oldest index >= `from` still intact in both rings: the meta ring holds the last pk_mask + 1
// entries, the byte ring the last (word_mask + 1) * 16 bytes written (to vclob: k_ingest's
// speculative copy may reach past vbyte_end); a replica holds nothing older than its floor.
// `R` is `D`'s rings and `head` its head (or an earlier value of it); `head` when nothing is left.
__device__ __forceinline__ uint64_t intact_from(const SenderDev& D, const Rings& R, uint64_t from, uint64_t head) {
    const PktMeta* meta = reinterpret_cast<const PktMeta*>(R.meta);
    const uint64_t pk_cap = (uint64_t)R.pk_mask + 1, byte_cap = ((uint64_t)R.word_mask + 1) * 16;
    const uint64_t vend = max(D.vbyte_end, D.vclob);
    uint64_t lo = max(from, (uint64_t)D.floor);
    if (lo >= head) return head;
    if (head - lo > pk_cap) lo = head - pk_cap;
    if (vend - meta[lo & R.pk_mask].vbyte <= byte_cap) return lo;      // nothing lost: the usual case
    uint64_t hi = head;
    lo++;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (vend - meta[mid & R.pk_mask].vbyte <= byte_cap) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// Lane's PktMeta of queue index i (zero, i.e. an empty packet, when i is past the head)
__device__ __forceinline__ void load_meta(const Rings& R, uint64_t i, uint64_t head, u32x4& m0, u32x4& m1) {
    m0 = m1 = u32x4{0u, 0u, 0u, 0u};
    if (i < head) {
        const u32x4* p = R.meta + 2 * (size_t)(i & R.pk_mask);
        m0 = p[0];
        m1 = p[1];
    }
}
__device__ __forceinline__ uint32_t meta_len(const u32x4& m1) { return m1.z & 0xFFFFu; }
// Word `k` of the packet's slot, when the packet has at least `need` bytes (else zero)
__device__ __forceinline__ u32x4 load_word(const Rings& R, const u32x4& m0, const u32x4& m1, uint32_t need, uint32_t k) {
    u32x4 w = u32x4{0u, 0u, 0u, 0u};
    if (meta_len(m1) >= need) {
        const uint64_t vbyte = (uint64_t)m0.x | ((uint64_t)m0.y << 32);
        w = R.ring[(size_t)(((vbyte >> 4) + k) & R.word_mask)];
    }
    return w;
}

// Byte `off` of the packet whose slot starts at virtual byte `vbyte` (the packet starts at slot byte 4)
__device__ __forceinline__ uint32_t pkt_byte(const Rings& R, uint64_t vbyte, uint32_t off) {
    const uint64_t mask = ((uint64_t)R.word_mask << 4) | 15u;
    return reinterpret_cast<const uint8_t*>(R.ring)[(vbyte + 4 + off) & mask];
}
// Virtual byte `v` of a byte ring
__device__ __forceinline__ uint32_t ring_byte(const u32x4* ring, uint32_t word_mask, uint64_t v) {
    const uint64_t mask = ((uint64_t)word_mask << 4) | 15u;
    return reinterpret_cast<const uint8_t*>(ring)[v & mask];
}

}  // namespace edgpu
