// edgpu_tap.hip -- the H.264 elementary-stream tap: RTP sender rings -> Annex-B access units on the
// GPU (gfx950).  RFC 6184 non-interleaved mode; the rules are stated in include/edgpu.h and
// restated on the CPU in tests/tap_model.py.  One drain of every enabled tap is three kernels:
//
//   k_tap_scan   one wave64 per enabled tap.  The wave walks the track's RTP sender over the queue
//                indices [intact_from(TapDev.head), SenderDev.head) in rounds of kTapRound entries.
//                A lane loads one PktMeta and the slot's first two 16-B words (RTP bytes 0..27 decide
//                every common case; CC, X, P and STAP-A read further bytes on a slower path) and
//                classifies its packet.  Across the wave: the previous good packet of every lane
//                (ballot + clz), gaps, access-unit starts, the FU-A chain as a segmented scan whose
//                carry crosses rounds, and prefix sums for the byte offsets and the counters.  Only
//                the access-unit bookkeeping is serial, one step per unit start of the round, in
//                wave-uniform registers.  Every entry gets a TapRec (what to copy where), every unit
//                an edgpu_tap_unit with stream-relative offsets.  The drain's outcome -- the end of
//                the last complete unit, the counters up to it, the state to carry -- goes to the
//                tap's d_* fields; nothing carried is changed.
//   k_tap_place  one workgroup scans the taps in blocks of 256: 16-B aligned stream offsets, unit
//                bases, k_tap_copy's work items, and the three capacities.  It alone decides whether
//                the drain commits; if so it moves every tap's carried state on and writes the
//                stream rows.
//   k_tap_copy   work items are (tap, round of 64 records) and (tap, round of 64 units), found by
//                binary search in the items' prefix sums, so one fast stream spreads over many
//                waves.  A 16-lane group copies one packet's bytes: the body in whole 16-B
//                destination words, each assembled from two aligned source words (funnel16);
//                byte stores only for the start code / rebuilt header and the packet's own
//                unaligned head and tail.  Ring indices are masked per word and per byte.
//
// A tap's row has one writer at a time, so there are no atomics.
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

constexpr uint32_t kNoChain = 0xFFu;
constexpr uint32_t kPlaceThreads = 256;

__device__ __forceinline__ uint32_t bit_of(unsigned long long m, uint32_t l) { return (uint32_t)((m >> l) & 1ull); }
__device__ __forceinline__ uint32_t top_bit(unsigned long long m) { return 63u - (uint32_t)__clzll((long long)m); }

// Totals of a drain so far: entries, and what the good packets among them did
struct Tally {
    uint32_t packets, skipped, malformed, orphans, unsupported;
};

}  // namespace

__global__ __launch_bounds__(64) void k_tap_scan(TapParams P) {
    if (blockIdx.x >= P.ntaps) return;
    TapDev& T = P.taps[P.list[blockIdx.x]];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t snd = uni(T.sender);
    const bool flush = (P.flags & EDGPU_TAP_FLUSH) != 0;
    uint64_t from = uni(T.head);
    if (!uni(T.enabled) || snd >= P.nsenders) {
        if (lane == 0) {
            T.d_start = T.d_cut = from; T.d_bytes = 0; T.d_nrec = T.d_nunits = 0;
            T.d_has_prev = T.has_prev; T.d_prev_seq = T.prev_seq; T.d_pending = T.pending; T.d_damaged = 0;
            T.d_packets = T.d_skipped = T.d_malformed = T.d_orphans = T.d_unsupported = 0;
        }
        return;
    }
    const SenderDev& D = P.senders[snd];
    const uint64_t head = uni(D.head);
    const Rings R{reinterpret_cast<const u32x4*>(D.meta), reinterpret_cast<const u32x4*>(D.ring), uni(D.pk_mask), uni(D.word_mask)};
    uint64_t start = uni(intact_from(D, R, from, head));
    const uint32_t cap = uni(T.cap);
    if (head - start > cap) start = head - cap;             // never more entries than the work buffers hold
    const uint32_t missed = (uint32_t)(start - from);
    TapRec* recs = reinterpret_cast<TapRec*>(T.rec);
    edgpu_tap_unit* units = reinterpret_cast<edgpu_tap_unit*>(T.unit);

    // carried along the walk (wave-uniform)
    uint32_t c_has_prev = missed ? 0u : uni(T.has_prev), c_prev_seq = uni(T.prev_seq), c_prev_ts = 0, c_prev_m = 0;
    uint32_t c_first = 1, c_chain = kNoChain;
    const uint32_t pending = (missed || uni(T.pending)) ? 1u : 0u;
    uint64_t c_good_end = start;                            // index past the newest good packet
    Tally tot = {0, 0, 0, 0, 0}, at_good = {0, 0, 0, 0, 0}; // every entry so far; up to the newest good packet
    uint64_t t_bytes = 0;
    uint32_t t_nals = 0, t_good = 0;
    // the open access unit
    uint32_t au_open = 0, au_ts = 0, au_seq = 0, au_flags = 0, au_nals0 = 0, au_good0 = 0, au_has_prev = 0, au_prev_seq = 0;
    uint64_t au_off = 0, au_arrival = 0, au_cut = start;
    Tally au_tally = {0, 0, 0, 0, 0};
    uint32_t n_units = 0, n_damaged = 0;

    for (uint64_t base = start; base < head; base += kTapRound) {
        const uint64_t idx = base + lane;
        u32x4 m0 = u32x4{0u, 0u, 0u, 0u}, m1 = m0, w0 = m0, w1 = m0;
        if (idx < head) {
            const u32x4* p = R.meta + 2 * (size_t)(idx & R.pk_mask);
            m0 = p[0];
            m1 = p[1];
        }
        const uint32_t len = m1.z & 0xFFFFu;
        const uint64_t vbyte = (uint64_t)m0.x | ((uint64_t)m0.y << 32);
        if (len >= 12) w0 = R.ring[(size_t)((vbyte >> 4) & R.word_mask)];
        if (len >= 13) w1 = R.ring[(size_t)(((vbyte >> 4) + 1) & R.word_mask)];

        // rule 1: parse
        const uint32_t b0 = w0.y & 0xFFu;
        bool bad = len < 12 || (b0 >> 6) != 2;
        uint32_t hdr = 12 + 4 * (b0 & 15u), end = len;
        if (!bad && (b0 & 0x10u)) {
            if (hdr + 4 > len) bad = true;
            else hdr += 4 + 4 * ((pkt_byte(R, vbyte, hdr + 2) << 8) | pkt_byte(R, vbyte, hdr + 3));
        }
        if (!bad && (b0 & 0x20u)) {
            const uint32_t pad = pkt_byte(R, vbyte, len - 1);
            if (pad == 0 || hdr + pad > len) bad = true; else end = len - pad;
        }
        if (!bad && hdr >= end) bad = true;
        const bool good = len != 0 && !bad;
        const uint32_t paylen = good ? end - hdr : 0u;
        uint32_t p0 = 0, p1 = 0;
        if (good) {
            if (hdr == 12) { p0 = w1.x & 0xFFu; p1 = paylen >= 2 ? (w1.x >> 8) & 0xFFu : 0u; }
            else { p0 = pkt_byte(R, vbyte, hdr); p1 = paylen >= 2 ? pkt_byte(R, vbyte, hdr + 1) : 0u; }
        }
        const uint32_t marker = (w0.y >> 15) & 1u;
        const uint32_t seq = __builtin_bswap32(w0.y) & 0xFFFFu;
        const uint32_t ts = __builtin_bswap32(w0.z);
        const uint32_t t = p0 & 0x1Fu, ftype = p1 & 0x1Fu;
        const bool fS = (p1 & 0x80u) != 0, fE = (p1 & 0x40u) != 0;

        // rules 2 and 3: the previous good packet of every lane
        const unsigned long long below = (1ull << lane) - 1ull;
        const unsigned long long good_m = __ballot(good);
        const unsigned long long gb = good_m & below;
        const uint32_t pl = gb ? top_bit(gb) : 0u;
        uint32_t pseq = __shfl(seq, pl, 64), pts = __shfl(ts, pl, 64), pm = __shfl(marker, pl, 64);
        if (!gb) { pseq = c_prev_seq; pts = c_prev_ts; pm = c_prev_m; }
        const bool gap = good && (gb || c_has_prev) && seq != ((pseq + 1) & 0xFFFFu);
        const bool au_start = good && ((!gb && c_first) || ts != pts || pm);

        // rule 4: the FU-A chain.  A continuation is emitted iff the newest good packet below it
        // that is not itself a plain link (N) is a start of its type, every link between being of
        // the type of the packet before it; without one in the round the carried chain decides.
        const bool fu_ok = good && t == 28 && paylen >= 2 && !(fS && fE);
        const bool opener = fu_ok && fS;
        const bool contc = fu_ok && !fS;
        const bool cont_valid = contc && !gap && !au_start;
        const uint32_t chainable = (opener || (cont_valid && !fE)) ? 1u : 0u;
        const uint32_t p_chainable = __shfl(chainable, pl, 64), p_ftype = __shfl(ftype, pl, 64);
        const bool tb = cont_valid && gb && !(p_chainable && p_ftype == ftype);     // cannot match what precedes it
        const bool link = cont_valid && !fE && !tb;
        const unsigned long long n_m = __ballot(good && !link), open_m = __ballot(opener);
        const unsigned long long nb = n_m & below;
        const bool emit_cont = cont_valid && !tb && (nb ? bit_of(open_m, top_bit(nb)) != 0 : c_chain == ftype);
        const bool open_after = opener || (link && emit_cont);

        // what the packet emits
        uint32_t kind = kTapNone, src = 0, clen = 0, hdrb = 0, nun = 0, bytes = 0, nals = 0, fl = 0;
        bool malformed = false, orphan = false, unsupported = false;
        if (good) {
            uint32_t nt = 0;
            if (t >= 1 && t <= 23) {
                kind = kTapStart; src = hdr; clen = paylen; bytes = 4 + paylen; nals = 1; nt = t;
            } else if (t == 24) {
                uint32_t o = 1;
                while (o < paylen) {
                    const uint32_t size = o + 2 <= paylen ? (pkt_byte(R, vbyte, hdr + o) << 8) | pkt_byte(R, vbyte, hdr + o + 1) : 0u;
                    if (size == 0 || o + 2 + size > paylen) { malformed = true; break; }
                    const uint32_t it = pkt_byte(R, vbyte, hdr + o + 2) & 0x1Fu;
                    if (it == 5) fl |= EDGPU_TAP_KEY;
                    if (it == 7 || it == 8) fl |= EDGPU_TAP_PARAMS;
                    nun++; bytes += 4 + size; o += 2 + size;
                }
                nals = nun;
                if (nun) { kind = kTapStap; src = hdr + 1; }
            } else if (t == 28) {
                if (!fu_ok) malformed = true;
                else if (opener) {
                    kind = kTapStartHdr; hdrb = (p0 & 0xE0u) | ftype; src = hdr + 2; clen = paylen - 2; bytes = 5 + clen; nals = 1; nt = ftype;
                } else if (emit_cont) {
                    kind = kTapRaw; src = hdr + 2; clen = paylen - 2; bytes = clen;
                } else orphan = true;
            } else unsupported = true;
            if (nt == 5) fl |= EDGPU_TAP_KEY;
            if (nt == 7 || nt == 8) fl |= EDGPU_TAP_PARAMS;
            if (gap || malformed || orphan || unsupported) fl |= EDGPU_TAP_DAMAGED;
        }

        // prefix sums: bytes; counters packed 8 bits each (a round adds at most 64 to each)
        const uint32_t in_bytes = wave_incl(bytes, lane);
        const uint32_t in_c1 = wave_incl((len ? 1u : 0u) | ((len && bad) ? 1u << 8 : 0u) | (malformed ? 1u << 16 : 0u) |
                                         (orphan ? 1u << 24 : 0u), lane);
        const uint32_t in_c2 = wave_incl((unsupported ? 1u : 0u) | (nals << 8), lane);
        if (idx < head) {
            TapRec r;
            r.dst = t_bytes + (in_bytes - bytes);
            r.src = (uint16_t)(4 + src); r.len = (uint16_t)clen; r.kind = (uint8_t)kind; r.hdr = (uint8_t)hdrb; r.nunits = (uint16_t)nun;
            recs[idx - start] = r;
        }

        // the access units that start in this round, in order (wave-uniform)
        const unsigned long long start_m = __ballot(au_start), gap_m = __ballot(gap), mark_m = __ballot(good && marker);
        const unsigned long long after_m = __ballot(open_after);
        const unsigned long long key_m = __ballot((fl & EDGPU_TAP_KEY) != 0), par_m = __ballot((fl & EDGPU_TAP_PARAMS) != 0);
        const unsigned long long dmg_m = __ballot((fl & EDGPU_TAP_DAMAGED) != 0);
        uint32_t lo_lane = 0;                                   // the open unit's first lane in this round
        for (unsigned long long m = start_m; m; m &= m - 1) {
            const uint32_t h = (uint32_t)__ffsll((long long)m) - 1;
            const unsigned long long bh = (1ull << h) - 1ull;
            const unsigned long long gbh = good_m & bh;
            const uint32_t plh = gbh ? top_bit(gbh) : 0u;
            const unsigned long long range = bh & ~((1ull << lo_lane) - 1ull);
            // totals before lane h
            const uint32_t xb = h ? lane_of(in_bytes, h - 1) : 0u, xc2 = h ? lane_of(in_c2, h - 1) : 0u;
            const uint64_t off_h = t_bytes + xb;
            const uint32_t nals_h = t_nals + (xc2 >> 8), good_h = t_good + (uint32_t)__popcll(gbh);
            if (au_open) {                                      // the unit before it is complete
                const uint32_t last_m = gbh ? bit_of(mark_m, plh) : c_prev_m;
                const uint32_t chain_open = gbh ? bit_of(after_m, plh) : (c_chain != kNoChain ? 1u : 0u);
                uint32_t f = au_flags | ((key_m & range) ? EDGPU_TAP_KEY : 0u) | ((par_m & range) ? EDGPU_TAP_PARAMS : 0u) |
                             ((dmg_m & range) ? EDGPU_TAP_DAMAGED : 0u);
                if (chain_open || (bit_of(gap_m, h) && !last_m)) f |= EDGPU_TAP_DAMAGED;
                if (!last_m) f |= EDGPU_TAP_NOMARKER;
                if (lane == 0) {
                    edgpu_tap_unit u;
                    u.offset = au_off; u.bytes = (uint32_t)(off_h - au_off); u.rtp_ts = au_ts; u.arrival_ms = (int64_t)au_arrival;
                    u.flags = f; u.first_seq = au_seq; u.n_packets = good_h - au_good0; u.n_nals = nals_h - au_nals0;
                    u.stream = 0; u._pad = 0;
                    units[n_units] = u;
                }
                n_units++;
                n_damaged += (f & EDGPU_TAP_DAMAGED) ? 1u : 0u;
            }
            // the unit that starts at lane h; if it stays incomplete the drain ends before it
            au_flags = (pending && !au_open && n_units == 0) ? (uint32_t)EDGPU_TAP_DAMAGED : 0u;
            au_open = 1;
            au_off = off_h; au_nals0 = nals_h; au_good0 = good_h;
            au_ts = lane_of(ts, h); au_seq = lane_of(seq, h);
            au_arrival = (uint64_t)lane_of(m1.x, h) | ((uint64_t)lane_of(m1.y, h) << 32);
            if (gbh) {
                const uint32_t c1 = lane_of(in_c1, plh), c2 = lane_of(in_c2, plh);
                au_cut = base + plh + 1;
                au_tally = Tally{tot.packets + (c1 & 0xFFu), tot.skipped + ((c1 >> 8) & 0xFFu), tot.malformed + ((c1 >> 16) & 0xFFu),
                                 tot.orphans + (c1 >> 24), tot.unsupported + (c2 & 0xFFu)};
                au_has_prev = 1; au_prev_seq = lane_of(seq, plh);
            } else {
                au_cut = c_good_end; au_tally = at_good; au_has_prev = c_has_prev; au_prev_seq = c_prev_seq;
            }
            lo_lane = h;
        }
        // the round's part of the unit still open
        {
            const unsigned long long range = ~((1ull << lo_lane) - 1ull);
            if (au_open)
                au_flags |= ((key_m & range) ? EDGPU_TAP_KEY : 0u) | ((par_m & range) ? EDGPU_TAP_PARAMS : 0u) |
                            ((dmg_m & range) ? EDGPU_TAP_DAMAGED : 0u);
        }
        // carry
        const uint32_t e1 = lane_of(in_c1, 63), e2 = lane_of(in_c2, 63);
        if (good_m) {
            const uint32_t L = top_bit(good_m);
            const uint32_t c1 = lane_of(in_c1, L), c2 = lane_of(in_c2, L);
            at_good = Tally{tot.packets + (c1 & 0xFFu), tot.skipped + ((c1 >> 8) & 0xFFu), tot.malformed + ((c1 >> 16) & 0xFFu),
                            tot.orphans + (c1 >> 24), tot.unsupported + (c2 & 0xFFu)};
            c_has_prev = 1; c_first = 0;
            c_prev_seq = lane_of(seq, L); c_prev_ts = lane_of(ts, L); c_prev_m = bit_of(mark_m, L);
            c_chain = bit_of(after_m, L) ? lane_of(ftype, L) : kNoChain;
            c_good_end = base + L + 1;
            t_good += (uint32_t)__popcll(good_m);
        }
        tot = Tally{tot.packets + (e1 & 0xFFu), tot.skipped + ((e1 >> 8) & 0xFFu), tot.malformed + ((e1 >> 16) & 0xFFu),
                    tot.orphans + (e1 >> 24), tot.unsupported + (e2 & 0xFFu)};
        t_bytes += lane_of(in_bytes, 63);
        t_nals += e2 >> 8;
    }

    // the last unit: complete with a marker, emitted open by a flush, else left waiting
    uint64_t cut = flush ? head : start, d_bytes = t_bytes;
    Tally fin = flush ? tot : Tally{0, 0, 0, 0, 0};
    uint32_t o_has_prev = c_has_prev, o_prev_seq = c_prev_seq;
    if (au_open) {
        uint32_t f = au_flags;
        if (c_chain != kNoChain) f |= EDGPU_TAP_DAMAGED;
        if (c_prev_m || flush) {
            if (!c_prev_m) f |= EDGPU_TAP_NOMARKER | EDGPU_TAP_OPEN_END;
            if (lane == 0) {
                edgpu_tap_unit u;
                u.offset = au_off; u.bytes = (uint32_t)(t_bytes - au_off); u.rtp_ts = au_ts; u.arrival_ms = (int64_t)au_arrival;
                u.flags = f; u.first_seq = au_seq; u.n_packets = t_good - au_good0; u.n_nals = t_nals - au_nals0;
                u.stream = 0; u._pad = 0;
                units[n_units] = u;
            }
            n_units++;
            n_damaged += (f & EDGPU_TAP_DAMAGED) ? 1u : 0u;
            if (!flush) { cut = c_good_end; fin = at_good; }
        } else {
            cut = au_cut; fin = au_tally; d_bytes = au_off;
            o_has_prev = au_has_prev; o_prev_seq = au_prev_seq;
        }
    }
    if (lane == 0) {
        T.d_start = start; T.d_cut = cut; T.d_bytes = d_bytes;
        T.d_nrec = (uint32_t)(cut - start); T.d_nunits = n_units;
        T.d_has_prev = o_has_prev; T.d_prev_seq = o_prev_seq;
        T.d_pending = (pending && n_units == 0) ? 1u : 0u;
        T.d_damaged = n_damaged;
        T.d_packets = fin.packets; T.d_skipped = fin.skipped; T.d_malformed = fin.malformed;
        T.d_orphans = fin.orphans; T.d_unsupported = fin.unsupported;
    }
}

__global__ __launch_bounds__(256) void k_tap_place(TapParams P) {
    __shared__ uint64_t scratch[kPlaceThreads / 64];
    uint64_t c_bytes = 0, c_units = 0, c_items = 0, c_uitems = 0;
    uint32_t* items = P.items;
    uint32_t* uitems = P.items + P.ntaps + 1;
    for (uint32_t b = 0; b < P.ntaps; b += kPlaceThreads) {
        const uint32_t i = b + threadIdx.x;
        uint64_t by = 0, un = 0, it = 0, ui = 0;
        TapDev* T = nullptr;
        if (i < P.ntaps) {
            T = &P.taps[P.list[i]];
            by = (T->d_bytes + 15) & ~15ull;
            un = T->d_nunits;
            it = (T->d_nrec + kTapRound - 1) / kTapRound;
            ui = (T->d_nunits + kTapRound - 1) / kTapRound;
        }
        uint64_t t_by, t_un, t_it, t_ui;                    // the block's totals; the carries are every thread's copy
        const uint64_t o_by = c_bytes + block_exclusive_scan<uint64_t>(by, scratch, t_by);
        const uint64_t o_un = c_units + block_exclusive_scan<uint64_t>(un, scratch, t_un);
        const uint64_t o_it = c_items + block_exclusive_scan<uint64_t>(it, scratch, t_it);
        const uint64_t o_ui = c_uitems + block_exclusive_scan<uint64_t>(ui, scratch, t_ui);
        c_bytes += t_by; c_units += t_un; c_items += t_it; c_uitems += t_ui;
        if (T) {
            T->p_offset = o_by;
            T->p_unit_first = (uint32_t)o_un;
            items[i] = (uint32_t)o_it;
            uitems[i] = (uint32_t)o_ui;
        }
    }
    const bool commit = c_bytes <= P.out_cap && c_units <= P.unit_cap && P.ntaps <= P.stream_cap;
    if (threadIdx.x == 0) {
        items[P.ntaps] = (uint32_t)c_items;
        uitems[P.ntaps] = (uint32_t)c_uitems;
        TapPlace pl;
        pl.bytes = c_bytes; pl.units = (uint32_t)c_units; pl.streams = P.ntaps; pl.commit = commit ? 1u : 0u;
        pl.n_items = (uint32_t)c_items; pl.n_uitems = (uint32_t)c_uitems; pl._pad = 0;
        *P.place = pl;
    }
    if (!commit) return;
    for (uint32_t i = threadIdx.x; i < P.ntaps; i += kPlaceThreads) {
        TapDev& T = P.taps[P.list[i]];
        T.missed += T.d_start > T.head ? T.d_start - T.head : 0ull;
        T.head = T.d_cut;
        T.has_prev = T.d_has_prev; T.prev_seq = T.d_prev_seq; T.pending = T.d_pending;
        T.packets += T.d_packets; T.skipped += T.d_skipped; T.malformed += T.d_malformed;
        T.orphans += T.d_orphans; T.unsupported += T.d_unsupported;
        T.units += T.d_nunits; T.damaged_units += T.d_damaged;
        edgpu_tap_stream s;
        s.session = T.session; s.track = T.track; s.offset = T.p_offset; s.bytes = T.d_bytes;
        s.unit_first = T.p_unit_first; s.unit_count = T.d_nunits;
        s.packets = T.packets; s.skipped = T.skipped; s.malformed = T.malformed; s.orphans = T.orphans;
        s.unsupported = T.unsupported; s.missed = T.missed; s.units = T.units; s.damaged_units = T.damaged_units;
        P.streams[i] = s;
    }
}

namespace {

// `len` bytes from virtual ring byte `s0` to `d`, after the prefix `kind` asks for, by the 16 lanes
// of a group (`sub` 0..15): whole 16-B words where the destination is aligned, bytes at its ends.
__device__ __forceinline__ void copy_piece(uint8_t* d, uint32_t kind, uint32_t hdr, const u32x4* ring, uint32_t word_mask,
                                           uint64_t s0, uint32_t len, uint32_t sub) {
    if (kind >= kTapStart) {
        if (sub < 4) d[sub] = sub == 3 ? 1 : 0;
        d += 4;
        if (kind == kTapStartHdr) {
            if (sub == 4) d[0] = (uint8_t)hdr;
            d += 1;
        }
    }
    const uintptr_t d0 = (uintptr_t)d, d1 = d0 + len;
    const uintptr_t a0 = min((d0 + 15) & ~(uintptr_t)15, d1), a1 = max(d1 & ~(uintptr_t)15, a0);
    if (sub < a0 - d0) d[sub] = (uint8_t)ring_byte(ring, word_mask, s0 + sub);
    if (sub < d1 - a1) reinterpret_cast<uint8_t*>(a1)[sub] = (uint8_t)ring_byte(ring, word_mask, s0 + (a1 - d0) + sub);
    const uint32_t nw = (uint32_t)((a1 - a0) >> 4);
    const uint64_t sp = s0 + (a0 - d0);
    const uint32_t sh = (uint32_t)(sp & 15u);
    const uint64_t w0 = sp >> 4;
    u32x4* out = reinterpret_cast<u32x4*>(a0);
    for (uint32_t w = sub; w < nw; w += 16) {
        const u32x4 lo = ring[(size_t)((w0 + w) & word_mask)];
        const u32x4 hi = sh ? ring[(size_t)((w0 + w + 1) & word_mask)] : lo;
        out[w] = funnel16(lo, hi, sh);
    }
}

}  // namespace

__global__ __launch_bounds__(256) void k_tap_copy(TapParams P) {
    const TapPlace pl = *P.place;
    if (!pl.commit) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    const uint32_t total = pl.n_items + pl.n_uitems;
    for (uint32_t item = wave; item < total; item += nwaves) {
        const bool is_units = item >= pl.n_items;
        const uint32_t k = is_units ? item - pl.n_items : item;
        const uint32_t* base = P.items + (is_units ? P.ntaps + 1 : 0u);
        uint32_t lo = 0, hi = P.ntaps;                      // base[lo] <= k < base[hi]
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (base[mid] <= k) lo = mid; else hi = mid;
        }
        const TapDev& T = P.taps[P.list[lo]];
        const uint32_t r = k - base[lo];
        if (is_units) {
            const uint32_t j = r * kTapRound + lane;
            if (j < T.d_nunits && T.p_unit_first + j < P.unit_cap) {
                edgpu_tap_unit u = reinterpret_cast<const edgpu_tap_unit*>(T.unit)[j];
                u.offset += T.p_offset;
                u.stream = lo;
                P.units[T.p_unit_first + j] = u;
            }
            continue;
        }
        if (T.sender >= P.nsenders) continue;
        const SenderDev& D = P.senders[T.sender];
        const u32x4* ring = reinterpret_cast<const u32x4*>(D.ring);
        const PktMeta* meta = reinterpret_cast<const PktMeta*>(D.meta);
        const uint32_t word_mask = D.word_mask, pk_mask = D.pk_mask;
        const TapRec* recs = reinterpret_cast<const TapRec*>(T.rec);
        const uint32_t nrec = T.d_nrec, sub = lane & 15u;
        const uint64_t first = T.d_start, d_bytes = T.d_bytes;
        uint8_t* out = P.out + T.p_offset;
        for (uint32_t q = lane >> 4; q < kTapRound; q += 4) {
            const uint32_t j = r * kTapRound + q;
            if (j >= nrec) break;
            const TapRec rec = recs[j];
            if (rec.kind == kTapNone) continue;
            const uint64_t slot = meta[(first + j) & pk_mask].vbyte;
            if (rec.kind != kTapStap) {
                const uint32_t pre = rec.kind == kTapStart ? 4u : rec.kind == kTapStartHdr ? 5u : 0u;
                if (rec.dst + pre + rec.len <= d_bytes)
                    copy_piece(out + rec.dst, rec.kind, rec.hdr, ring, word_mask, slot + rec.src, rec.len, sub);
            } else {
                uint64_t s = slot + rec.src, d = rec.dst;
                for (uint32_t u = 0; u < rec.nunits; u++) {
                    const uint32_t size = (ring_byte(ring, word_mask, s) << 8) | ring_byte(ring, word_mask, s + 1);
                    if (d + 4 + size > d_bytes) break;
                    copy_piece(out + d, kTapStart, 0, ring, word_mask, s + 2, size, sub);
                    s += 2 + size;
                    d += 4 + size;
                }
            }
        }
    }
}

hipError_t launch_tap_drain(const TapParams& p, uint32_t copy_blocks, hipStream_t st) {
    if (!p.ntaps) return hipSuccess;
    EDGPU_LAUNCH(k_tap_scan, dim3(p.ntaps), dim3(64), 0, st, p);
    EDGPU_LAUNCH(k_tap_place, dim3(1), dim3(kPlaceThreads), 0, st, p);
    EDGPU_LAUNCH(k_tap_copy, dim3(copy_blocks), dim3(256), 0, st, p);
    return hipGetLastError();
}

}  // namespace edgpu
