// edgpu_params.h -- kernel argument blocks (shared by edgpu_kernels.hip and edgpu_engine.cpp).
#pragma once
#include <stdint.h>
#include "edgpu.h"
#include "edgpu_device.h"

// The library has the two fan-out kernels and one ingest kernel it runs.  The measurement build
// (`make ab`: every fan-out variant ever measured, the EDGPU_ABLATE skip-work bits, the
// alternative ingest copy paths EDGPU_INGEST / EDGPU_INGEST_TCP) was removed; its code is in git
// at commit 0dd0039, its numbers in docs/MEASUREMENT_HISTORY.md (A.1-A.3).
namespace edgpu {

// Kernel launches made on this thread (edgpu_counters.kernel_launches: the engine adds what each
// API call launched).  Every launch goes through EDGPU_LAUNCH.
extern thread_local uint64_t tl_launches;
#define EDGPU_LAUNCH(...)                          \
    do {                                           \
        ++::edgpu::tl_launches;                    \
        hipLaunchKernelGGL(__VA_ARGS__);           \
    } while (0)

// Interleaved frames a k_ingest wave copies per round (all their loads before the first
// store): 4 since the copy is specialised on the frame's word offset (128 VGPRs, 4 waves per
// SIMD); it was 2
constexpr uint32_t kTcpFramesPerRound = 4;

struct TcpGroup;
struct TcpChunkRes;
struct TcpRead;

struct IngestParams {
    const edgpu_pkt_desc* desc;
    const uint32_t* seg_off;
    const uint32_t* seg_sess;
    const uint8_t* blob;
    const uint64_t* src_addr;   // per desc: device address of the frame ('$' header first, any
                                // alignment) instead of blob + slot * 16 (interleaved ingest); or null
    SessionDev* sessions;
    SenderDev* senders;
    StreamDev* streams;
    uint32_t npk;           // descriptors in the batch
    uint32_t spec_min;      // the speculative copy from this many packets per segment on (0: never)
    uint32_t host_epoch;    // != 0: the blob is a host batch the host keeps for the tick; record each
                            // packet's slot and the batch (edgpu_fanout_sources)
    TickTotals* totals;
    uint32_t ing_slot;      // this batch's ingest counters: TickTotals.ing_pk / ing_b [ing_slot]
    // reflector_use_in_packet_receive_time / reflector_in_packet_max_receive_sec
    // (ReflectorStream.cpp:103-107, 113): strip a 12-byte "aktt" BE64 receive-time trailer and
    // rebase the packet's arrival on it (:1960-1994)
    uint32_t recv_time;
    int64_t max_future_ms;  // sMaxFuturePacketMSec
    // Interleaved ingest (null otherwise): segment g is deframe group g, and k_ingest finds each
    // frame itself -- its chunk from the per-chunk results, its start from the walk's recorded
    // starts, its length and channel from its own '$' header, its arrival from the reads --
    // instead of reading a per-frame descriptor.  Frames of chunks the walk did not record
    // (cand kTcpNone, or more than kTcpFrames frames) come from desc / src_addr (k_tcp_finish).
    const TcpGroup* tcp_groups;
    const TcpChunkRes* tcp_chunkres;
    const uint16_t* tcp_offs;
    const TcpRead* tcp_reads;
    const uint8_t* tcp_raw;
    const uint8_t* tcp_stage;
};

struct PlanParams {
    SenderDev* senders;
    SubDev* subs;
    const uint32_t* sub_index;
    const uint32_t* sub_pos;    // SubDev index -> position in sub_index order (~0: inactive)
    const uint32_t* sub_range;  // per sender [begin, end) into sub_index
    edgpu_substream_out* sub_out;
    FanWork* work;
    FanSub* fansub;             // per sub_index position
    uint64_t* blk_bytes;        // per K2 block partials
    uint32_t* blk_count;
    uint64_t* blk_maxb;         // per K2 block: the largest sub-stream (bytes, descriptors)
    uint32_t* blk_maxc;
    SessionDev* sessions;       // stream errors (per-session isolation)
    TickTotals* totals;
    GrowReq* grow;              // ring growth requests (kMaxGrow)
    TickParams T;
};

struct FanoutParams {
    const SenderDev* senders;
    const uint32_t* sub_range;  // per sender [begin, end) into sub_index
    const SubDev* subs;
    const uint32_t* sub_index;
    const FanWork* work;
    const FanSub* fansub;
    uint8_t* arena;
    edgpu_out_desc* desc;
    uint64_t arena_words;       // capacities: stores outside them are dropped and flagged
    uint32_t max_desc;
    TickTotals* totals;
};

// ---- RTSP-interleaved ingest ('$'-deframe of pusher TCP reads, edgpu_ingest_interleaved) ----
// A session's stream in one call = its carried bytes (a partial frame from the previous call)
// followed by its reads.  The stream is cut into kTcpChunk-byte chunks walked in parallel from
// every '$' that can start a frame in the chunk's first kTcpMaxFrame bytes; the true walk is
// then stitched chunk to chunk (k_tcp_resolve).
#ifndef EDGPU_TCP_CHUNK
#define EDGPU_TCP_CHUNK 32768                // 32 KiB: ingest incl. deframe 0.405 vs 0.421 ms at 16 KiB,
                                             // 0.479 at 8 KiB (profiles/r02z28_tcp_chunk_ab/)
#endif
constexpr uint32_t kTcpChunk = EDGPU_TCP_CHUNK;   // stream bytes per walk chunk
#ifndef EDGPU_TCP_SPEC
#define EDGPU_TCP_SPEC 0                     // frame headers guessed per burst of the walk (0: none);
                                             // 4 / 8 / 16 measured slower (profiles/r02z30_tcp_spec_ab/,
                                             // r02z33_tcp_walk_spec_ab/)
#endif
constexpr uint32_t kTcpSpec = EDGPU_TCP_SPEC;
#ifndef EDGPU_TCP_CAND_FUSED
#define EDGPU_TCP_CAND_FUSED 0               // 1: a chunk's two candidate windows loaded at once (A/B)
#endif
#ifndef EDGPU_TCP_WALK_CPW
#define EDGPU_TCP_WALK_CPW 2                 // chunks walked side by side per wave (1, 2 or 4): walk
                                             // ~100 -> 60 us (profiles/r02z32_tcp_walk_ab/); four
                                             // (16 / 24 / 32 KiB chunks) slower: 0.289 / 0.285 /
                                             // 0.289 vs 0.281 ms (profiles/r03t_walk_shape_ab/)
#endif
constexpr int kTcpWalkCpw = EDGPU_TCP_WALK_CPW;
#ifndef EDGPU_TCP_WALK_WPE
#define EDGPU_TCP_WALK_WPE 8                 // waves per SIMD asked of k_tcp_walk's registers (63 VGPRs, no spill)
#endif
static_assert(kTcpChunk >= 4096 && kTcpChunk + 2 * 2051 <= 65536, "chunk offsets are 16-bit");
constexpr uint32_t kTcpCands = 64;         // candidates kept per chunk (more: sequential walk)
constexpr uint32_t kTcpFrames = 32;        // frame starts recorded per candidate walk
constexpr uint32_t kTcpMaxFrame = 2047;    // usable request-buffer bytes (QTSS_MAX_REQUEST_BUFFER_SIZE - 1)
constexpr uint32_t kTcpCarry = 2048;       // per-session carry buffer / staged frame
constexpr uint32_t kTcpNone = 0xFFFFFFFFu;

// walk outcome codes (TcpCand.code, TcpGroup.code)
constexpr uint32_t kWalkRun = 0;           // reached the chunk end / the stream end
constexpr uint32_t kWalkPartial = 1;       // incomplete frame at `exit`: carried
constexpr uint32_t kWalkMessage = 2;       // non-'$' byte at a frame boundary: an RTSP message
constexpr uint32_t kWalkDropped = 3;       // frame longer than the request buffer: connection dropped

struct TcpGroup {           // one pusher connection's reads in this call
    uint32_t session, first_read, nreads, first_chunk;
    uint32_t nchunks, carry_len;
    uint64_t raw_off;       // raw-buffer offset of the first read
    uint64_t len;           // stream bytes: carry_len + the reads' bytes
    // k_tcp_resolve
    uint32_t nframes, code;
    uint64_t stop;          // stream position where the walk ended (len: everything framed)
    // k_tcp_scan
    uint32_t frame_base, _pad;
};

struct TcpRead { uint64_t start; int64_t arrival; uint32_t len, _pad; };   // start: stream position
struct TcpCand { uint32_t q, exit, nframes, code; };                        // q / exit: chunk offsets
struct TcpChunkRes { uint32_t entry, fbase, nframes, cand; };   // entry kTcpNone: idle; cand kTcpNone: re-walk
struct TcpTotals { uint32_t frames; int32_t status; };

struct TcpParams {
    TcpGroup* groups;
    uint32_t ngroups, nchunks;
    const TcpRead* reads;
    const uint32_t* chunk_group;
    TcpCand* cands;         // nchunks x kTcpCands
    uint16_t* offs;         // nchunks x kTcpCands x kTcpFrames: frame starts of each candidate walk
    uint8_t* links;         // nchunks x kTcpCands: next chunk's candidate, 0xFE terminal, 0xFF search
    uint32_t* ncand;
    TcpChunkRes* chunkres;
    const uint8_t* raw;
    uint64_t raw_bytes;
    uint8_t* carry;         // per session kTcpCarry bytes
    uint8_t* stage;         // per group kTcpCarry bytes: a frame that starts in the carried bytes
    edgpu_pkt_desc* desc;
    uint64_t* src_addr;     // per frame: its address for k_ingest (IngestParams.src_addr)
    uint32_t max_desc;
    uint32_t* seg_off;      // ngroups + 1
    uint32_t* seg_sess;
    edgpu_tcp_result* results;
    TcpTotals* tot;
    uint32_t walk;          // 0: k_tcp_walk + k_tcp_resolve (candidate windows, every chunk at once);
                            // 1: k_tcp_chain (each stream walked in order, one lane per session);
                            // 2: k_tcp_walk_seg + k_tcp_resolve (candidate windows every `seg` chunks)
    uint32_t seg;           // walk 2: chunks per segment
};

struct BlockedParams {
    const edgpu_blocked* reports;
    uint32_t n;
    SubDev* subs;
    const SenderDev* senders;
    SessionDev* sessions;
    int64_t now;                // the tick's clock
    int64_t relocate_ms;        // sRelocatePacketAgeMSec (rtp_reflector_threshold_msec)
    TickTotals* totals;
};

// Per-stream reception statistics (edgpu_stats.hip): k_stream_stats after every ingest while a
// session is enabled, k_stream_bitrate at edgpu_stream_stats_sample.
struct StatsParams {
    const SenderDev* senders;
    StatDev* stats;
    uint32_t nstreams;          // rows of `stats`
    uint32_t nsenders;          // rows of `senders` (a row naming a sender outside them is skipped)
    int64_t now;                // k_stream_bitrate: the sample's clock
};
hipError_t launch_stream_stats(const StatsParams& p, hipStream_t st);
hipError_t launch_stream_bitrate(const StatsParams& p, hipStream_t st);

// The H.264 elementary-stream tap (edgpu_tap.hip): one drain is k_tap_scan (a wave per enabled
// tap), k_tap_place (one workgroup) and k_tap_copy.
constexpr uint32_t kTapRound = EDGPU_TAP_ROUND;     // queue entries per scan round and per copy item
struct TapParams {
    const SenderDev* senders;
    TapDev* taps;
    const uint32_t* list;       // the enabled taps' rows, ascending
    uint32_t ntaps;
    uint32_t nsenders;
    uint32_t flags;             // EDGPU_TAP_FLUSH
    uint32_t unit_cap, stream_cap;
    uint64_t out_cap;
    uint8_t* out;
    edgpu_tap_unit* units;      // device staging of the caller's arrays
    edgpu_tap_stream* streams;
    uint32_t* items;            // 2 x (ntaps + 1): exclusive sums of the taps' record rounds, unit rounds
    TapPlace* place;
};
hipError_t launch_tap_drain(const TapParams& p, uint32_t copy_blocks, hipStream_t st);

// The AAC audio tap (edgpu_aac.hip): one drain is k_aac_scan (a wave per enabled tap), k_aac_place
// (one workgroup) and k_aac_copy.
constexpr uint32_t kAacRound = 64;                  // queue entries per scan round and per copy item
struct AacParams {
    const SenderDev* senders;
    AacDev* taps;
    const uint32_t* list;       // the enabled taps' rows, ascending
    uint32_t ntaps;
    uint32_t nsenders;
    uint32_t flags;             // EDGPU_AAC_FLUSH
    uint32_t frame_cap, stream_cap;
    uint64_t out_cap;
    uint8_t* out;
    edgpu_aac_frame* frames;    // device staging of the caller's arrays
    edgpu_aac_stream* streams;
    uint32_t* items;            // ntaps + 1: exclusive sums of the taps' record rounds
    AacPlace* place;
};
hipError_t launch_aac_drain(const AacParams& p, uint32_t copy_blocks, hipStream_t st);

// The transport-stream mux (edgpu_ts_mux, edgpu_ts.hip): k_ts_plan (a wave per stream row),
// k_ts_place (one workgroup) and k_ts_pack (flat over the output's 16-B words).
struct TsRec {                  // what k_ts_plan leaves per unit for k_ts_pack; zero for a unit no row covers
    uint64_t pts;               // 33 bits
    uint32_t pk;                // its first packet, relative to the stream's
    uint32_t npk;               // its packets, PAT / PMT included
    uint32_t misc;              // cc_video | cc_pat << 4 | cc_pmt << 8 | key << 12 | aud << 13 of its first packets
    uint32_t stream;
    uint32_t flags, _pad;       // the tap unit's
};
static_assert(sizeof(TsRec) == 32, "TsRec layout");
struct TsRange { uint32_t first, count; };
struct TsPlace {                // k_ts_place's verdict
    uint64_t bytes;
    uint32_t packets;
    uint32_t commit;
};
struct TsParams {
    const uint8_t* es;
    const edgpu_tap_unit* units;
    const TsRange* ranges;      // per stream row: its units
    const edgpu_ts_state* states;
    edgpu_ts_state* new_states;
    TsRec* recs;                // n_units
    uint32_t* base;             // n_streams + 1: k_ts_plan leaves each stream's packets, k_ts_place their exclusive sums
    TsPlace* place;
    const uint32_t* tmpl;       // PAT and PMT packets, 47 words each
    uint8_t* out;
    edgpu_ts_unit* ts_units;
    uint64_t out_cap;
    uint64_t pts_offset;
    uint32_t n_units, n_streams;
    uint32_t pcr_lead;
    uint32_t video_pid;
    uint32_t aud;
};
hipError_t launch_ts_mux(const TsParams& p, uint32_t pack_blocks, hipStream_t st);

// The start codes of an elementary stream, as the fragmented-MP4 and the FLV mux find them
// (edgpu_scode.h): a bitmap of every 00 00 00 01 and the distance from each to the next.
constexpr uint32_t kScodeNone = 0xFFFFFFFFu;
constexpr uint32_t kScodeChunkWords = 64;   // bitmap words (of 32 ES bytes) one wave marks: a chunk is 2 KiB of ES
constexpr uint32_t kScodeChunkBytes = kScodeChunkWords * 32;
struct ScodeView {
    const uint8_t* es;
    uint64_t es_bytes;
    uint32_t* bitmap;           // nwords: bit b of word w: a start code begins at ES byte 32 w + b
    uint32_t* chunk_first;      // nchunks: the chunk's first start code, relative, or kScodeNone
    uint32_t* lens;             // es_bytes / 4 + 1: at [q >> 2], the bytes from start code q's end to the next start code (or the ES end)
    uint64_t nwords, nchunks;
};

// The fragmented-MP4 mux (edgpu_mp4_mux, edgpu_mp4.hip): k_mp4_mark and k_mp4_resolve (flat over the
// ES: the start codes and the distance from each to the next), k_mp4_plan (a wave per stream row),
// k_mp4_place (one workgroup), k_mp4_rows (flat over fragments and units) and k_mp4_pack (flat over
// the output's 16-B words).
constexpr uint32_t kMp4None = 0xFFFFFFFFu;
struct Mp4Range { uint32_t first, count, slot, _pad; };   // slot: the row's first Mp4FragRec (the rows before it hold count + 1 each)
struct Mp4Rec {                 // per unit, from k_mp4_plan; zero for a unit no row covers
    uint64_t dts;
    uint32_t slot;              // Mp4FragRec of its fragment
    uint32_t poff;              // of its bytes in the fragment's mdat payload
    uint32_t rank;              // its sample number within the stream's call
    uint32_t duration;          // written by the lane of the stream's next sample
    uint32_t flags;             // the sample row's | kind << 30: 0 uncovered, 1 no bytes, 2 a sample
    uint32_t _pad;
};
static_assert(sizeof(Mp4Rec) == 32, "Mp4Rec layout");
struct Mp4FragRec {             // per fragment start, and one more that closes the stream's last fragment
    uint64_t tfdt;
    uint64_t dsum;              // durations of the stream's samples before it
    uint32_t unit_first;
    uint32_t rank;              // samples of the stream before it
    uint32_t bex;               // ES bytes of the stream before it
    uint32_t prev_or;           // OR of the flags of the fragment it closes
};
static_assert(sizeof(Mp4FragRec) == 32, "Mp4FragRec layout");
struct Mp4StreamRec { uint64_t bytes, base; uint32_t nfrags, fbase; };
struct Mp4Samp { uint64_t off; uint32_t unit, _pad; };      // a stream's samples in order: offset in the stream's run
struct Mp4Place { uint64_t bytes; uint32_t frags, commit; };
struct Mp4Params {
    ScodeView sc;               // the ES and its start codes
    const edgpu_tap_unit* units;
    const Mp4Range* ranges;
    const edgpu_mp4_state* states;
    edgpu_mp4_state* new_states;
    Mp4Rec* recs;               // n_units
    Mp4FragRec* frecs;          // n_units + n_streams
    Mp4StreamRec* srecs;        // n_streams
    Mp4Samp* samps;             // n_units
    Mp4Place* place;
    uint8_t* out;
    edgpu_mp4_sample* rows;     // n_units
    edgpu_mp4_frag* frags;      // n_units (staging holds the most there can be)
    uint64_t out_cap;
    uint64_t time_offset;
    uint32_t frag_cap, n_units, n_streams, n_slots;
    uint32_t max_samples, default_duration;
};
hipError_t launch_mp4_mux(const Mp4Params& p, uint32_t flat_blocks, hipStream_t st);

// The FLV mux (edgpu_flv_mux, edgpu_flv.hip): k_flv_mark and k_flv_resolve (the start codes, as the
// fragmented-MP4 mux finds them), k_flv_plan (a wave per stream row), k_flv_place (one workgroup)
// and k_flv_pack (flat over the output's 16-B words, then over the tag rows).
struct FlvRange { uint32_t first, count; };
struct FlvRec {                 // per unit, from k_flv_plan; zero for a unit no row covers
    uint32_t pre;               // of its tag, relative to the stream's run
    uint32_t ts_ms;
    uint32_t flags;             // the tag row's | kind << 30: 0 uncovered, 1 no bytes, 2 a tag
    uint32_t stream;
    uint32_t sps_offset, sps_bytes, pps_offset, pps_bytes;
};
static_assert(sizeof(FlvRec) == 32, "FlvRec layout");
struct FlvStreamRec { uint64_t bytes, base; };
struct FlvPlace { uint64_t bytes; uint32_t commit, _pad; };
struct FlvParams {
    ScodeView sc;               // the ES and its start codes
    const edgpu_tap_unit* units;
    const FlvRange* ranges;
    const edgpu_flv_state* states;
    edgpu_flv_state* new_states;
    FlvRec* recs;               // n_units
    FlvStreamRec* srecs;        // n_streams
    FlvPlace* place;
    uint8_t* out;
    edgpu_flv_tag* rows;        // n_units
    uint64_t out_cap;
    uint64_t time_offset;
    uint32_t n_units, n_streams;
};
hipError_t launch_flv_mux(const FlvParams& p, uint32_t flat_blocks, hipStream_t st);

struct ImageParams {
    SenderDev* senders;
    SessionDev* sessions;
    StreamDev* streams;
    ImgPlan* plan;
    uint32_t nplan;
    int64_t now;
    int64_t over_buffer_ms;
    uint8_t* buf;           // export: destination images; import: source images
    int* status;            // first error wins
};

}  // namespace edgpu
