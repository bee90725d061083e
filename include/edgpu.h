/*
 * edgpu.h -- C ABI of the MI355X-native batched RTP relay engine (libedgpu.so).
 *
 * The engine replaces EasyDarwin's reflector hot path behind the QTSSReflectorModule
 * plugin boundary.  Each entry point names the reference interface it stands in for
 * (paths relative to the EasyDarwin reference tree):
 *
 *   edgpu_session_add      ReflectorSession::SetupReflectorSession
 *                          (APIModules/QTSSReflectorModule/ReflectorSession.cpp:140-188) with the
 *                          SDP parse of SDPSourceInfo (APICommonCode/SDPSourceInfo.cpp:259-353)
 *   edgpu_session_remove   the end of a ReflectorSession: RemoveOutput's refcount-0 branch
 *                          (QTSSReflectorModule.cpp:2162-2192) with TearDownAllOutputs when a
 *                          broadcast stops with kill_clients (:2156-2159, ReflectorSession.cpp:
 *                          281-285)
 *   edgpu_subscriber_add   RTPSessionOutput ctor + ReflectorSession::AddOutput
 *                          (RTPSessionOutput.cpp:73-88, ReflectorSession.cpp:209-253),
 *                          i.e. QTSSReflectorModule DoSetup/DoPlay for a player
 *                          (QTSSReflectorModule.cpp:1610-1622, 1942-1946)
 *   edgpu_subscriber_play  the same for an RTP-Info player: DoPlay + HaveStreamBuffers
 *                          (QTSSReflectorModule.cpp:1804-1865, 1971-2004)
 *   edgpu_subscriber_remove ReflectorSession::RemoveOutput (ReflectorSession.cpp:255-279)
 *   edgpu_subscriber_rewrite the per-output seq / timestamp / SSRC rewrite the reference leaves
 *                          dead (RTPSessionOutput.cpp:403-561, 600-601, 685-773)
 *   edgpu_ingest           ReflectorStream::PushPacket + ReflectorSocket::ProcessPacket
 *                          (ReflectorStream.cpp:529-576, 1769-2010), called per packet by
 *                          ProcessRTPData (QTSSReflectorModule.cpp:604-678)
 *   edgpu_ingest_interleaved RTSPRequestStream::ReadRequest's '$' deframing of a pusher's
 *                          RTSP connection (Server.tproj/RTSPRequestStream.cpp:65-171) +
 *                          edgpu_ingest of the frames
 *   edgpu_keyframe_index   the keyframe index update + audio anchor inside ProcessPacket
 *                          (ReflectorStream.cpp:1876-1934, IsKeyFrameFirstPacket :1403-1513)
 *   edgpu_fanout           ReflectorSender::ReflectPackets / SendPacketsToOutput /
 *                          RTPSessionOutput::WritePacket and the egress framing of
 *                          RTPStream::Write (ReflectorStream.cpp:1024-1198,
 *                          RTPSessionOutput.cpp:564-662, Server.tproj/RTPStream.cpp:1084-1147,
 *                          RTSPSessionInterface.cpp:329-344), for every sender at once
 *   edgpu_udp_sources      the pusher RTCP-address update in ProcessPacket for UDP pushers
 *                          (ReflectorStream.cpp:1836-1866, NAT_WORKAROUND)
 *   edgpu_source_reports   ReflectorStream::SendReceiverReport on the RTCP sender's 5-s
 *                          timer (ReflectorStream.cpp:164-201, 510-527, 1039-1047)
 *
 * Conventions
 *   - Every function returns an int status using QTSS_Error values (QTSS.h:61-76):
 *     EDGPU_OK = QTSS_NoErr, EDGPU_ERR = QTSS_RequestFailed, EDGPU_BAD_ARGUMENT =
 *     QTSS_BadArgument, EDGPU_WOULD_BLOCK = QTSS_WouldBlock, plus engine-specific codes
 *     below -100 (capacity / device errors).  edgpu_last_error() gives a message.
 *   - One context per GPU.  Calls on a context are externally serialised (the reference's
 *     per-stream fBucketMutex); different contexts -- on different GPUs, or several on one GPU
 *     (replica sessions) -- may be called from different threads at the same time.
 *     edgpu_last_error() is per thread.
 *   - All device work runs on the context's HIP stream and is asynchronous unless stated.
 *     Pointers flagged EDGPU_PTR_DEVICE must stay valid until edgpu_sync() returns.
 *   - No torch or HIP types in the ABI: plain pointers and sizes.
 */
#ifndef EDGPU_H
#define EDGPU_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes (QTSS_Error-compatible where a reference counterpart exists) */
#define EDGPU_OK                 0
#define EDGPU_ERR               -1     /* QTSS_RequestFailed  */
#define EDGPU_BAD_ARGUMENT     -10     /* QTSS_BadArgument    */
#define EDGPU_WOULD_BLOCK      -14     /* QTSS_WouldBlock     */
#define EDGPU_NOT_CONNECTED    -15     /* QTSS_NotConnected   */
#define EDGPU_NO_DEVICE       -101     /* no usable gfx950 device / HIP failure */
#define EDGPU_OUT_OF_MEMORY   -102
#define EDGPU_RING_OVERFLOW   -103     /* a needed packet fell out of a sender ring */
#define EDGPU_TIMEOUT        -105     /* GPU watchdog: the device did not finish within watchdog_ms */
#define EDGPU_OUT_OVERFLOW    -104     /* a buffer too small (a fan-out sub-stream larger than the
                                          arena, a batch, a gather destination, ...) */

/* transport of a subscriber (qtssRTPTransportType, QTSS.h:219-221) */
#define EDGPU_TRANSPORT_UDP      0
#define EDGPU_TRANSPORT_TCP      1     /* RTSP-interleaved '$' framing */

/* pointer-location flags for edgpu_ingest */
#define EDGPU_PTR_HOST           0     /* host memory: copied to the device before the call returns */
#define EDGPU_PTR_DEVICE         1     /* already resident in HBM on the ctx device */
#define EDGPU_PTR_PINNED         2     /* pinned host memory from edgpu_host_alloc: copied to HBM
                                          asynchronously on the context's copy stream (below) */

/* Engine configuration.  Reflector prefs keep the reference's XML key names
 * (WinNTSupport/easydarwin.xml:131-163, read at ReflectorStream.cpp:87-117 and
 * QTSSReflectorModule.cpp:450-586); 0 selects the reference default. */
typedef struct edgpu_config {
    int32_t  device;                        /* HIP device ordinal */
    uint32_t reflector_buffer_size_sec;     /* default 1  -> 1000 ms new-client window */
    uint32_t rtp_reflector_threshold_msec;  /* default 2000, floor 1000 (relocation)   */
    uint32_t timeout_stream_SSRC_secs;      /* default 30                               */
    uint32_t use_one_SSRC_per_stream;       /* default 1 (0 = keep every SSRC) -- pass
                                               EDGPU_FALSE to disable                   */
    /* capacities (0 = default) */
    uint32_t video_ring_packets;            /* per video RTP sender, power of two (8192)  */
    uint64_t video_ring_bytes;              /* per video RTP sender, power of two (8 MiB) */
    uint32_t other_ring_packets;            /* audio/RTCP/other senders (2048)           */
    uint64_t other_ring_bytes;              /* (1 MiB)                                   */
    uint64_t out_arena_bytes;               /* fan-out output arena per tick (256 MiB)   */
    uint32_t max_out_packets;               /* descriptor capacity per tick (1 Mi)       */
    uint32_t max_batch_packets;             /* ingest batch capacity (1 Mi)              */
    uint64_t max_batch_bytes;               /* ingest blob capacity (1 GiB)              */
    uint32_t reflector_rtp_info_offset_msec; /* RTP-Info first packet: within over-buffer minus
                                               this (ReflectorStream.cpp:109-110); default 500,
                                               EDGPU_FALSE for an offset of 0 */
    /* Ring growth (default on; EDGPU_FALSE: the rings keep their configured capacities).  The
     * reference keeps every packet younger than 10 x reflector_buffer_size_sec, the key packet
     * and everything after it, and whatever a blocked output still needs, in an unbounded queue
     * (RemoveOldPackets, ReflectorStream.cpp:1233-1289, 112-114).  Each fan-out's plan measures
     * that span per sender; a sender whose span passes half of either of its rings has that ring
     * doubled (powers of two, up to the bounds below) before the next edgpu_ingest, its packets
     * moved over.  The request is noticed when the host reads the tick (edgpu_tick_stats_get /
     * edgpu_fanout_next), as every tick driver does. */
    uint32_t ring_growth;
    uint32_t max_ring_packets;              /* per sender bound of growth (1 Mi), power of two */
    uint64_t max_ring_bytes;                /* per sender bound of growth (1 GiB), power of two */
    /* reflector_use_in_packet_receive_time (default false; read once, ReflectorStream.cpp:103-104):
     * a packet longer than 12 bytes whose last 12 are "aktt" + a BE64 receive time (ms) loses
     * them, and its arrival (fTimeArrived: the new-output window, retention, relocation, transmit
     * times) becomes the socket's anchor arrival plus the receive time's offset from the anchor's
     * receive time; the anchor is the socket's first tagged packet since its SSRC -- by the
     * remote port's parity, EDGPU_PKT_REMOTE_ODD -- last changed (ReflectorSocket::ProcessPacket,
     * :1960-1994).  Arrivals further than reflector_in_packet_max_receive_sec (default 60,
     * EDGPU_FALSE for 0; :106-107, 113) ahead of the push time are clamped there. */
    uint32_t reflector_use_in_packet_receive_time;
    uint32_t reflector_in_packet_max_receive_sec;
    /* GPU watchdog (default 10000 ms; EDGPU_FALSE: unbounded): the longest any call waits for the
     * device.  A wait that runs out returns EDGPU_TIMEOUT and wedges the context: every call that
     * would enqueue work or wait returns EDGPU_TIMEOUT at once, enqueueing nothing, until the work
     * it timed out on has finished; then the context is usable again (the results of that work were
     * never read: the host re-runs or drops the tick).  edgpu_ctx_destroy waits without a bound. */
    uint32_t watchdog_ms;
    /* k_ingest's speculative copy (no reference counterpart; output bytes are the same either
     * way): a descriptor batch whose segments average at least this many packets is copied first
     * and its header words read from the copy (default 128, a 1-s C2 tick; 1: always; EDGPU_FALSE:
     * never, the header-first order).  DESIGN.md §3. */
    uint32_t ingest_spec_min;
} edgpu_config;
#define EDGPU_FALSE 0xFFFFFFFFu   /* a flag off / a value of 0 where 0 would select the default */

/* One ingested packet.  The batch blob is a sequence of 16-byte-aligned slots; a packet's
 * bytes start 4 bytes into its slot (the 4 bytes before it are the RTSP-interleaved header
 * slot the engine rewrites), so `slot` is the slot's offset / 16.  Packets of one session
 * must be contiguous and in arrival order (a pusher's TCP connection delivers exactly that);
 * `seg_offsets` (n_segments + 1 entries) splits the descriptor array into per-session
 * segments and `seg_session` names each segment's session.  A session appears in at most
 * one segment per batch. */
typedef struct edgpu_pkt_desc {
    uint32_t slot;          /* blob byte offset / 16 */
    uint16_t len;           /* packet length as received (clamped to 2060 at ingest, Q11) */
    uint8_t  channel;       /* interleaved channel: 2*track + is_rtcp */
    uint8_t  flags;         /* EDGPU_PKT_REMOTE_ODD or 0 */
    int64_t  arrival_ms;    /* OS::Milliseconds() when the packet was pushed */
} edgpu_pkt_desc;
/* A UDP push datagram from an odd source port: ProcessPacket's GetSSRC(theRemotePort & 1) reads
 * the RTCP SSRC word for it (ReflectorStream.cpp:1969; only the receive-time trailer reads it).
 * An RTSP-interleaved push has remote port 0 (PushPacket, :548, :572). */
#define EDGPU_PKT_REMOTE_ODD 1u

/* One send-ready output packet (16 bytes).  `offset` is the byte offset in the output
 * arena of the bytes to put on the wire: the UDP datagram, or the '$' ch BE16(len) frame
 * for an RTSP-interleaved subscriber. */
typedef struct edgpu_out_desc {
    uint64_t offset;
    uint32_t len;
    uint32_t packet_id;     /* low 32 bits of fStreamCountID */
} edgpu_out_desc;

/* One sub-stream (subscriber x track x RTP|RTCP) of a fan-out tick.  The table is in the
 * engine's sub-stream row order: a subscriber's rows are consecutive, in track, kind order, and
 * subscribers follow their join order, except that a subscriber may take the rows a removed
 * one left (edgpu_session_remove).  Rows of removed subscribers have desc_count 0.  Its
 * packets are desc[desc_base .. desc_base + desc_count). */
typedef struct edgpu_substream_out {
    uint32_t subscriber;    /* handle from edgpu_subscriber_add */
    uint16_t track;
    uint8_t  kind;          /* 0 RTP, 1 RTCP */
    uint8_t  transport;     /* EDGPU_TRANSPORT_* */
    uint32_t desc_base;
    uint32_t desc_count;
    uint64_t out_base;      /* arena offset of the first slot */
    uint64_t out_bytes;     /* arena bytes spanned (slot-padded) */
    uint32_t sender;        /* the engine sender (track x RTP|RTCP of a session) it relays */
    uint32_t flags;         /* EDGPU_SUB_IDENTITY: its bytes are the sender's packets unmodified
                               (UDP, no rewrite) -- two such sub-streams of one sender carry the
                               same bytes, the shorter one a suffix of the longer.
                               EDGPU_SUB_NEW: the output had no bookmark on this sender when the
                               tick began (GetBookMarkedPacket == NULL: ReflectPackets takes the
                               new-output start and sets `firstPacket`, ReflectorStream.cpp:
                               1097-1104) */
} edgpu_substream_out;
#define EDGPU_SUB_IDENTITY 1u
#define EDGPU_SUB_NEW      2u

/* Result of edgpu_fanout.  Device pointers, valid until the next edgpu_fanout.  Ticks run in
 * order on one stream: a tick's fan-out reads the rings after its own ingest and before the
 * next one (the engine had a pipelined mode that overlapped the next ingest with the fan-out;
 * it was dropped because backpressure reports and arrivals of the overlapped batch arrived a
 * tick late -- the pushers' H2D copies still overlap through edgpu_ingest_host). */
typedef struct edgpu_fanout_result {
    const uint8_t*              arena;          /* device */
    const edgpu_out_desc*       desc;           /* device */
    const edgpu_substream_out*  substreams;     /* device */
    uint32_t                    n_substreams;
} edgpu_fanout_result;

/* Per-tick totals, read back by edgpu_tick_stats_get (which syncs). */
typedef struct edgpu_tick_stats {
    uint64_t relayed_packets;   /* IncrementTotalPackets semantics (RTPStream.cpp:1213-1216) */
    uint64_t relayed_bytes;     /* wire bytes incl. '$' framing (of the passes copied so far) */
    uint64_t arena_bytes;       /* slot bytes of the whole tick (every pass) */
    uint64_t ingested_packets;  /* the batch the last edgpu_keyframe_index indexed (the counters
                                   move at the index, not at edgpu_ingest) */
    uint64_t ingested_bytes;
    int32_t  status;            /* device-side error of the whole tick (EDGPU_OUT_OVERFLOW, ...); a
                                   ring that lost a packet one session needed marks that session
                                   instead (stream_errors) */
    uint32_t _pad;
    /* the current copy pass (edgpu_fanout_next): arena bytes and descriptors the result's
     * sub-streams span, its ordinal (0 = the pass edgpu_fanout launched) and whether another
     * pass follows */
    uint64_t pass_arena_bytes;
    uint32_t pass_packets;
    uint32_t pass;
    uint32_t more_passes;
    /* sessions the tick newly marked with a stream error (edgpu_stream_errors): their outputs
     * lost packets, every other session's went out as usual */
    uint32_t stream_errors;
} edgpu_tick_stats;

typedef struct edgpu_ctx edgpu_ctx;

const char* edgpu_version(void);
const char* edgpu_last_error(void);
void        edgpu_config_default(edgpu_config* cfg);

int  edgpu_ctx_create(const edgpu_config* cfg, edgpu_ctx** out);
int  edgpu_ctx_destroy(edgpu_ctx* ctx);
int  edgpu_sync(edgpu_ctx* ctx);

/* Push sessions.  `udp_push` = 0 for an RTSP-interleaved (TCP) push, 1 for UDP push
 * (then the RTCP socket is bound on an odd port and only SRs are accepted, Q12/Q14). */
int  edgpu_session_add(edgpu_ctx* ctx, const char* sdp, uint32_t sdp_len, int udp_push,
                       uint32_t* out_session);
int  edgpu_session_tracks(edgpu_ctx* ctx, uint32_t session, uint32_t* out_tracks);
/* The session's SSRC filter settings: SetupReflectorSession takes use_one_SSRC_per_stream and
 * timeout_stream_SSRC_secs per session, from the module prefs as they are when the session is set
 * up (QTSSReflectorModule.cpp:1457, RereadPrefs :478-481 -> FilterInvalidSSRCs,
 * ReflectorStream.cpp:1732-1767).  edgpu_session_add gives a session the context's
 * edgpu_config values; this changes them (before its first packet, for a session a module set up
 * after a RereadPrefs).  Both are taken as given (a timeout of 0 s is the reference's too). */
int  edgpu_session_ssrc_prefs(edgpu_ctx* ctx, uint32_t session, uint32_t use_one_SSRC_per_stream,
                              uint32_t timeout_stream_SSRC_secs);

/* Destroys a push session -- what the reference does when a ReflectorSession's reference
 * count reaches 0 (its pusher gone, every output removed: RemoveOutput, QTSSReflectorModule.cpp:
 * 2133-2196).  The reference counting itself is the host's (the module's session map): the
 * engine keeps a session, its queues, packet ids, key pointers and SSRC latch, for as long as
 * the host does -- a pusher that reconnects to a session its players kept alive continues it
 * (FindOrCreateSession, :1479-1536), a pusher after edgpu_session_remove gets a fresh one from
 * edgpu_session_add (ids from 1, unlatched SSRC filter, empty queues).
 * flags: EDGPU_SESSION_KILL_OUTPUTS removes the session's subscribers with it
 * (kill_clients_when_broadcast_stops: TearDownAllOutputs, :2156-2159; their handles become
 * invalid); without it the call fails with EDGPU_ERR while a subscriber is attached.
 * Frees the session's HBM rings.  The session id, and its sender / stream table rows, are
 * reused by a later edgpu_session_add of a session with as many tracks; a removed subscriber's
 * sub-stream rows are reused by a later subscriber of a session with as many tracks
 * (subscriber handles are never reused).  Fails while an ingest is pending a keyframe index.
 * Syncs (a fan-out copy in flight may still read the rings). */
#define EDGPU_SESSION_KILL_OUTPUTS 1u
int  edgpu_session_remove(edgpu_ctx* ctx, uint32_t session, uint32_t flags);

/* The SDP parse edgpu_session_add applies (host only, no context, no GPU): the restatement of
 * SDPSourceInfo::Parse (APICommonCode/SDPSourceInfo.cpp:172-420) -- one track per line
 * starting with 'm', its payload type (1 video, 2 audio, 0 other), its rtpmap payload name
 * (the text the H.264 keyframe gate compares, ReflectorStream.cpp:1879, Q3) and its trackID
 * (a=control, else its position).  Names longer than 244 bytes are truncated here (not in the
 * session).  *n_tracks receives the count; EDGPU_BAD_ARGUMENT if it exceeds `cap`. */
typedef struct edgpu_sdp_track {
    uint32_t payload_type;
    uint32_t track_id;
    uint32_t name_len;
    char     name[244];
} edgpu_sdp_track;
int  edgpu_sdp_parse(const char* sdp, uint32_t sdp_len, edgpu_sdp_track* out, uint32_t cap, uint32_t* n_tracks);

/* Subscribers: a join takes effect at the next edgpu_fanout, like a new output being
 * picked up by the next ReflectPackets. */
int  edgpu_subscriber_add(edgpu_ctx* ctx, uint32_t session, int transport,
                          uint32_t* out_handle);
int  edgpu_subscriber_remove(edgpu_ctx* ctx, uint32_t handle);
/* The subscriber's place in its session's bucket arrays, as ReflectorStream::AddOutput /
 * FindBucket give it (ReflectorStream.cpp:281-334: the first empty place, 16 per bucket, a
 * removed output's place reused): its writes' transmit times are bucket x
 * reflector_bucket_offset_delay_msec early (ReflectorStream.cpp:1107, RTPSessionOutput.cpp:
 * 603-608), and a new output's first write decides for every output after it in this order
 * (ReflectorStream.cpp:1088-1104).  Used by the egress's write gate (edgpu_egress_pacing). */
int  edgpu_subscriber_slot(edgpu_ctx* ctx, uint32_t handle, int32_t* out_slot);
/* A burst of joins (e.g. BASELINE config C4's 10k mid-GOP joins) in one call: subscriber i
 * joins sessions[i] with transports[i]; handles as edgpu_subscriber_add would return them. */
int  edgpu_subscribers_add(edgpu_ctx* ctx, uint32_t n, const uint32_t* sessions,
                           const int32_t* transports, uint32_t* out_handles);

/* PLAY of a player that needs RTP-Info (DoPlay's rtpInfoEnabled branch,
 * QTSSReflectorModule.cpp:1867-2023: the kRequiresRTPInfoSeqAndTime player profile, user
 * agents "Android" and "vlc").  For every track, HaveStreamBuffers (:1804-1865) needs a
 * received RTP packet (HasFirstRTP) and a first packet no older than reflector_buffer_size
 * minus reflector_rtp_info_offset_msec at `now_ms` (ReflectorSender::GetFirstPacketInfo,
 * ReflectorStream.cpp:728-753).  Its sequence number and RTP timestamp go to out_info[track]
 * (the PLAY response's RTP-Info), and until the player's first write on a track, RTP packets
 * with a lower sequence number are not sent to it (FilterPacket, RTPSessionOutput.cpp:249-280;
 * a plain 16-bit compare).  If a track has nothing buffered, no subscriber is added and
 * EDGPU_WOULD_BLOCK is returned: the reference retries the PLAY from a 100 ms idle timer
 * (:1985-2003).  Ingested packets must be indexed (edgpu_keyframe_index) first.
 * flags: 0 (then this is edgpu_subscriber_add) or EDGPU_PLAY_RTP_INFO. */
#define EDGPU_PLAY_RTP_INFO 1u
typedef struct edgpu_rtp_info {
    uint16_t seq;           /* qtssRTPStrFirstSeqNumber */
    uint16_t _pad;
    uint32_t rtptime;       /* qtssRTPStrFirstTimestamp */
} edgpu_rtp_info;
int  edgpu_subscriber_play(edgpu_ctx* ctx, uint32_t session, int transport, uint32_t flags,
                           int64_t now_ms, uint32_t* out_handle, edgpu_rtp_info* out_info);

/* Per-output rewrite stage (north_star item 3).  From the next edgpu_fanout, every packet
 * written to subscriber `handle`'s track `track` is rewritten in flight:
 *   RTP sub-stream:  sequence number += seq_delta (mod 2^16), timestamp += ts_delta (mod 2^32),
 *                    SSRC = ssrc when flags has EDGPU_REWRITE_SSRC -- for packets of >= 12 bytes;
 *   RTCP sub-stream: sender SSRC (bytes 4-7) = ssrc with EDGPU_REWRITE_SSRC (>= 8 bytes), and the
 *                    RTP timestamp of a sender report (PT 200, bytes 16-19) += ts_delta (>= 20 B).
 * CSRC lists, extensions and payloads are never touched; lengths and descriptors are unchanged.
 * NULL (or all-zero deltas without EDGPU_REWRITE_SSRC) is the identity, the default.  The
 * reference never rewrites (Q1: RTPSessionOutput::PacketShouldBeThinned returns false at
 * RTPSessionOutput.cpp:685-687, and the RTCP rewrite RewriteRTCP / TrackRTCPPackets,
 * :403-561, is not called, :600-601), so parity runs use the identity; FilterPacket's first-seq
 * test and an RTP-Info PLAY's reply see the source's sequence numbers (a host that rewrites an
 * RTP-Info player's stream adjusts its RTP-Info header by the same deltas). */
#define EDGPU_REWRITE_SSRC 1u
typedef struct edgpu_rewrite {
    uint16_t seq_delta;
    uint16_t flags;
    uint32_t ts_delta;
    uint32_t ssrc;          /* host order */
} edgpu_rewrite;
int  edgpu_subscriber_rewrite(edgpu_ctx* ctx, uint32_t handle, uint32_t track, const edgpu_rewrite* rw);

int  edgpu_ingest(edgpu_ctx* ctx, const edgpu_pkt_desc* desc, uint32_t n_packets,
                  const uint32_t* seg_offsets, const uint32_t* seg_session,
                  uint32_t n_segments, const uint8_t* blob, uint64_t blob_bytes,
                  int ptr_location);

/* Pinned host staging for edgpu_ingest (north_star: "C++ host code batches ingested RTP
 * packets ... into pinned HBM ring buffers"; replaces the per-packet memcpy into a
 * ReflectorPacket, ReflectorStream.h:104-114).  The host (its socket reader) writes a batch --
 * descriptors, segments and the slot blob -- straight into buffers from edgpu_host_alloc and
 * calls edgpu_ingest(..., EDGPU_PTR_PINNED): the batch is validated on the host, copied to one
 * of two device staging sets on a dedicated copy stream, and k_ingest waits for that copy on
 * the context stream -- so the PCIe transfer of batch t+1 overlaps the fan-out of batch t, and
 * the call returns without waiting for the GPU.  Buffer reuse: a pinned batch may be rewritten
 * once the NEXT ingest call (edgpu_ingest of any pointer kind, or edgpu_ingest_interleaved), or
 * any call that synchronises the context (edgpu_sync, edgpu_tick_stats_get), has returned --
 * every ingest entry point waits for the previous pinned batch's copy, and the context stream
 * waits for it before its ingest kernel -- so two host batches used alternately never stall the
 * reader on the GPU.  edgpu_host_alloc / edgpu_host_free
 * may be called from any thread (a pusher growing its blob); a free waits for the copy stream. */
int  edgpu_host_alloc(edgpu_ctx* ctx, uint64_t bytes, void** out);
int  edgpu_host_free(edgpu_ctx* ctx, void* ptr);
/* Copies bytes [offset, offset + bytes) of the NEXT pinned batch's blob to the device ahead of
 * its edgpu_ingest(..., EDGPU_PTR_PINNED), on the copy stream, while the host is still filling
 * the rest: a host whose pushers write the blob in slabs streams each finished prefix (the
 * QTSS module drop-in does, reflector_adapter.cpp), and the ingest call then copies only the
 * remainder.  Ranges must extend the prefix staged so far (offset == bytes already staged) and
 * those bytes must not change before the ingest (a blob moved to a larger buffer keeps them).
 * May be called from another thread than the context's other calls.  A pinned batch that
 * edgpu_ingest refuses for its size or structure drops what was copied ahead of it; offset 0 with
 * bytes 0 drops it explicitly (a host whose batch came to nothing, e.g. every packet of it belonged
 * to a session removed since: the next pinned batch is then copied whole). */
int  edgpu_ingest_prestage(edgpu_ctx* ctx, const uint8_t* blob, uint64_t offset, uint64_t bytes);
/* RTSP-interleaved push ingest: the pusher connections' raw TCP reads, deframed on the GPU.
 * Replaces RTSPRequestStream::ReadRequest's '$' branch (Server.tproj/RTSPRequestStream.cpp:
 * 65-171, RTSPSession.cpp:240-262) and the per-frame hand-off to ProcessRTPData
 * (RTSPSession.cpp:2131-2178, QTSSReflectorModule.cpp:604-678): each connection's bytes are
 * split into '$' ch BE16(len) frames, frame i of a session becomes a packet on channel `ch`
 * (track ch/2, RTCP when odd) with the arrival time of the read that completed it, and the
 * packets are ingested exactly as edgpu_ingest would (same batch semantics; run
 * edgpu_keyframe_index next).  A frame split across calls is carried on the device (at most
 * 2046 bytes per session).
 *
 * reads[i] is one read of session reads[i].session (an RTSP-interleaved, udp_push = 0
 * session): `len` bytes at bytes + offset.  A session's reads are consecutive entries of
 * `reads`, in arrival order, and contiguous in `bytes`.  `bytes` is host memory
 * (EDGPU_PTR_HOST, staged) or device memory on the ctx GPU (EDGPU_PTR_DEVICE, 16-B aligned).
 *
 * results[i] (host memory) reports read i: `frames` it completed, `consumed` bytes the engine
 * took (framed or carried), and `status`:
 *   EDGPU_TCP_MESSAGE  a non-'$' byte at a frame boundary: an RTSP request (e.g. a
 *                      SET_PARAMETER keep-alive or TEARDOWN) starts at byte `consumed` of this
 *                      read; the rest of this read and the session's later reads in this call
 *                      are the host RTSP stack's.  The session's carry is cleared.
 *   EDGPU_TCP_DROPPED  a frame longer than the 2047-byte request buffer: the reference asks the
 *                      socket for 0 bytes and treats the connection as closed (Socket.cpp:
 *                      383-388); set on the read that fills the buffer and later reads.
 * `carry` is the session's carried byte count after the call.  Returns EDGPU_OUT_OVERFLOW
 * (nothing ingested, no carry changed) when the frames exceed max_batch_packets.  Host reads
 * are staged in a max_batch_bytes buffer; device reads are read in place (the frames are
 * copied from them into the sender rings).  Returns once the frames are found and `results`
 * written, which is before the copy into the rings has run (it is stream-ordered before the
 * context's next work): device `bytes`, like every EDGPU_PTR_DEVICE pointer, stay valid until
 * edgpu_sync (or a synchronising call) returns; host `bytes` are consumed on return. */
#define EDGPU_TCP_MESSAGE  1
#define EDGPU_TCP_DROPPED  2
typedef struct edgpu_tcp_read {
    uint32_t session;
    uint32_t len;
    uint64_t offset;        /* byte offset of the read in `bytes` */
    int64_t  arrival_ms;    /* OS::Milliseconds() when the read returned */
} edgpu_tcp_read;
typedef struct edgpu_tcp_result {
    uint32_t frames;
    uint32_t consumed;
    int32_t  status;        /* 0, EDGPU_TCP_MESSAGE or EDGPU_TCP_DROPPED */
    uint32_t carry;
} edgpu_tcp_result;
int  edgpu_ingest_interleaved(edgpu_ctx* ctx, const edgpu_tcp_read* reads, uint32_t n_reads,
                              const uint8_t* bytes, uint64_t n_bytes, int ptr_location,
                              edgpu_tcp_result* results);

/* Closes the ingested batch (the keyframe index itself runs inside the ingest kernel, after each
 * segment's packets are enqueued); required between an ingest and the next call. */
int  edgpu_keyframe_index(edgpu_ctx* ctx);
int  edgpu_fanout(edgpu_ctx* ctx, int64_t now_ms, edgpu_fanout_result* out);

/* Over-capacity ticks.  A tick whose outputs exceed out_arena_bytes or max_out_packets is not
 * dropped: it is delivered in copy passes over consecutive rows of the sub-stream table, each
 * within the arena and the descriptor array (the reference walks every output of every sender in
 * each ReflectPackets, ReflectorStream.cpp:1088-1120, so no output may lose a tick).  edgpu_fanout
 * launches pass 0; the result then shows only that pass's sub-streams (the other rows have
 * desc_count 0 and out_bytes 0; flags are set on every row), their out_base / desc_base relative to
 * the pass's arena and descriptors.  After consuming a pass the host calls edgpu_fanout_next:
 * *launched = 1 when it launched the next pass (`out` as above), 0 when the tick is complete.
 * edgpu_tick_stats_get reports the current pass (pass_arena_bytes, pass_packets, more_passes).
 * Every pass of a tick must be consumed before the next edgpu_fanout and edgpu_session_remove:
 * those fail with EDGPU_ERR while a pass is owed (session removal reads that from the device when
 * the host has not read the tick's stats; edgpu_counters.lost_passes counts passes a tick still
 * owed when the next tick was planned).  edgpu_ingest / edgpu_ingest_interleaved fail the same
 * way while the host knows of an owed pass; before it has read the stats an ingest may run, and a batch that would lap the tick's window in a ring while a pass is
 * owed fails the ring (EDGPU_RING_OVERFLOW) instead of corrupting the pass.  Subscribers may come and go between passes: the passes keep the tick's table (rows
 * added since are not in it, rows of removed subscribers still deliver the tick, and their rows
 * are reused only from the next tick).  Backpressure reports (edgpu_fanout_blocked) take
 * tick-wide sub-stream rows and may follow any pass.  A tick fits one pass whenever its bytes and descriptors do; a single
 * sub-stream larger than the arena (out_arena_bytes below a sender ring) still fails the tick
 * with EDGPU_OUT_OVERFLOW. */
int  edgpu_fanout_next(edgpu_ctx* ctx, edgpu_fanout_result* out, uint32_t* launched);

/* Egress backpressure.  The host writes a tick's sub-streams to their sockets; when a socket
 * stops accepting (EAGAIN -> QTSS_WouldBlock, RTPStream::Write -> RTPSessionOutput::
 * WritePacket, RTPSessionOutput.cpp:600-615) after `sent` of the sub-stream's desc_count
 * packets, report it here, after edgpu_fanout and before the next edgpu_ingest.  The engine
 * then keeps the state ReflectorSender::SendPacketsToOutput leaves for a blocked output
 * (ReflectorStream.cpp:1138-1198): the bookmark is the blocked packet -- moved to the key
 * frame when it is older than rtp_reflector_threshold_msec and the key frame is newer
 * (NeedRelocateBookMark, :1293-1322, Q9; the session's video-key flag is set, so the next
 * audio packet becomes the audio anchor) -- the last-sent packet id is the last packet
 * written, and the next edgpu_fanout resumes at the bookmark.  The tick's relayed counters
 * drop the unsent packets.  `substream` indexes the tick's edgpu_substream_out table.
 * Reports with sent >= desc_count are no-ops. */
typedef struct edgpu_blocked {
    uint32_t substream;
    uint32_t sent;
} edgpu_blocked;
int  edgpu_fanout_blocked(edgpu_ctx* ctx, const edgpu_blocked* reports, uint32_t n);

/* ---- UDP pushers: source addresses and receiver reports ----
 * A UDP push session (edgpu_session_add udp_push=1) receives datagrams on a bound even/odd
 * port pair; the host's socket reader passes the packets to edgpu_ingest (channel =
 * 2*track + 1 for the odd, RTCP port) and, in the same arrival order, their source
 * addresses here -- ReflectorSocket::ProcessPacket's remote address (ReflectorStream.cpp:
 * 1769-1866).  The engine keeps each track's pusher RTCP address as the reference does
 * with NAT_WORKAROUND (ReflectorStream.h:63, .cpp:1843-1855): set by the first datagram,
 * moved by every RTCP-port datagram that passes the SR-only gate (RTCPPacket::ParsePacket
 * + type 200, Q14), an even RTP source port followed by +1.  Datagrams from address 0,
 * empty ones and tracks out of range change nothing.  `head` = the datagram's first 4
 * bytes (what the SR gate reads with `len`).  Only RTCP datagrams and a track's first RTP
 * datagram can change the address, so a reader may pass just those.
 * Replaces: the fDestRTCPAddr/fDestRTCPPort update inside ReflectorSocket::ProcessPacket. */
typedef struct edgpu_udp_source {
    uint32_t session;
    uint8_t  channel;
    uint8_t  _pad;
    uint16_t port;        /* host order */
    uint32_t addr;        /* IPv4, host order */
    uint32_t len;
    uint8_t  head[4];
} edgpu_udp_source;
int  edgpu_udp_sources(edgpu_ctx* ctx, const edgpu_udp_source* src, uint32_t n);

/* Receiver reports to UDP pushers.  Every edgpu_fanout(now) runs, for each track, the RTCP
 * sender's report timer (ReflectorSender::ReflectPackets, ReflectorStream.cpp:1039-1047):
 * when now > last + kRRInterval (5000 ms) the timer restarts at now and, if the pusher's
 * RTCP address is known, one report is queued -- ReflectorStream::SendReceiverReport
 * (:510-527): RR (header + SSRC), SDES CNAME, and the 'QTSS' APP packet carrying the eye
 * count (client subscribers of the session, ReflectorSession.cpp:215-268) twice, built as
 * the ReflectorStream constructor lays it out (:164-201).  edgpu_source_reports returns the
 * reports queued by the last edgpu_fanout (session then track order) for the host to send
 * from the track's RTCP socket to (addr, port).
 * Identity: the reference draws the report SSRC from rand() and the CNAME from
 * OS::Milliseconds()/1000 when the stream is created (RTCPSRPacket.cpp:87-117); the engine
 * does the same at edgpu_session_add, and edgpu_source_identity overrides both. */
#define EDGPU_RR_MAX 96
typedef struct edgpu_source_report {
    uint32_t session;
    uint16_t track;
    uint16_t port;        /* host order */
    uint32_t addr;        /* IPv4, host order */
    uint32_t len;
    uint8_t  bytes[EDGPU_RR_MAX];
} edgpu_source_report;
int  edgpu_source_reports(edgpu_ctx* ctx, edgpu_source_report* out, uint32_t cap, uint32_t* n_out);
int  edgpu_source_identity(edgpu_ctx* ctx, uint32_t session, uint32_t track, uint32_t ssrc,
                           int64_t cname_secs);
/* Subscribers of `session` served by other contexts (replica sessions on other GPUs, §8.e):
 * the owner's eye count is its own clients plus these, as the single reference process
 * counts every output (IncEyeCount / DecEyeCount).  `delta` is +1 per remote join, -1 per
 * remote leave. */
int  edgpu_session_eyes_add(edgpu_ctx* ctx, uint32_t session, int32_t delta);
/* The same for a remote subscriber that also takes its place in the owner's bucket arrays
 * (ReflectorStream::AddOutput / RemoveOutput, ReflectorStream.cpp:281-336: the first empty place,
 * 16 a bucket), so that the owner's and its replicas' subscribers of one session are numbered
 * in one array, as the reference numbers them in one process: a subscriber past the first
 * bucket then gets the reference's bucket lateness in its transmit times on whichever GPU serves
 * it.  edgpu_session_remote_join counts the eye and returns the place; the replica passes it to
 * edgpu_subscriber_set_slot for its subscriber.  edgpu_session_remote_leave frees it. */
int  edgpu_session_remote_join(edgpu_ctx* ctx, uint32_t session, int32_t* out_place);
int  edgpu_session_remote_leave(edgpu_ctx* ctx, uint32_t session, int32_t place);
/* Moves a subscriber to bucket place `slot` of its session (a replica session's subscriber takes
 * the place its owner gave it, edgpu_session_remote_join).  Fails if another output holds it. */
int  edgpu_subscriber_set_slot(edgpu_ctx* ctx, uint32_t handle, int32_t slot);

/* ---- Socket egress (host side) ----
 * Sends a fan-out tick to the subscribers' sockets as RTPStream::Write does
 * (Server.tproj/RTPStream.cpp:1084-1147): UDP datagrams through the sub-stream's RTP / RTCP
 * socket with send errors ignored (a full socket drops the datagram, as the reference's
 * (void)SendTo); RTSP-interleaved frames on the subscriber's RTSP connection with
 * RTSPResponseStream::WriteV(kAllOrNothing) semantics (RTSPResponseStream.cpp:36-140: a frame
 * that goes out in part counts as sent and its tail is buffered; a frame that gets no byte
 * blocks).  Blocked TCP sub-streams are reported with edgpu_fanout_blocked before returning.
 * The tick's distinct bytes come over PCIe in one copy (identity UDP sub-streams of a sender share
 * one region, edgpu_arena_gather), with the descriptors and sub-stream table; `threads` workers
 * own disjoint subscribers and send with sendmmsg / sendmsg.  An over-capacity tick is sent pass
 * by pass (the call runs edgpu_fanout_next itself), so `r` is the result of edgpu_fanout.
 *
 * UDP loss granularity.  By default (EDGPU_EGRESS_GSO unset or 1) runs of equal-length
 * datagrams of a sub-stream (FU-A fragments of a frame) leave as UDP GSO messages (UDP_SEGMENT,
 * up to 64 datagrams / 64 KiB each): the wire carries exactly the datagrams the reference
 * sends, but a send the socket refuses (EAGAIN / ENOBUFS) drops the whole message, where the
 * reference's per-packet (void)SendTo drops one datagram (RTPStream.cpp:1145).  What arrives is
 * always an in-order subset of the tick's datagrams per sub-stream (no reordering, no
 * duplicates; tests/test_gpu_egress.py).  EDGPU_EGRESS_GSO=0 is the reference-exact mode: one
 * datagram per message, one datagram lost per refused send. */
typedef struct edgpu_egress edgpu_egress;
typedef struct edgpu_egress_stats {
    uint64_t udp_datagrams, udp_bytes;
    uint64_t udp_dropped;       /* SendTo failures, ignored like the reference */
    uint64_t tcp_frames, tcp_bytes;
    uint32_t blocked_substreams;
    uint32_t _pad;
    double   copy_ms, send_ms;  /* device -> pinned host copy; socket writes */
    uint64_t copied_bytes;      /* bytes brought over PCIe for this tick */
    uint64_t stale_dropped;     /* paced subscribers: stale TCP non-video RTP packets dropped (Q20) */
} edgpu_egress_stats;
int  edgpu_egress_create(edgpu_ctx* ctx, uint32_t threads, edgpu_egress** out);
int  edgpu_egress_destroy(edgpu_egress* eg);
const char* edgpu_egress_last_error(edgpu_egress* eg);
/* UDP subscriber track: datagrams leave through rtp_fd / rtcp_fd (-1: a per-worker socket) to
 * ipv4:port (network byte order, as in sockaddr_in). */
int  edgpu_egress_udp(edgpu_egress* eg, uint32_t subscriber, uint32_t track, int rtp_fd, int rtcp_fd,
                      uint32_t ipv4_be, uint16_t rtp_port_be, uint16_t rtcp_port_be);
/* RTSP-interleaved subscriber: its (non-blocking) RTSP connection. */
int  edgpu_egress_tcp(edgpu_egress* eg, uint32_t subscriber, int fd);
int  edgpu_egress_send(edgpu_egress* eg, const edgpu_fanout_result* r, edgpu_egress_stats* out);
/* The (sub-stream, sent) backpressure reports of the last edgpu_egress_send (*n = count). */
int  edgpu_egress_blocked(edgpu_egress* eg, edgpu_blocked* out, uint32_t cap, uint32_t* n);
/* Writes buffered TCP tails that fit now; *pending = bytes still buffered. */
int  edgpu_egress_flush(edgpu_egress* eg, uint64_t* pending);
/* Subscribers whose RTSP connection failed with an error other than EAGAIN since the last
 * call (reset / closed peer): their frames are no longer written (the reference counts such a
 * write as done, RTPSessionOutput.cpp:612-653); the host tears the session down
 * (ClientSessionClosing -> edgpu_subscriber_remove).  Sockets are written with MSG_NOSIGNAL. */
int  edgpu_egress_disconnected(edgpu_egress* eg, uint32_t* out, uint32_t cap, uint32_t* n);

/* ---- The server's write gate (Q20): over-buffer window and TCP-audio thinning ----
 * Behind the reference module, each relayed packet goes through the server's RTPStream::Write
 * (Server.tproj/RTPStream.cpp:1048-1147) with the transmit time RTPSessionOutput::WritePacket gave
 * it (RTPSessionOutput.cpp:603-608: now - bucket lateness, + the output's buffer delay left for the
 * packet).  There the session's over-buffer window (RTPOverbufferWindow::CheckTransmitTime) holds a
 * packet whose time has not come -- QTSS_WouldBlock: the output stops for this reflect, and on a new
 * output's first pass the packet's age becomes its buffer delay (RTPSessionOutput.cpp:612-622) --
 * and RTPStream::UpdateQualityLevel (:936-1045) drops RTP packets of a TCP non-video stream that have
 * fallen more than drop_all_packets_delay behind.  With pacing on for a subscriber the egress does
 * the same before its socket writes: held packets are reported to the engine like a blocked socket
 * (edgpu_fanout_blocked), dropped ones count as written.  It needs each packet's arrival (so serial
 * ticks: edgpu_fanout_arrivals) and the tick's clock (edgpu_egress_clock), the subscriber's bucket
 * place comes from the engine (edgpu_subscriber_slot). */
#define EDGPU_PACE_OVERBUFFER 1u   /* the client asked for dynamic rate (x-dynamic-rate: 1): the
                                      reflector otherwise turns overbuffering off, QRM:1772-1777 */
typedef struct edgpu_pacing {
    int64_t  play_time_ms;         /* the PLAY's time (RTPSession::fPlayTime): packets due before it
                                      are never thinned (RTPStream.cpp:941-942) */
    uint32_t video_tracks;         /* bit t: track t is video (never thinned, :946-948) */
    uint32_t flags;                /* EDGPU_PACE_* */
} edgpu_pacing;
/* Server and reflector prefs the gate reads; edgpu_egress_create sets the reference defaults
 * (QTSServerPrefs.cpp: send_interval 50, max_send_ahead_time 25, overbuffer_rate 2.0,
 * drop_all_packets_delay 2500, thin_all_the_way_delay 1500, start_thinning_delay 0; the late
 * tolerance's 1.5-s default adjusts none, RTPStream.cpp:897-918; the reflector's bucket offset
 * delay 73 ms, 16 outputs a bucket, buffer 1000 ms, ReflectorStream.cpp:53-117). */
typedef struct edgpu_pacing_config {
    int64_t  bucket_delay_ms;      /* reflector_bucket_offset_delay_msec */
    int64_t  over_buffer_ms;       /* reflector_buffer_size_sec x 1000: a new output's buffer delay */
    int64_t  drop_all_packets_ms, thin_all_the_way_ms, start_thinning_ms;
    uint32_t bucket_size;          /* outputs per bucket (16) */
    uint32_t send_interval_ms, max_send_ahead_s;
    float    overbuffer_rate;
} edgpu_pacing_config;
/* (A subscriber's over-buffer window takes send_interval_ms, max_send_ahead_s, overbuffer_rate and
 * over_buffer_ms when edgpu_egress_pacing turns its gate on, as an RTPSession builds its window at
 * SETUP; the other fields apply at every send.) */
int  edgpu_egress_pacing_config(edgpu_egress* eg, const edgpu_pacing_config* cfg);
/* Turns the gate on for `subscriber` (NULL: off).  Call after its edgpu_egress_udp / _tcp. */
int  edgpu_egress_pacing(edgpu_egress* eg, uint32_t subscriber, const edgpu_pacing* p);
/* The tick's clock (OS::Milliseconds at the reflect), for the next edgpu_egress_send. */
int  edgpu_egress_clock(edgpu_egress* eg, int64_t now_ms);
/* Why each sub-stream of the last edgpu_egress_send stopped: `sent` descriptors went (written,
 * or dropped as stale), `written` of them reached the socket; cause 0 = the socket would block,
 * 1 = the write gate held the next packet. */
typedef struct edgpu_egress_block {
    uint32_t substream, sent, written, cause;
} edgpu_egress_block;
int  edgpu_egress_block_info(edgpu_egress* eg, edgpu_egress_block* out, uint32_t cap, uint32_t* n);

/* Per-stream error isolation (a bad stream marks that stream, not the batch).  A
 * sender ring too small for what a session's outputs still need -- a blocked output's bookmark
 * or a new output's key frame overwritten by newer packets (the reference's queue is unbounded,
 * ReflectorStream.cpp:1088-1120) -- marks the session; its outputs resume at the oldest packet
 * still held (a new output waits for the next tick), and every other session's tick is
 * unaffected.  Lists the marked live sessions (code EDGPU_RING_OVERFLOW) and clears the marks of
 * those returned; *n = how many are marked.  Syncs. */
int  edgpu_stream_errors(edgpu_ctx* ctx, uint32_t* sessions, int32_t* codes, uint32_t cap, uint32_t* n);

int  edgpu_tick_stats_get(edgpu_ctx* ctx, edgpu_tick_stats* out);   /* syncs; EDGPU_ERR while an
                                                                       ingest awaits its index */

/* The arrival time (fTimeArrived, OS::Milliseconds() at PushPacket) of each descriptor of
 * the current copy pass of the last edgpu_fanout: out[i] for desc[i], i < the pass's
 * pass_packets (serial ticks; call before the next edgpu_fanout / edgpu_fanout_next).
 * RTPSessionOutput::WritePacket derives the
 * QTSS_PacketStruct transmit time from it (RTPSessionOutput.cpp:604-608), which the server's
 * RTPStream::Write hands to its thinning and over-buffer logic (RTPStream.cpp:1062,1119-1137).
 * `out` is host memory (ptr_kind EDGPU_PTR_HOST) or device memory (EDGPU_PTR_DEVICE); `n`
 * must be at least the pass's descriptors. */
int  edgpu_fanout_arrivals(edgpu_ctx* ctx, int64_t* out, uint32_t n, int ptr_kind);
/* edgpu_fanout_arrivals and / or, per descriptor of the current pass, the blob slot (byte offset /
 * 16) of its packet in the batch of the LAST edgpu_ingest -- when that was a host batch
 * (EDGPU_PTR_PINNED or EDGPU_PTR_HOST) and the packet came with it -- else EDGPU_NO_SOURCE.  A host
 * that still holds that blob can read an identity UDP descriptor's bytes (the packet, `len` bytes)
 * at blob + slot * 16 + 4 instead of reading the arena back (the module adapter does); for other
 * sub-streams the arena's bytes differ (framing, rewrite).  Either output may be NULL; serial
 * ticks; syncs. */
#define EDGPU_NO_SOURCE 0xFFFFFFFFu
int  edgpu_fanout_packet_info(edgpu_ctx* ctx, int64_t* arrivals, uint32_t* sources, uint32_t n, int ptr_kind);

/* What a host write loop needs of one descriptor, in one row: the descriptor, its packet's
 * arrival (edgpu_fanout_arrivals) and batch slot (edgpu_fanout_packet_info's sources). */
typedef struct edgpu_packet_row {
    uint64_t offset;        /* edgpu_out_desc.offset */
    uint32_t len;           /* edgpu_out_desc.len */
    uint32_t packet_id;     /* edgpu_out_desc.packet_id */
    int64_t  arrival;       /* fTimeArrived */
    uint32_t source;        /* blob slot in the last host batch, or EDGPU_NO_SOURCE */
    uint32_t _pad;
} edgpu_packet_row;
/* The sub-streams of the current copy pass that carry descriptors or are new outputs
 * (EDGPU_SUB_NEW: a host deriving per-tick state from new outputs sees every one), compacted and
 * in table order:
 * rows[i] is row q[i] of the pass's sub-stream table (edgpu_fanout_result.substreams), i <
 * min(*n_out, cap); *n_out counts all of them.  A host delivering a tick reads back only what it
 * writes -- at 2-ms ticks a few % of a 32k-row table.  `rows` / `q`: device memory
 * (EDGPU_PTR_DEVICE) or host memory (EDGPU_PTR_HOST; pinned buffers from edgpu_host_alloc are
 * stored into by the kernel over PCIe, others through a device copy).  Syncs. */
int  edgpu_fanout_active(edgpu_ctx* ctx, edgpu_substream_out* rows, uint32_t* q, uint32_t cap, uint32_t* n_out,
                         int kind);
/* The rows of SELECTED sub-streams of the current copy pass only: sel[2k] is a row of the
 * sub-stream table, sel[2k + 1] where its rows start in `rows`: rows[sel[2k + 1] + i] for its
 * descriptor desc_base + i, i < desc_count (rows at or past `nrows` are not written).  Two
 * EDGPU_SUB_IDENTITY sub-streams of one sender share their packets (the shorter a suffix of the
 * longer), so a host reads one sender's rows once for all of them -- at C2 the module's
 * readback falls from 28 B per write to 32 B per relayed packet.  `sel` is host
 * memory; `rows` host (EDGPU_PTR_HOST) or device (EDGPU_PTR_DEVICE).  Serial ticks; syncs. */
int  edgpu_fanout_rows(edgpu_ctx* ctx, const uint32_t* sel, uint32_t nsel, edgpu_packet_row* rows, uint64_t nrows,
                       int ptr_kind);

/* Packs regions of a fan-out arena (16-B aligned offsets and lengths; in the order given)
 * back to back into `dst` on the context stream -- so a host egress brings only the distinct
 * bytes of a tick over PCIe instead of the whole write-many arena.  `dst` is device memory, or
 * pinned host memory from edgpu_host_alloc: the gather kernel then stores straight over PCIe
 * (one pass, ~53 GB/s on the MI355X box against ~29 GB/s for a DMA copy).
 * Synchronous: the bytes are in `dst` when the call returns. */
typedef struct edgpu_region {
    uint64_t offset;        /* arena byte offset, multiple of 16 */
    uint64_t bytes;         /* multiple of 16 */
} edgpu_region;
int  edgpu_arena_gather(edgpu_ctx* ctx, const edgpu_fanout_result* r, const edgpu_region* regions, uint32_t n,
                        void* dst, uint64_t dst_cap);

/* Name of the fan-out copy kernel of this context's last edgpu_fanout (before the first: the one
 * it would launch), for measurement reports.  There are two (every other variant and the
 * measurement build that carried them were removed; git commit 0dd0039 has their code).  Unless
 * EDGPU_FANOUT=0|1 pins one, a tick takes the
 * 32-packet-chunk kernel when any active sub-stream is RTSP-interleaved or rewrites (a per-output
 * patch) or when the outputs added since the last tick hold a quarter or more of its sub-stream
 * rows and at least 4096 of them (a join burst), else the 16-packet-chunk one; see DESIGN.md §3. */
const char* edgpu_fanout_kernel(edgpu_ctx* ctx);

/* Cumulative counters since context creation (syncs).  fanout_in_bytes counts the
 * ingested bytes the fan-out read (each referenced packet once per launch). */
typedef struct edgpu_counters {
    uint64_t relayed_packets;
    uint64_t relayed_bytes;
    uint64_t fanout_in_bytes;
    uint64_t fanout_launches;
    uint64_t ingested_packets;
    uint64_t ingested_bytes;
    uint64_t fanout_passes;     /* copy passes launched (> fanout_launches: over-capacity ticks) */
    uint64_t lost_passes;       /* passes a tick still owed when the next tick was planned */
    uint32_t senders;           /* sender rows (2 per track) and sub-stream rows of the tables: */
    uint32_t substream_rows;    /* removed sessions' / subscribers' rows are reused, best fit */
    uint64_t ring_grows;        /* sender rings grown so far (edgpu_config.ring_growth) */
    uint64_t ring_bytes;        /* device bytes of every live sender's two rings now */
    uint64_t ring_pool_bytes;   /* device bytes the ring pool holds now: live rings, rings on its free
                                   lists (reused by later sessions / growths) and unused chunk space */
    uint64_t ring_grow_failures; /* growths skipped because the device memory could not hold the new
                                    rings (growth is best effort; the ingest goes on) */
    uint64_t watchdog_timeouts; /* waits the GPU watchdog ended (edgpu_config.watchdog_ms) */
    uint64_t kernel_launches;   /* kernels the context's calls launched */
    uint64_t host_syncs;        /* times a call waited for the GPU (stream / event synchronize) */
} edgpu_counters;
int  edgpu_counters_get(edgpu_ctx* ctx, edgpu_counters* out);

/* ---- Per-stream reception statistics and the reference's per-stream bitrate ----
 * Opt-in per push session.  While at least one session of the context is enabled, every ingest
 * (edgpu_ingest of any pointer kind, edgpu_ingest_interleaved) is followed on the context stream
 * by one read-only kernel that walks, per enabled track, the packets enqueued since its last
 * launch; with no session enabled nothing is launched, recorded or copied.
 *
 * A "packet" is a queue entry with its final length: after the 2060-byte clamp (Q11), the SSRC
 * filter's zeroing (FilterInvalidSSRCs) and the receive-time trailer strip.  Entries of length 0
 * are skipped everywhere.
 *
 * RTP sender of a track: `packets` / `bytes` count every packet; one shorter than 12 bytes
 * counts in `short_packets` and nothing else.  The others run, in queue order, RFC 3550 A.1
 * update_seq without probation (MAX_DROPOUT 3000, MAX_MISORDER 100) on bytes 2-3 (seq), and the
 * A.8 interarrival jitter on bytes 4-7 (timestamp) against the arrival time scaled to the
 * track's clock rate: arrival_rtp = (u32)((u64)arrival_ms * clock_rate / 1000).  The first such
 * packet, and one whose SSRC (bytes 8-11) differs from the current one (counted in
 * `ssrc_changes`), restarts the sequence state, `received` and the jitter.  A jump of 3000 or
 * more is not accepted until its successor arrives (`restarts`); a packet fewer than 100 behind
 * is accepted and counted in `misordered`.  expected = cycles + max_seq - base_seq + 1 (mod 2^32;
 * 0 before the first such packet), lost = expected - received.  clock_rate is the number after
 * the first '/' of the track's rtpmap name (edgpu_sdp_track.name: "H264/90000" gives 90000,
 * "MPEG4-GENERIC/44100/2" 44100); a name without one gives 0 and jitter stays 0.  `missed`
 * counts packets that left a ring before they were examined (a single batch larger than the
 * ring).
 *
 * RTCP sender: `rtcp_packets` / `rtcp_bytes` likewise; a packet of 28 bytes or more whose byte 1
 * is 200 is a sender report: sr_ntp = bytes 8-15, sr_rtp 16-19, sr_packets 20-23, sr_octets
 * 24-27, sr_arrival_ms its arrival; the last one wins.
 *
 * Bitrate: ReflectorStream::UpdateBitRate (APIModules/QTSSReflectorModule/ReflectorStream.h:
 * 542-557), bit for bit.  interval_bytes += len (32-bit, wrapping) for every packet of every
 * sender of the stream that is RTP by port parity (ReflectorStream.cpp:1947; on an
 * RTSP-interleaved push both channels, Q12; on a UDP push the even port only).  The sample step
 * at `now` runs when last_sample_ms + 30000 < now: bps = (float)(u32)(interval_bytes * 8) /
 * (float)(now - last_sample_ms); bps *= 1000; bitrate = (u32)bps; interval_bytes = 0;
 * last_sample_ms = now.
 *
 * Statistics belong to the owning context: they do not travel in session images, a replica
 * session starts disabled, and edgpu_session_remove disables and clears them. */
typedef struct edgpu_stream_stats {
    uint32_t track;
    uint32_t clock_rate;
    /* RTP sender */
    uint64_t packets, bytes;
    uint64_t missed;
    uint32_t short_packets;
    uint32_t has_src, ssrc, ssrc_changes;
    uint32_t base_seq, max_seq, cycles, bad_seq;
    uint32_t received, misordered, restarts;
    uint32_t expected;
    int64_t  lost;
    uint32_t jitter;            /* RTP timestamp units (the filter's state >> 4) */
    uint32_t jitter_scaled;     /* the filter's state, scaled by 16 */
    uint32_t has_transit, transit;
    /* RTCP sender */
    uint64_t rtcp_packets, rtcp_bytes, rtcp_missed;
    uint32_t sr_count, sr_rtp;
    uint64_t sr_ntp;
    uint32_t sr_packets, sr_octets;
    int64_t  sr_arrival_ms;
    /* bitrate */
    uint32_t interval_bytes, bitrate;
    int64_t  last_sample_ms;
} edgpu_stream_stats;
/* Zeroes the statistics of `session`'s tracks and enables them.  last_sample_ms = now_ms, the
 * fLastBitRateSample of the ReflectorStream constructor (ReflectorStream.cpp:141); statistics
 * start at the next packet enqueued.  Enabling an enabled session resets it.  EDGPU_BAD_ARGUMENT
 * for an unknown session.  Syncs. */
int  edgpu_stream_stats_enable(edgpu_ctx* ctx, uint32_t session, int64_t now_ms);
/* Disables and clears them (no-op for a session not enabled). */
int  edgpu_stream_stats_disable(edgpu_ctx* ctx, uint32_t session);
/* The UpdateBitRate call of a ReflectPackets (ReflectorStream.cpp:1054) for every enabled stream:
 * a host calls it with the `now` it gives edgpu_fanout.  Does nothing while no session is
 * enabled. */
int  edgpu_stream_stats_sample(edgpu_ctx* ctx, int64_t now_ms);
/* One record per track of `session`; *n_tracks receives the count (EDGPU_BAD_ARGUMENT if it
 * exceeds `cap`).  EDGPU_ERR when the session is not enabled.  Syncs. */
int  edgpu_stream_stats_get(edgpu_ctx* ctx, uint32_t session, edgpu_stream_stats* out, uint32_t cap,
                            uint32_t* n_tracks);
/* ReflectorSession::GetBitRate (ReflectorSession.cpp:297-309): the sum of the session's streams'
 * bitrates -- what the reference puts into qtssCliSesMovieAverageBitRate at PLAY
 * (QTSSReflectorModule.cpp:1951-1952) and into the stream-info record (ReflectorSession.cpp:372).
 * EDGPU_ERR when the session is not enabled.  Syncs. */
int  edgpu_session_bitrate(edgpu_ctx* ctx, uint32_t session, uint32_t* bps);

/* ---- H.264 elementary-stream tap ----
 *
 * An opt-in tap per H.264 track turns the track's RTP sender ring into an Annex-B elementary
 * stream on the GPU (RFC 6184, non-interleaved mode: single NAL unit packets, STAP-A, FU-A), in
 * whole access units with an index -- what a recorder, a segmenter or a snapshot service needs,
 * without pulling RTP packets to the host.  With no tap enabled nothing is launched, allocated,
 * recorded or copied; a tap reads the rings and never pins a packet: packets that leave a ring
 * before a drain examined them are counted in `missed`.  tests/tap_model.py is the executable
 * statement of the rules below.
 *
 * A drain takes the queue entries of the track's RTP sender in queue order from the tap's head,
 * each with its final length (as the statistics see it); empty entries are ignored.
 *   Parse.  A packet is bad if it is shorter than 12 bytes or its version is not 2.  The header is
 *     12 + 4 CC bytes; with X the 4-byte extension header must fit and the header grows by 4 + 4 x
 *     its BE16 length; with P the last byte is the pad count, bad if 0 or reaching into the header.
 *     An empty payload is bad.  Bad packets count in `skipped` and are otherwise absent: their
 *     sequence number is not trusted (a gap follows naturally if they had one).
 *   Gap.  A good packet has a gap when a previous good packet exists and its sequence number is
 *     not that packet's + 1 (mod 2^16).  Nothing is reordered.
 *   Access units.  A good packet starts a unit if it is the first of a drain, its timestamp
 *     differs from the previous good packet's, or that packet had the marker bit.
 *   NALs, by payload[0] & 0x1F:  1..23: 00 00 00 01 + payload.  24 (STAP-A): after the first byte,
 *     units of [BE16 size][NAL], each emitted as 00 00 00 01 + NAL; a size of 0 or one past the
 *     payload ends the packet there (`malformed`).  28 (FU-A): with S and not E: 00 00 00 01, the
 *     rebuilt header (payload[0] & 0xE0) | (payload[1] & 0x1F), payload[2..]; this opens a chain of
 *     that type.  Without S: payload[2..] iff a chain of the same type is open, the packet has no
 *     gap and starts no unit (E closes the chain); otherwise it is dropped (`orphans`) and the
 *     chain closes.  S and E together, or a payload of one byte: dropped (`malformed`), the chain
 *     closes.  Every other packet closes the chain.  0, 25..27, 29..31: dropped (`unsupported`).
 *   Flags.  KEY: an emitted NAL of type 5.  PARAMS: one of type 7 or 8.  NOMARKER: the unit's last
 *     packet has no marker.  OPEN_END: emitted by a flush.  DAMAGED: a packet of the unit has a gap
 *     (the previous unit too when its last packet had no marker), a packet of it was dropped, a
 *     chain is open at its last packet, or packets were missed before it.
 *   Whole units only.  A unit is complete when its last packet has the marker or a later good
 *     packet is enqueued.  A drain consumes the complete units: the head moves just past the last
 *     packet of the last one, the rest waits.  EDGPU_TAP_FLUSH emits the trailing unit too and
 *     consumes everything.  The counters count consumed entries.
 * Between drains a tap carries its head, the previous good packet's sequence number, a
 * pending-damage bit and the counters.  Taps belong to the owning context: they do not travel in
 * session images, a replica session starts without them, edgpu_session_remove clears them.
 * Out of scope: packetization-mode 2, H.265, reordering.  Audio has a tap of its own: the section
 * "AAC audio tap" below, edgpu_aac_tap_enable and its drain.  (The drained units as an MPEG-2
 * transport stream: edgpu_ts_mux below; as fragmented MP4: edgpu_mp4_mux; as FLV tags: edgpu_flv_mux.) */
#define EDGPU_TAP_KEY       1u
#define EDGPU_TAP_PARAMS    2u
#define EDGPU_TAP_DAMAGED   4u
#define EDGPU_TAP_NOMARKER  8u
#define EDGPU_TAP_OPEN_END 16u
#define EDGPU_TAP_FLUSH     1u      /* edgpu_tap_drain flags */
#define EDGPU_TAP_ROUND    64u      /* queue entries the scan kernel examines per round */
typedef struct edgpu_tap_unit {     /* one access unit */
    uint64_t offset;            /* of its first byte in `out` */
    uint32_t bytes;             /* 0: the unit emitted nothing (it still reports DAMAGED) */
    uint32_t rtp_ts;
    int64_t  arrival_ms;        /* of its first packet */
    uint32_t flags;             /* EDGPU_TAP_KEY ... */
    uint32_t first_seq;
    uint32_t n_packets;         /* good packets, emitted or dropped */
    uint32_t n_nals;            /* start codes emitted */
    uint32_t stream;            /* index of its edgpu_tap_stream row */
    uint32_t _pad;
} edgpu_tap_unit;
typedef struct edgpu_tap_stream {   /* one enabled tap, in (session, track) order */
    uint32_t session, track;
    uint64_t offset;            /* 16-B aligned; the stream's units follow each other from here */
    uint64_t bytes;
    uint32_t unit_first, unit_count;
    /* cumulative since the tap was enabled */
    uint64_t packets;           /* non-empty entries consumed */
    uint64_t skipped, malformed, orphans, unsupported, missed;
    uint64_t units, damaged_units;
} edgpu_tap_stream;
typedef struct edgpu_tap_result {
    uint64_t bytes;             /* of `out` used (or needed) */
    uint32_t units, streams;    /* rows written (or needed) */
} edgpu_tap_result;
/* Enables (or resets) the tap of `track`, from the next packet enqueued.  EDGPU_BAD_ARGUMENT
 * unless the track's payload name is exactly "H264/90000".  The first enable allocates the
 * context's tap tables; each tap holds work buffers sized from its sender's ring.  Syncs. */
int  edgpu_tap_enable(edgpu_ctx* ctx, uint32_t session, uint32_t track);
/* Disables and clears it (no-op for a tap not enabled).  Syncs. */
int  edgpu_tap_disable(edgpu_ctx* ctx, uint32_t session, uint32_t track);
/* Drains every enabled tap in one call, on the context stream (after every earlier ingest), and
 * syncs.  `out` receives the bytes: device memory the kernel writes directly (EDGPU_PTR_DEVICE, 16-B
 * aligned) or host memory (EDGPU_PTR_HOST / EDGPU_PTR_PINNED: the kernel writes a context-owned
 * device buffer that grows on demand, read back before the call returns).  `units` and `streams`
 * are host arrays.  If the bytes, the units or the stream rows do not fit, the call returns
 * EDGPU_OUT_OVERFLOW, `result` holds the sizes needed and nothing is consumed: no head, counter
 * or state changes, and a retry with room yields what a first call would have.  No byte of `out`
 * outside [offset, roundup16(offset + bytes)) of some stream is written. */
int  edgpu_tap_drain(edgpu_ctx* ctx, uint32_t flags, void* out, uint64_t out_cap, int ptr_kind,
                     edgpu_tap_unit* units, uint32_t unit_cap, edgpu_tap_stream* streams, uint32_t stream_cap,
                     edgpu_tap_result* result);

/* ---- MPEG-2 transport-stream mux of tapped access units ----
 *
 * edgpu_ts_mux turns what edgpu_tap_drain returned -- the Annex-B bytes, the unit rows, the stream
 * rows -- into 188-byte transport-stream packets on the GPU: what an HLS segmenter cuts into .ts
 * files (easydarwin_amd/hls.py).  Between calls it depends only on one edgpu_ts_state row per
 * stream, which the caller holds (zero to start): the context keeps no table and there is nothing
 * to enable or disable.  Nothing is launched or allocated until the first call.
 * tests/ts_model.py is the executable statement of the rules below.
 *
 * The output is one run of packets: the streams in row order, each stream's units
 * [unit_first, unit_first + unit_count) in order.  The stream rows' ranges must ascend without
 * overlap (as a drain yields them); a unit no row covers is not muxed and its row is zero.
 *   PTS.  The RTP timestamp is extended per stream: the first unit ever (started == 0) has
 *     ext = rtp_ts; after that ext = prev_ext + (int32)(rtp_ts - (uint32)prev_ext) (mod 2^64).  The
 *     deltas are signed, so a timestamp that steps back gives a smaller PTS.
 *     pts = (ext + pts_offset) mod 2^33.  There is no DTS: every unit is presented in decoding
 *     order, so streams with B-frames are out of scope.  A unit with bytes == 0 emits nothing but
 *     still advances ext (and sets started).
 *   PES.  One per unit with ES bytes: 00 00 01 E0, PES length 00 00 (unbounded), 84 (marker bits +
 *     data alignment), 80 (PTS only), 05, the 5-byte PTS (prefix 0010, 33 bits, three marker
 *     bits); with EDGPU_TS_AUD in effect and the unit shorter than 5 bytes or its byte 4 (the first
 *     NAL header) not of type 9 (& 0x1F): an access unit delimiter 00 00 00 01 09 F0; then the
 *     unit's ES bytes.
 *   Packets of a unit, PID video_pid.  The first has payload-unit-start and an adaptation field of
 *     length 7: flags 0x10 (PCR), plus 0x40 (random access) on an EDGPU_TAP_KEY unit; PCR base
 *     (ext + pts_offset - pcr_lead) mod 2^33, the six reserved bits set, extension 0.  So the first
 *     packet carries up to 176 PES bytes, each later one up to 184.  The last packet is filled from
 *     the front by adaptation-field stuffing: the adaptation-field length, a flags byte 00 when the
 *     length is at least 1, then FF bytes (a remainder of exactly 183 bytes takes an adaptation
 *     field of length 0); when the last packet is also the first, the FF bytes follow the PCR and
 *     lengthen the first packet's adaptation field.  The 4-bit continuity counter runs through the
 *     stream's video packets from cc_video.
 *   PSI.  Before every EDGPU_TAP_KEY unit that has ES bytes: one PAT packet on PID 0 and one PMT
 *     packet on pmt_pid, each with payload-unit-start, pointer field 00, FF fill and a continuity
 *     counter of its own (cc_pat, cc_pmt).  The PAT names one program; the PMT declares stream type
 *     0x1B on video_pid, PCR PID video_pid, no descriptors; both version 0, current.  (The host
 *     computes the CRC-32/MPEG-2 once per call; the kernel patches the counters into two packet
 *     templates.)  The defaults give the PAT section 00 B0 0D 00 01 C1 00 00 00 01 F0 00 2A B1 04 B2
 *     and the PMT section 02 B0 12 00 01 C1 00 00 E1 00 F0 00 1B E1 00 F0 00 15 BD 4D 56.
 *   A unit's row: offset and bytes of its packets (PAT / PMT included; bytes 0 for a unit without ES
 *     bytes, offset where its packets would begin), the tap unit's flags, its pts, its stream row.
 * Configuration: a field that is 0 takes its default, so `flags` 0 means EDGPU_TS_AUD;
 * EDGPU_TS_NOAUD alone turns the delimiter off; pcr_lead 0 means 63000.  PIDs above 0x1FFF, equal
 * PIDs or unknown flag bits are EDGPU_BAD_ARGUMENT.
 * Out of scope: audio PIDs, DTS / B-frames, H.265, SCTE markers.  (Fragmented MP4: edgpu_mp4_mux;
 * FLV: edgpu_flv_mux.) */
#define EDGPU_TS_AUD      1u
#define EDGPU_TS_NOAUD    2u
#define EDGPU_TS_PACKET 188u
typedef struct edgpu_ts_config {     /* 0 in a field: the default */
    uint16_t pmt_pid;                /* 0x1000 */
    uint16_t video_pid;              /* 0x0100, also the PCR PID */
    uint16_t tsid, program;          /* 1, 1 */
    uint32_t flags;                  /* EDGPU_TS_AUD */
    uint32_t pcr_lead;               /* 90-kHz ticks the PCR runs before the PTS; default 63000 (0.7 s) */
    uint64_t pts_offset;             /* added to every PTS, 90 kHz */
} edgpu_ts_config;
typedef struct edgpu_ts_state {      /* per stream, caller-held, zero to start */
    uint64_t ext_ts;                 /* extended RTP timestamp of the last unit muxed */
    uint8_t  started, cc_pat, cc_pmt, cc_video;
    uint32_t _pad;
} edgpu_ts_state;
typedef struct edgpu_ts_unit {       /* one per input unit, same index */
    uint64_t offset;                 /* of its first TS packet in `out`, a multiple of 188 */
    uint32_t bytes;                  /* 188 x its packets, PAT/PMT included; 0 for a unit with no ES bytes */
    uint32_t flags;                  /* the tap unit's */
    uint64_t pts;                    /* 33 bits */
    uint32_t stream, _pad;
} edgpu_ts_unit;
typedef struct edgpu_ts_result { uint64_t bytes; uint32_t units, streams; } edgpu_ts_result;
/* Muxes on the context stream and syncs.  `es` and `out` are each device memory used in place
 * (EDGPU_PTR_DEVICE, 16-B aligned) or host memory (EDGPU_PTR_HOST / EDGPU_PTR_PINNED, through
 * context-owned device staging that grows on demand); `units`, `streams`, `states` (n_streams rows,
 * in / out) and `ts_units` (n_units rows) are host arrays.  EDGPU_BAD_ARGUMENT when a unit reaches
 * outside es_bytes, a unit's `stream` is not below n_streams or a stream's unit range is out of
 * range.  When out_cap is too small the call returns EDGPU_OUT_OVERFLOW, `result` holds what is
 * needed, and no byte of `out`, no unit row and no state row is written: a retry with room gives
 * what a first call would have given.  No byte at or beyond result->bytes is written. */
int  edgpu_ts_mux(edgpu_ctx* ctx, const edgpu_ts_config* cfg /* NULL: defaults */,
                  const void* es, uint64_t es_bytes, int es_kind,
                  const edgpu_tap_unit* units, uint32_t n_units,
                  const edgpu_tap_stream* streams, uint32_t n_streams,
                  edgpu_ts_state* states /* n_streams, in/out */,
                  void* out, uint64_t out_cap, int out_kind,
                  edgpu_ts_unit* ts_units /* n_units */, edgpu_ts_result* result);

/* ---- Fragmented MP4 (CMAF) mux of tapped access units ----
 *
 * edgpu_mp4_mux turns what edgpu_tap_drain returned into movie fragments (ISO/IEC 14496-12 moof +
 * mdat, samples in the length-prefixed form of 14496-15) on the GPU: appended to the ftyp + moov of
 * edgpu_mp4_init they are a recording that is valid after every fragment, and the same fragments are
 * HLS fMP4 / CMAF segments (easydarwin_amd/mp4.py, hls.py).  As with edgpu_ts_mux the caller holds
 * one edgpu_mp4_state row per stream (zero to start); the context keeps no table, and nothing is
 * launched or allocated until the first call.  tests/mp4_model.py is the executable statement of
 * the rules below.
 *
 *   Order.  The streams in row order, each stream's run at the next 16-B aligned offset of `out`
 *     (the bytes between two runs are not written); a stream's fragments follow each other without
 *     a gap, so a run is appended to a file as it is.  result->bytes is the end of the last row's
 *     run.  The stream rows' unit ranges must ascend without overlap; a unit no row covers gets a
 *     zero sample row.
 *   Time.  ext is the RTP timestamp extended per stream exactly as in edgpu_ts_mux (signed 32-bit
 *     steps; started == 0: ext = rtp_ts).  origin is ext at the stream's first unit ever;
 *     dts = (ext - origin + time_offset) mod 2^64.  A unit with bytes == 0 carries no sample: it is
 *     in no fragment, its row has fragment 0xFFFFFFFF, its dts and the tap unit's flags, and is
 *     otherwise zero; it still advances ext and sets started.
 *   Samples.  Each unit with ES bytes is one sample of the same size.  Every occurrence of
 *     00 00 00 01 wholly inside the unit is a start code (so in 00 00 00 00 01 the first byte is
 *     data, and 00 00 01 alone is data); it is replaced by the big-endian 32-bit count of bytes
 *     from its end to the next start code or the unit's end.  Every other byte is copied.  A unit
 *     with ES bytes that does not begin with a start code keeps the bytes before its first one
 *     unchanged and its sample row gets EDGPU_TAP_DAMAGED.  All NALs stay in the sample.
 *   Duration.  A sample's duration is the signed 64-bit difference of the stream's next sample's
 *     ext (in the same call) to its own: 0 if not positive, 0xFFFFFFFF if above that.  last_step
 *     becomes the last strictly positive (clamped) difference computed in the call and is unchanged
 *     if there was none; then the stream's last sample of the call takes last_step if it is
 *     non-zero, otherwise default_duration.  A fragment's tfdt comes from ext, never from summed
 *     durations, so timing cannot drift; the last sample of a call may be off by the difference
 *     between the guessed and the real step.
 *   Fragments.  A stream's fragment starts at its first sample of the call, at every EDGPU_TAP_KEY
 *     sample, and where the running fragment already holds max_samples samples.  Every call closes
 *     its fragments.  sequence counts the stream's fragments from 1 across calls.
 *   Bytes of a fragment of n samples, all fields big-endian: moof (88 + 12n bytes) = box header;
 *     mfhd (16: version/flags 0, sequence_number); traf box header; tfhd (16: flags 0x020000
 *     default-base-is-moof, track 1); tfdt (20: version 1, the u64 dts of the first sample); trun
 *     (20 + 12n: version 0, flags 0x000701, sample_count, data_offset = 88 + 12n + 8, then per
 *     sample duration, size, flags -- 0x02000000 for an EDGPU_TAP_KEY unit, 0x01010000 otherwise);
 *     then mdat: u32 size 8 + the samples' bytes, 'mdat', the samples.
 *   Rows.  A sample row: offset of the sample's bytes in `out`, its size, duration, flags (the tap
 *     unit's, with DAMAGED as above), the index of its fragment row, its dts.  A fragment row:
 *     offset and bytes of moof + mdat, tfdt, sequence, the unit index of its first sample, its
 *     samples, the sum of their durations, the OR of its sample rows' flags (so EDGPU_TAP_KEY says
 *     the fragment begins with a key unit), its stream row.  Fragment rows are in output order.
 * Configuration: a field that is 0 takes its default (max_samples 0: no limit; default_duration
 * 3600).  No flags are defined: a non-zero `flags` is EDGPU_BAD_ARGUMENT, as is a stream row whose
 * units total 2^31 bytes or more, or whose run could reach 2^32 bytes (its units' bytes + 108 per
 * unit: a fragment of one sample has 108 bytes of boxes).
 * Out of scope: audio tracks, B-frames / composition offsets, H.265, a trailing moov, sidx / mfra,
 * encryption.  (The transport stream: edgpu_ts_mux; FLV: edgpu_flv_mux.) */
typedef struct edgpu_mp4_config {    /* 0 in a field: the default */
    uint64_t time_offset;            /* added to every dts, 90 kHz */
    uint32_t max_samples;            /* per fragment; 0: no limit */
    uint32_t default_duration;       /* 3600 */
    uint32_t flags;                  /* none defined */
    uint32_t _pad;
} edgpu_mp4_config;
typedef struct edgpu_mp4_state {     /* per stream, caller-held, zero to start */
    uint64_t ext_ts;                 /* extended RTP timestamp of the last unit muxed */
    uint64_t origin;                 /* ext of the first unit ever */
    uint32_t sequence;               /* fragments emitted so far */
    uint32_t last_step;              /* the last strictly positive sample step */
    uint32_t started, _pad;
} edgpu_mp4_state;
typedef struct edgpu_mp4_sample {    /* one per input unit, same index */
    uint64_t offset;                 /* of its bytes in `out` */
    uint64_t dts;
    uint32_t bytes, duration;
    uint32_t flags;                  /* the tap unit's, | EDGPU_TAP_DAMAGED without a leading start code */
    uint32_t fragment;               /* index of its fragment row; 0xFFFFFFFF: no sample */
} edgpu_mp4_sample;
typedef struct edgpu_mp4_frag {
    uint64_t offset;                 /* of its moof in `out` */
    uint64_t tfdt;
    uint64_t duration;               /* sum of its samples' durations */
    uint32_t bytes;                  /* moof + mdat */
    uint32_t sequence;
    uint32_t unit_first;             /* unit index of its first sample */
    uint32_t samples;
    uint32_t flags;
    uint32_t stream;
} edgpu_mp4_frag;
typedef struct edgpu_mp4_result { uint64_t bytes; uint32_t units, frags, streams, _pad; } edgpu_mp4_result;
/* Muxes on the context stream and syncs.  Pointer kinds, the host arrays and the index checks are
 * those of edgpu_ts_mux; `samples` has n_units rows, `frags` frag_cap rows.  When out_cap or
 * frag_cap is too small the call returns EDGPU_OUT_OVERFLOW, `result` holds the bytes, sample rows
 * and fragment rows needed, and no byte of `out`, no row and no state is written: a retry with room
 * gives what a first call would have given.  No byte outside a stream's run is written. */
int  edgpu_mp4_mux(edgpu_ctx* ctx, const edgpu_mp4_config* cfg /* NULL: defaults */,
                   const void* es, uint64_t es_bytes, int es_kind,
                   const edgpu_tap_unit* units, uint32_t n_units,
                   const edgpu_tap_stream* streams, uint32_t n_streams,
                   edgpu_mp4_state* states /* n_streams, in/out */,
                   void* out, uint64_t out_cap, int out_kind,
                   edgpu_mp4_sample* samples /* n_units */,
                   edgpu_mp4_frag* frags, uint32_t frag_cap, edgpu_mp4_result* result);
/* The initialisation segment the fragments need: ftyp + moov (mvhd; one video trak with tkhd, mdia /
 * mdhd / hdlr 'vide' / minf / vmhd / dinf / stbl; an avc1 sample entry with avcC; empty stts, stsc,
 * stsz, stco; mvex / trex for track 1).  Host only: no context, nothing is launched.  `sps` and
 * `pps` are one NAL each without start code (nal_unit_type 7 and 8, else EDGPU_BAD_ARGUMENT).
 * avcC: version 1, profile / compatibility / level from SPS bytes 1..3, 4-byte lengths, the SPS, the
 * PPS and, for profile_idc 100, 110, 122 and 144, chroma_format_idc and the bit depths.  Width and
 * height (tkhd, sample entry) come from parsing the SPS (H.264 7.3.2.1.1: emulation prevention
 * removed, scaling lists skipped, frame_mbs_only_flag, cropping in crop units); an SPS that does not
 * parse is EDGPU_BAD_ARGUMENT.  timescale 0 means 90000.  *out_len receives the size; when `cap` is
 * smaller the call returns EDGPU_OUT_OVERFLOW and writes nothing else. */
int  edgpu_mp4_init(const uint8_t* sps, uint32_t sps_len, const uint8_t* pps, uint32_t pps_len, uint32_t timescale,
                    uint8_t* out, uint64_t cap, uint64_t* out_len);

/* ---- FLV mux of tapped access units ----
 *
 * edgpu_flv_mux turns what edgpu_tap_drain returned into FLV video tags on the GPU, one per access
 * unit and each complete by itself: after the bytes of edgpu_flv_header they are an .flv file or an
 * HTTP-FLV response, and a tag's bytes from its 12th on (less the last four) are the body of an RTMP
 * video message (easydarwin_amd/flv.py).  Latency is one access unit, not one segment.  As with
 * edgpu_mp4_mux the caller holds one edgpu_flv_state row per stream (zero to start); the context
 * keeps no table, and nothing is launched or allocated until the first call.  tests/flv_model.py is
 * the executable statement of the rules below.
 *
 *   Order.  That of edgpu_mp4_mux: the streams in row order, each stream's run at the next 16-B
 *     aligned offset of `out` (the bytes between two runs are not written); a stream's tags follow
 *     each other without a gap, so a run is appended to a file or a response as it is.
 *     result->bytes is the end of the last row's run.  The stream rows' unit ranges must ascend
 *     without overlap; a unit no row covers gets a zero tag row.
 *   Time.  ext and origin are exactly those of edgpu_mp4_mux (signed 32-bit steps; started == 0:
 *     ext = rtp_ts and origin = ext).  t90 = (ext - origin + time_offset) mod 2^64 and
 *     timestamp_ms = (t90 / 90) mod 2^32, the division unsigned and rounding down.  A unit with
 *     bytes == 0 emits no tag: its row has bytes 0, the offset where its tag would begin, its
 *     timestamp, the tap unit's flags and its stream row; it still advances ext and sets started.
 *   Tag.  A unit of S ES bytes is a tag of S + 20 bytes: 09; BE24 DataSize = S + 5; BE24 the
 *     timestamp's low 24 bits, then its bits 31..24; 00 00 00 (stream id); 17 for an EDGPU_TAP_KEY
 *     unit, else 27 (frame type, codec 7); 01 (AVC NALU); 00 00 00 (composition time); the S sample
 *     bytes; BE32 PreviousTagSize = S + 16.
 *   Sample bytes.  The rule of edgpu_mp4_mux: every occurrence of 00 00 00 01 wholly inside the unit
 *     is a start code (so in 00 00 00 00 01 the first byte is data, and 00 00 01 alone is data); it
 *     is replaced by the big-endian 32-bit count of bytes from its end to the next start code or
 *     the unit's end.  Every other byte is copied.  A unit with ES bytes that does not begin with a
 *     start code keeps the bytes before its first one unchanged and its row gets EDGPU_TAP_DAMAGED.
 *     All NALs stay in the tag.
 *   Parameter sets.  For a unit with EDGPU_TAP_PARAMS (and ES bytes), among its first 8 NALs counted
 *     from its first start code: the first NAL whose header & 0x1F is 7 and the first where it is 8,
 *     each by the offset of its header byte relative to the tag's first byte and by its length.  A
 *     parameter set beyond the eighth NAL is not reported, a NAL of length 0 never; bytes 0: none.
 * No flags are defined: a non-zero `flags` is EDGPU_BAD_ARGUMENT, as is a unit of more than 0xFFFFFA
 * bytes (DataSize is 24 bits) or a stream row whose run could reach 2^32 bytes (its units' bytes +
 * 20 per unit).
 * Out of scope: audio tags, B-frames / a non-zero composition time, H.265 / enhanced FLV, the HTTP
 * and RTMP servers themselves, module prefs, taps on replica sessions, a method of the C++ adapter. */
typedef struct edgpu_flv_config {
    uint64_t time_offset;            /* added to every timestamp before the division, 90 kHz */
    uint32_t flags;                  /* none defined */
    uint32_t _pad;
} edgpu_flv_config;
typedef struct edgpu_flv_state {     /* per stream, caller-held, zero to start */
    uint64_t ext_ts;                 /* extended RTP timestamp of the last unit muxed */
    uint64_t origin;                 /* ext of the first unit ever */
    uint32_t started, _pad;
} edgpu_flv_state;
typedef struct edgpu_flv_tag {       /* one per input unit, same index */
    uint64_t offset;                 /* of the tag's first byte in `out` */
    uint32_t bytes;                  /* unit bytes + 20; 0: no tag */
    uint32_t timestamp_ms;
    uint32_t flags;                  /* the tap unit's, | EDGPU_TAP_DAMAGED without a leading start code */
    uint32_t stream;
    uint32_t sps_offset, sps_bytes;  /* relative to `offset`; bytes 0: none */
    uint32_t pps_offset, pps_bytes;
} edgpu_flv_tag;
typedef struct edgpu_flv_result { uint64_t bytes; uint32_t units, streams; } edgpu_flv_result;
/* Muxes on the context stream and syncs.  Pointer kinds, the host arrays and the index checks are
 * those of edgpu_ts_mux; `tags` has n_units rows.  When out_cap is too small the call returns
 * EDGPU_OUT_OVERFLOW, `result` holds the bytes needed, and no byte of `out`, no row and no state is
 * written: a retry with room gives what a first call would have given.  No byte outside a stream's
 * run is written. */
int  edgpu_flv_mux(edgpu_ctx* ctx, const edgpu_flv_config* cfg /* NULL: defaults */,
                   const void* es, uint64_t es_bytes, int es_kind,
                   const edgpu_tap_unit* units, uint32_t n_units,
                   const edgpu_tap_stream* streams, uint32_t n_streams,
                   edgpu_flv_state* states /* n_streams, in/out */,
                   void* out, uint64_t out_cap, int out_kind,
                   edgpu_flv_tag* tags /* n_units */, edgpu_flv_result* result);
/* What stands before the tags, in up to three parts (`parts` 0: all three, in this order).  Host
 * only: no context, nothing is launched.
 *   EDGPU_FLV_FILE  the 13 bytes 46 4C 56 01 01 00 00 00 09 00 00 00 00: signature, version 1, video
 *     only, header size, PreviousTagSize0.
 *   EDGPU_FLV_META  a script tag (type 12, timestamp 0, DataSize 77; 92 bytes with its
 *     PreviousTagSize) whose data is AMF0: the string "onMetaData" and an ECMA array of three
 *     numbers, width, height and videocodecid (7), closed by 00 00 09.
 *   EDGPU_FLV_SEQ   a video tag at timestamp_ms whose data is 17 00 00 00 00 and the
 *     AVCDecoderConfigurationRecord: the AVC sequence header a decoder needs before the first tag.
 * `sps` and `pps`, the record (byte for byte the payload of edgpu_mp4_init's avcC box) and width and
 * height are those of edgpu_mp4_init, and so are the argument errors, unknown bits of `parts` among
 * them, and the overflow convention: *out_len receives the size; when `cap` is smaller the call
 * returns EDGPU_OUT_OVERFLOW and writes nothing else. */
#define EDGPU_FLV_FILE 1u
#define EDGPU_FLV_META 2u
#define EDGPU_FLV_SEQ  4u
int  edgpu_flv_header(const uint8_t* sps, uint32_t sps_len, const uint8_t* pps, uint32_t pps_len, uint32_t timestamp_ms,
                      uint32_t parts, uint8_t* out, uint64_t cap, uint64_t* out_len);

/* ---- AAC audio tap ----
 *
 * An opt-in tap per MPEG4-GENERIC track turns the track's RTP sender ring into AAC frames on the
 * GPU (RFC 3640, AAC-hbr and AAC-lbr, not interleaved), each behind a generated ADTS header or raw,
 * with an index of the frames -- the audio half of what a recorder or a muxer needs.  It has its own
 * entry points, tables and kernels (edgpu_aac.hip): an RFC 3640 packet carries many units where the
 * H.264 tap builds one unit from many packets, and edgpu_tap_enable refuses every other payload by
 * contract.  With no audio tap enabled nothing is launched, allocated, recorded or copied; a tap
 * reads the rings and never pins a packet.  tests/aac_model.py is the executable statement of the
 * rules below.
 *
 * A drain takes the queue entries of the track's RTP sender in queue order from the tap's head,
 * each with its final length; empty entries are ignored.  Entries that left the ring before a drain
 * examined them count in `missed`.
 *   Parse.  Word for word the H.264 tap's: version, CC, X, P, empty payload.  Bad packets count in
 *     `skipped` and are otherwise absent (a gap follows naturally if they had a sequence number).
 *   Gap.  A good packet has a gap when a previous good packet exists and its sequence number is
 *     not that packet's + 1 (mod 2^16).  Nothing is reordered.
 *   AU-header section.  For a payload of P bytes and an AU header of h bytes (2 for HBR, 1 for
 *     LBR): P < 2, a BE16 bit count of 0, or one that is not a multiple of 8h: the whole packet is
 *     dropped (`malformed`).  n is that count / 8h and H = 2 + n h; H > P: dropped (`malformed`).
 *     n > EDGPU_AAC_MAX_AUS: dropped (`unsupported`).  A non-zero AU-index in the first header or
 *     AU-index-delta in a later one (the header's low 3 bits in HBR, low 2 in LBR) means
 *     interleaving: dropped (`unsupported`).  AU-size is the header's top 13 bits (HBR) or top 6
 *     bits (LBR).  The checks are made in this order.
 *   Whole frames.  If n > 1, or n == 1 with size0 <= P - H, the AUs are emitted in order from
 *     payload byte H.  An AU of size 0, or one that ends past the payload, ends the packet there:
 *     the packet counts once in `malformed`, the AUs before it stay.  Bytes after the last AU are
 *     ignored.
 *   Fragments (HBR only).  A packet with n == 1 and size0 > P - H is a fragment: it carries P - H
 *     bytes of a frame of size0 bytes.  In LBR it is dropped (`malformed`); under ADTS framing with
 *     size0 > 8184 it is dropped (`unsupported`: the ADTS length field has 13 bits).  A fragment
 *     continues the open chain iff a chain is open, the packet has no gap, and its timestamp and
 *     size0 equal the chain's; otherwise it opens a new chain.  A continuing fragment that would
 *     overrun size0 is dropped (`malformed`) and the chain is abandoned.  The chain completes when
 *     its bytes equal size0: the frame is emitted, whatever the marker bit says, and the chain is
 *     closed.  Every other good packet, dropped or not, abandons an open chain.  The fragments of an
 *     abandoned chain count in `orphans`, at the packet that abandons it.
 *   Whole units only.  A drain consumes every entry before the first fragment of a chain still
 *     open at the end of the queue; that fragment and everything behind it waits, and their counters
 *     wait with them -- except that a chain this fragment abandoned is consumed: its fragments count
 *     in `orphans` now and the discontinuity stays pending.  EDGPU_AAC_FLUSH consumes everything; the
 *     open chain's fragments then count in `orphans`.
 *   Frame rows.  rtp_ts is the packet's timestamp + k x frame_samples (mod 2^32) for the k-th AU
 *     of the packet (au_index k); arrival_ms and first_seq are the packet's, a chain's first
 *     fragment's; n_packets is 1, or the chain's fragments.  EDGPU_AAC_FRAGMENTED: rebuilt from a
 *     chain.  EDGPU_AAC_DISCONT: the first frame emitted after a gap, a dropped packet, an abandoned
 *     chain or missed entries -- a muxer must not assume it follows the previous frame.
 *   ADTS.  Under EDGPU_AAC_ADTS seven bytes precede each frame, with L = size + 7, prof =
 *     object_type - 1, f = freq_index, c = channels: FF, F1, (prof<<6)|(f<<2)|(c>>2),
 *     ((c&3)<<6)|(L>>11), (L>>3)&FF, ((L&7)<<5)|1F, FC.  (AAC-LC 44.1 kHz stereo: FF F1 50 80.)
 *   Layout.  A stream's frames follow each other without a gap from a 16-B aligned stream offset,
 *     so a stream's run under ADTS framing is an .aac file as it stands.
 * Between drains a tap carries its head, the previous good packet's sequence number, a
 * pending-discontinuity bit and the counters; it carries no chain, since open chains are never
 * consumed.  Taps belong to the owning context: they do not travel in session images, a replica
 * session starts without them, edgpu_session_remove clears them.
 * Out of scope: audio in edgpu_ts_mux / edgpu_mp4_mux / edgpu_flv_mux, other audio payloads, LATM,
 * interleaved RFC 3640, CTS / DTS / auxiliary sections, reordering, taps on replica sessions, module
 * prefs, a method of the C++ adapter. */
#define EDGPU_AAC_HBR        1u     /* edgpu_aac_config.mode: sizelength 13, indexlength 3, indexdeltalength 3 */
#define EDGPU_AAC_LBR        2u     /* sizelength 6, indexlength 2, indexdeltalength 2 */
#define EDGPU_AAC_ADTS       1u     /* edgpu_aac_config.framing (0 means ADTS) */
#define EDGPU_AAC_RAW        2u
#define EDGPU_AAC_MAX_AUS   16u     /* AU headers per packet */
#define EDGPU_AAC_DISCONT    1u     /* edgpu_aac_frame.flags */
#define EDGPU_AAC_FRAGMENTED 2u
#define EDGPU_AAC_FLUSH      1u     /* edgpu_aac_tap_drain flags */
typedef struct edgpu_aac_config {
    uint32_t mode;              /* EDGPU_AAC_HBR / EDGPU_AAC_LBR */
    uint32_t framing;           /* 0 or EDGPU_AAC_ADTS, EDGPU_AAC_RAW */
    uint32_t object_type;       /* 1..4   \                                               */
    uint32_t freq_index;        /* 0..12   > the first 13 bits of the AudioSpecificConfig */
    uint32_t channels;          /* 1..7   /                                               */
    uint32_t frame_samples;     /* RTP ticks per frame; 0 means 1024 */
} edgpu_aac_config;
typedef struct edgpu_aac_frame {    /* one AAC frame */
    uint64_t offset;            /* of its first byte (its ADTS header's under ADTS framing) in `out` */
    uint32_t bytes;             /* the ADTS header included */
    uint32_t rtp_ts;
    int64_t  arrival_ms;        /* of its (first) packet */
    uint32_t flags;             /* EDGPU_AAC_DISCONT ... */
    uint32_t first_seq;
    uint32_t n_packets;
    uint32_t au_index;          /* its place among its packet's AUs */
    uint32_t stream;            /* index of its edgpu_aac_stream row */
    uint32_t _pad;
} edgpu_aac_frame;
typedef struct edgpu_aac_stream {   /* one enabled audio tap, in (session, track) order */
    uint32_t session, track;
    uint64_t offset;            /* 16-B aligned; the stream's frames follow each other from here */
    uint64_t bytes;
    uint32_t frame_first, frame_count;
    /* cumulative since the tap was enabled */
    uint64_t packets;           /* non-empty entries consumed */
    uint64_t skipped, malformed, orphans, unsupported, missed;
    uint64_t frames, discontinuities;   /* frames emitted; those with EDGPU_AAC_DISCONT */
} edgpu_aac_stream;
typedef struct edgpu_aac_result {
    uint64_t bytes;             /* of `out` used (or needed) */
    uint32_t frames, streams;   /* rows written (or needed) */
} edgpu_aac_result;
/* Reads the a=fmtp line of the SDP's `track`-th media section (0-based): mode=, sizelength,
 * indexlength, indexdeltalength and config= (hex), keys matched case-insensitively.  Host only: no
 * context, nothing is launched.  `out` gets the mode and the first 13 bits of the config; framing
 * and frame_samples are left 0 (ADTS, 1024).  EDGPU_BAD_ARGUMENT: no such section or no fmtp line;
 * a mode or lengths other than AAC-hbr with 13/3/3 or AAC-lbr with 6/2/2; a non-zero
 * auxiliarydatasizelength, ctsdeltalength, dtsdeltalength, randomaccessindication or
 * streamstateindication; a config shorter than 2 bytes; an object type, frequency index or channel
 * count outside the ranges above. */
int  edgpu_aac_config_parse(const char* sdp, uint32_t sdp_len, uint32_t track, edgpu_aac_config* out);
/* Enables (or resets) the audio tap of `track`, from the next packet enqueued.  EDGPU_BAD_ARGUMENT
 * unless the part of the track's payload name before its first '/' is "MPEG4-GENERIC" (compared
 * case-insensitively) and `cfg` is in range.  The first enable allocates the context's audio-tap
 * tables; each tap holds a work buffer sized from its sender's ring (again after the ring grows).
 * Syncs. */
int  edgpu_aac_tap_enable(edgpu_ctx* ctx, uint32_t session, uint32_t track, const edgpu_aac_config* cfg);
/* Disables and clears it (no-op for a tap not enabled).  Syncs. */
int  edgpu_aac_tap_disable(edgpu_ctx* ctx, uint32_t session, uint32_t track);
/* Drains every enabled audio tap in one call, on the context stream, and syncs.  `out`, the host
 * arrays and the pointer kinds are those of edgpu_tap_drain.  If the bytes, the frame rows or the
 * stream rows do not fit, the call returns EDGPU_OUT_OVERFLOW, `result` holds the sizes needed and
 * nothing is consumed: no head, counter or carried state changes, and a retry with room yields what
 * a first call would have.  No byte of `out` outside [offset, roundup16(offset + bytes)) of some
 * stream is written.  Its kernels' event pairs are edgpu_kernel_times(9). */
int  edgpu_aac_tap_drain(edgpu_ctx* ctx, uint32_t flags, void* out, uint64_t out_cap, int ptr_kind,
                         edgpu_aac_frame* frames, uint32_t frame_cap, edgpu_aac_stream* streams, uint32_t stream_cap,
                         edgpu_aac_result* result);

/* Per-launch device durations (ms, HIP events on the ctx stream) recorded since the last
 * call, oldest first, for `which` = 0 fan-out copy kernel, 1 whole fan-out tick (plan +
 * copy), 2 ingest (with the keyframe index it carries), 3 keyframe index (no entries since the
 * index runs inside the ingest kernel), 4 the stream-statistics kernel, 5 a tap drain's kernels,
 * 6 a transport-stream mux's kernels, 7 a fragmented-MP4 mux's kernels, 8 an FLV mux's kernels, 9 an
 * audio-tap drain's kernels (4 to 9 recorded only at EDGPU_TIMING_ALL).  Up to 256 launches are kept; the history is
 * cleared after reading.  Syncs. */
int  edgpu_kernel_times(edgpu_ctx* ctx, int which, float* out_ms, uint32_t max_n, uint32_t* out_n);

/* Which per-launch timing events the context records from now on (default EDGPU_TIMING_ALL).
 * Every event is a marker the stream waits on between two kernels (4-8 us of idle GPU each on
 * MI355X, profiles/r03ak_timing_events_ab/): EDGPU_TIMING_FANOUT keeps only the fan-out copy
 * kernel's pair (edgpu_kernel_times which = 0), EDGPU_TIMING_NONE records none.  Rings not
 * recorded return no entries; edgpu_last_timings reports their last recorded pair, or 0. */
#define EDGPU_TIMING_NONE    0
#define EDGPU_TIMING_FANOUT  1
#define EDGPU_TIMING_ALL     2
int  edgpu_set_timing(edgpu_ctx* ctx, int level);

/* Copies device memory of this context to the host (synchronous).  Reads of 256 KiB or more
 * into pinned memory from edgpu_host_alloc are done by a copy kernel storing over PCIe (faster
 * than the DMA engine's device-to-host copy here); other reads are hipMemcpy copies. */
int  edgpu_copy_to_host(edgpu_ctx* ctx, void* dst, const void* device_src, uint64_t bytes);

/* Device-side timing of the last edgpu_fanout's kernels (HIP events on the ctx stream),
 * in milliseconds: [0] fan-out copy kernel, [1] whole fan-out (plan + copy),
 * [2] ingest (with the keyframe index), [3] 0 (the index runs inside the ingest). */
int  edgpu_last_timings(edgpu_ctx* ctx, float out_ms[4]);

/* Keyframe fast start: bytes a joining subscriber of `session`/`track` would receive now
 * (key pointer -> newest), cf. CKeyFrameCache (CommonUtilitiesLib/keyframecache.h:14-72). */
int  edgpu_gop_span(edgpu_ctx* ctx, uint32_t session, uint32_t track,
                    uint64_t* out_packets, uint64_t* out_bytes);

/* Copies the GOP a joining subscriber of `session`/`track` would receive (key pointer ->
 * newest, RTP sender) to host memory in CKeyFrameCache's TLV record format
 * [0x28][BE16 len][packet][0x29] (CommonUtilitiesLib/keyframecache.cpp:103-143), so the
 * keyframecache interface is served from the GPU's GOP index.  Empty packets (SSRC-filtered)
 * are skipped.  Returns EDGPU_OUT_OVERFLOW if `cap` is too small.  Syncs. */
int  edgpu_gop_copy(edgpu_ctx* ctx, uint32_t session, uint32_t track, uint8_t* dst, uint64_t cap,
                    uint64_t* out_len, uint32_t* out_packets);

/* ---- Cross-GPU keyframe fast start (BASELINE config C4) ----
 * Streams are owned by one GPU (FNV-1a-64 of the stream ID); a subscriber whose egress GPU
 * differs joins a *replica session* there.  The owner exports a session image -- the part
 * of each sender ring a new output can still be served from: key pointer -> newest, or the
 * new-output window when there is no key (ReflectorStream.cpp:1058-1069, 1201-1231) --
 * which travels once per (session, destination GPU) over xGMI (edgpu_memcpy_peer inside a
 * process, RCCL send/recv between processes), and the replica imports it.  A subscriber
 * joining the replica then receives exactly what it would have received joining the owner.
 * Later ticks ship delta images (packets after the previous export's heads), so a replica
 * follows its owner without re-sending the GOP.  Replica sessions are created with
 * edgpu_session_add from the owner's SDP and are never passed to edgpu_ingest.
 *
 * Image format (16-B aligned sections): 64-B header {magic "EDGI", version 1, ntracks,
 * nsenders, bytes, export time, session video-key flag, delta}, per track the packet-id
 * counter, per sender its ring state, then per sender the packet metadata (32 B each) and
 * the slot bytes ('$' 0 BE16(len) + packet + pad) of the packets carried. */
#define EDGPU_IMAGE_FULL 0xFFFFFFFFFFFFFFFFull

/* Exports images of `sessions[0..n)` into device memory `dst` (capacity `cap`), image i
 * at dst + offsets[i], offsets[n] = total bytes.  `from` is NULL (full images) or holds, per
 * sender of each listed session in order (2 * ntracks per session: track t RTP = 2t,
 * RTCP = 2t+1), EDGPU_IMAGE_FULL or the first queue index of a delta (a previous call's
 * `heads` value).  `heads` (optional, same shape) receives each sender's newest index + 1.
 * With dst == NULL only offsets/heads are computed (size query).  Syncs. */
int  edgpu_session_export(edgpu_ctx* ctx, const uint32_t* sessions, uint32_t n, int64_t now_ms,
                          const uint64_t* from, void* dst, uint64_t cap, uint64_t* offsets,
                          uint64_t* heads);

/* Applies images (device memory readable by this context's GPU; offsets as returned by the
 * export, n + 1 entries) to replica sessions `sessions[0..n)` of this context.  A delta
 * must start at the replica's current head.  Returns EDGPU_BAD_ARGUMENT for a mismatched
 * or out-of-order image, EDGPU_RING_OVERFLOW if the replica's rings are too small.  Syncs. */
int  edgpu_session_import(edgpu_ctx* ctx, const void* images, const uint64_t* offsets, uint32_t n,
                          const uint32_t* sessions);
/* Replica feedback (Q9 on a replica).  A backpressure report that relocates an output's bookmark
 * to the newest key frame sets the session's video-key-update flag
 * (ReflectorSender::NeedRelocateBookMark -> ReflectorSession::SetHasVideoKeyFrameUpdate(true),
 * ReflectorStream.cpp:1311-1317), and the session's next audio packet becomes the audio key
 * pointer (:1913-1930).  A replica session does not ingest: its relocations must reach the owner
 * before the owner's next edgpu_keyframe_index.  edgpu_session_relocations: out[i] = 1 when a
 * relocation happened on sessions[i] (of this context) since the last call; the indication is
 * cleared.  edgpu_session_key_update: sets the flag on the owner's sessions (not while an ingest
 * awaits its keyframe index). */
int  edgpu_session_relocations(edgpu_ctx* ctx, const uint32_t* sessions, uint32_t n, uint8_t* out);
int  edgpu_session_key_update(edgpu_ctx* ctx, const uint32_t* sessions, uint32_t n);

/* Enqueues a device-to-device copy from GPU `src_device` into this context's GPU on the
 * context stream (hipMemcpyPeerAsync over xGMI; a plain device copy when the devices are
 * the same).  Stream-ordered before the next call on this context. */
int  edgpu_memcpy_peer(edgpu_ctx* ctx, void* dst, int src_device, const void* src, uint64_t bytes);

/* Device memory on this context's GPU for image buffers (hipMalloc / hipFree).  Peer access
 * to it is enabled for every GPU that can reach this one, so RCCL and peer copies may use it. */
int  edgpu_device_alloc(edgpu_ctx* ctx, uint64_t bytes, void** out);
int  edgpu_device_free(edgpu_ctx* ctx, void* ptr);

/* Peer mailboxes between processes (one process per GPU): the steady-state replica feed without a
 * collective (easydarwin_amd/replica.py PeerMailbox).  edgpu_ipc_export gives the
 * handle of a buffer from edgpu_device_alloc (hipIpcGetMemHandle, HSA dmabuf IPC); another process
 * opens it with edgpu_ipc_open and gets a pointer its own GPU reads and writes over xGMI (peer
 * access enabled lazily) -- edgpu_session_import can read images straight from it, and
 * edgpu_copy_to_host / edgpu_copy_to_device move its header words.  edgpu_ipc_close unmaps it. */
#define EDGPU_IPC_HANDLE_BYTES 64
int  edgpu_ipc_export(edgpu_ctx* ctx, const void* device_ptr, uint8_t handle[EDGPU_IPC_HANDLE_BYTES]);
int  edgpu_ipc_open(edgpu_ctx* ctx, const uint8_t handle[EDGPU_IPC_HANDLE_BYTES], void** out);
int  edgpu_ipc_close(edgpu_ctx* ctx, void* ptr);
/* Copies host memory into device memory this context's GPU can write (its own, or a peer buffer
 * from edgpu_ipc_open); complete when the call returns. */
int  edgpu_copy_to_device(edgpu_ctx* ctx, void* device_dst, const void* src, uint64_t bytes);
/* Diagnostics: enqueues on the context stream one wave that waits `us` microseconds of the device
 * clock and exits -- work the GPU watchdog (edgpu_config.watchdog_ms) can time out on. */
int  edgpu_debug_stall(edgpu_ctx* ctx, uint32_t us);
/* The host CPUs of device `device`'s NUMA node (the sysfs local_cpulist of its PCI function) that
 * the calling thread may run on: cpus[0 .. min(*n_out, cap)), *n_out = how many -- where a server
 * hosting the module belongs (tools/bench_module.py --affinity gpu-node).  No
 * reference counterpart (host placement next to the GPU). */
int  edgpu_device_local_cpus(int device, uint32_t* cpus, uint32_t cap, uint32_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* EDGPU_H */
