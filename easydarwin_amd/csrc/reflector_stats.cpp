// reflector_stats.cpp -- the reflector adapter's per-stream statistics (Reflector::EnableStreamStats,
// GetStreamStats, GetBitRate) over edgpu_stream_stats_*.  They live apart from reflector_adapter.cpp
// so that the adapter also links against a stand-in of the engine ABI that has no statistics
// (tests/tsan): the tick reaches the sample step only through Reflector::fSampleStats, which
// EnableStreamStats sets.
#include "reflector_adapter.h"

namespace edgpu_reflector {

int Reflector::EnableStreamStats(uint32_t session, int64_t nowMs) {
    if (!fCtx) return kRequestFailed;
    std::unique_lock<std::mutex> eg(fEngineMu);
    WaitIdle(eg);                                           // a tick's writes may read the batch
    int err = FlushIngest();                                // statistics start at the next pushed packet
    if (err) return err;
    if ((err = edgpu_stream_stats_enable(fCtx, session, nowMs))) return err;
    if (fStatsOn.size() <= session) fStatsOn.resize(session + 1, 0);
    if (!fStatsOn[session]) { fStatsOn[session] = 1; fNumStats++; }
    fSampleStats = &edgpu_stream_stats_sample;
    return kNoErr;
}

int Reflector::DisableStreamStats(uint32_t session) {
    if (!fCtx) return kRequestFailed;
    std::lock_guard<std::mutex> eg(fEngineMu);
    const int err = edgpu_stream_stats_disable(fCtx, session);
    if (!err) StatsOff(session);
    return err;
}

int Reflector::GetStreamStats(uint32_t session, std::vector<edgpu_stream_stats>* out) {
    if (!fCtx || !out) return kBadArgument;
    std::lock_guard<std::mutex> eg(fEngineMu);
    out->assign(16, edgpu_stream_stats());                  // a session has at most 16 tracks
    uint32_t n = 0;
    const int err = edgpu_stream_stats_get(fCtx, session, out->data(), (uint32_t)out->size(), &n);
    out->resize(err ? 0 : n);
    return err;
}

uint32_t Reflector::GetBitRate(uint32_t session) {
    if (!fCtx) return 0;
    std::lock_guard<std::mutex> eg(fEngineMu);
    uint32_t bps = 0;
    return edgpu_session_bitrate(fCtx, session, &bps) ? 0u : bps;
}

}  // namespace edgpu_reflector
