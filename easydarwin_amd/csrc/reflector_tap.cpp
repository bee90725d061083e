// reflector_tap.cpp -- the reflector adapter's H.264 elementary-stream tap (Reflector::
// EnableElementaryStream, DisableElementaryStream, DrainElementaryStreams) over edgpu_tap_*.  Apart
// from reflector_adapter.cpp for the reason reflector_stats.cpp is: the adapter object also links
// against a stand-in of the engine ABI that has no tap (tests/tsan).
#include "reflector_adapter.h"

namespace edgpu_reflector {

int Reflector::EnableElementaryStream(uint32_t session, uint32_t track) {
    if (!fCtx) return kRequestFailed;
    std::unique_lock<std::mutex> eg(fEngineMu);
    WaitIdle(eg);                                           // a tick's writes may read the batch
    if (int err = FlushIngest()) return err;                // the tap starts at the next pushed packet
    return edgpu_tap_enable(fCtx, session, track);
}

int Reflector::DisableElementaryStream(uint32_t session, uint32_t track) {
    if (!fCtx) return kRequestFailed;
    std::lock_guard<std::mutex> eg(fEngineMu);
    return edgpu_tap_disable(fCtx, session, track);
}

int Reflector::DrainElementaryStreams(const TapSink& sink, bool flush) {
    if (!fCtx) return kRequestFailed;
    std::unique_lock<std::mutex> eg(fEngineMu);
    WaitIdle(eg);
    if (int err = FlushIngest()) return err;
    std::vector<uint8_t> bytes(1 << 20);
    std::vector<edgpu_tap_unit> units(1024);
    std::vector<edgpu_tap_stream> streams(64);
    edgpu_tap_result res;
    for (int attempt = 0;; attempt++) {
        const int err = edgpu_tap_drain(fCtx, flush ? EDGPU_TAP_FLUSH : 0u, bytes.data(), bytes.size(), EDGPU_PTR_HOST,
                                        units.data(), (uint32_t)units.size(), streams.data(), (uint32_t)streams.size(), &res);
        if (!err) break;
        if (err != EDGPU_OUT_OVERFLOW || attempt) return err;
        bytes.resize(std::max<size_t>(res.bytes, 16));      // nothing was consumed: once more with room
        units.resize(std::max<uint32_t>(res.units, 1));
        streams.resize(std::max<uint32_t>(res.streams, 1));
    }
    if (sink)
        for (uint32_t s = 0; s < res.streams; s++)
            sink(streams[s], units.data() + streams[s].unit_first, bytes.data());
    return kNoErr;
}

}  // namespace edgpu_reflector
