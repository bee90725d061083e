// reflector_tap.cpp -- the reflector adapter's H.264 elementary-stream tap (Reflector::
// EnableElementaryStream, DisableElementaryStream, DrainElementaryStreams, DrainTransportStreams,
// DrainFragments) over edgpu_tap_*, edgpu_ts_mux and edgpu_mp4_mux.  Apart
// from reflector_adapter.cpp for the reason reflector_stats.cpp is: the adapter object also links
// against a stand-in of the engine ABI that has no tap (tests/tsan).
#include "reflector_adapter.h"

#include <algorithm>
#include <cstring>

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
    const uint64_t key = ((uint64_t)session << 32) | track;
    for (size_t i = 0; i < fTsStates.size(); i++)
        if (fTsStates[i].first == key) { fTsStates.erase(fTsStates.begin() + i); break; }
    for (size_t i = 0; i < fMp4States.size(); i++)
        if (fMp4States[i].first == key) { fMp4States.erase(fMp4States.begin() + i); break; }
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

int Reflector::DrainTransportStreams(const TsSink& sink, bool flush, const edgpu_ts_config* cfg) {
    if (!fCtx) return kRequestFailed;
    std::unique_lock<std::mutex> eg(fEngineMu);
    WaitIdle(eg);
    if (int err = FlushIngest()) return err;
    // the drain stays on the device: only the packets come to the host
    void* es = nullptr;
    uint64_t es_cap = 1 << 20;
    std::vector<edgpu_tap_unit> units(1024);
    std::vector<edgpu_tap_stream> streams(64);
    edgpu_tap_result res;
    if (int err = edgpu_device_alloc(fCtx, es_cap, &es)) return err;
    for (int attempt = 0;; attempt++) {
        const int err = edgpu_tap_drain(fCtx, flush ? EDGPU_TAP_FLUSH : 0u, es, es_cap, EDGPU_PTR_DEVICE,
                                        units.data(), (uint32_t)units.size(), streams.data(), (uint32_t)streams.size(), &res);
        if (!err) break;
        if (err != EDGPU_OUT_OVERFLOW || attempt) { edgpu_device_free(fCtx, es); return err; }
        units.resize(std::max<uint32_t>(res.units, 1));
        streams.resize(std::max<uint32_t>(res.streams, 1));
        if (res.bytes > es_cap) {
            edgpu_device_free(fCtx, es);
            es_cap = res.bytes;
            if (int e2 = edgpu_device_alloc(fCtx, es_cap, &es)) return e2;
        }
    }
    std::vector<edgpu_ts_state> states(res.streams);
    for (uint32_t s = 0; s < res.streams; s++) {
        const uint64_t key = ((uint64_t)streams[s].session << 32) | streams[s].track;
        memset(&states[s], 0, sizeof(edgpu_ts_state));
        for (const auto& k : fTsStates) if (k.first == key) states[s] = k.second;
    }
    std::vector<edgpu_ts_unit> rows(std::max<uint32_t>(res.units, 1));
    std::vector<uint8_t> packets(1 << 20);
    edgpu_ts_result tres;
    int err = 0;
    for (int attempt = 0;; attempt++) {
        err = edgpu_ts_mux(fCtx, cfg, es, res.bytes, EDGPU_PTR_DEVICE, units.data(), res.units, streams.data(), res.streams,
                           states.data(), packets.data(), packets.size(), EDGPU_PTR_HOST, rows.data(), &tres);
        if (err != EDGPU_OUT_OVERFLOW || attempt) break;
        packets.resize(tres.bytes);                         // nothing was written: once more with room
    }
    edgpu_device_free(fCtx, es);
    if (err) return err;
    for (uint32_t s = 0; s < res.streams; s++) {
        const uint64_t key = ((uint64_t)streams[s].session << 32) | streams[s].track;
        bool found = false;
        for (auto& k : fTsStates) if (k.first == key) { k.second = states[s]; found = true; }
        if (!found) fTsStates.emplace_back(key, states[s]);
    }
    if (sink)
        for (uint32_t s = 0; s < res.streams; s++)
            sink(streams[s], rows.data() + streams[s].unit_first, packets.data());
    return kNoErr;
}

int Reflector::DrainFragments(const Mp4Sink& sink, bool flush, const edgpu_mp4_config* cfg) {
    if (!fCtx) return kRequestFailed;
    std::unique_lock<std::mutex> eg(fEngineMu);
    WaitIdle(eg);
    if (int err = FlushIngest()) return err;
    // the drain stays on the device: only the fragments come to the host
    void* es = nullptr;
    uint64_t es_cap = 1 << 20;
    std::vector<edgpu_tap_unit> units(1024);
    std::vector<edgpu_tap_stream> streams(64);
    edgpu_tap_result res;
    if (int err = edgpu_device_alloc(fCtx, es_cap, &es)) return err;
    for (int attempt = 0;; attempt++) {
        const int err = edgpu_tap_drain(fCtx, flush ? EDGPU_TAP_FLUSH : 0u, es, es_cap, EDGPU_PTR_DEVICE,
                                        units.data(), (uint32_t)units.size(), streams.data(), (uint32_t)streams.size(), &res);
        if (!err) break;
        if (err != EDGPU_OUT_OVERFLOW || attempt) { edgpu_device_free(fCtx, es); return err; }
        units.resize(std::max<uint32_t>(res.units, 1));
        streams.resize(std::max<uint32_t>(res.streams, 1));
        if (res.bytes > es_cap) {
            edgpu_device_free(fCtx, es);
            es_cap = res.bytes;
            if (int e2 = edgpu_device_alloc(fCtx, es_cap, &es)) return e2;
        }
    }
    std::vector<edgpu_mp4_state> states(res.streams);
    for (uint32_t s = 0; s < res.streams; s++) {
        const uint64_t key = ((uint64_t)streams[s].session << 32) | streams[s].track;
        memset(&states[s], 0, sizeof(edgpu_mp4_state));
        for (const auto& k : fMp4States) if (k.first == key) states[s] = k.second;
    }
    std::vector<edgpu_mp4_sample> rows(std::max<uint32_t>(res.units, 1));
    std::vector<edgpu_mp4_frag> frags(std::max<uint32_t>(res.units, 1));     // a fragment holds at least one unit
    std::vector<uint8_t> bytes(1 << 20);
    edgpu_mp4_result mres;
    int err = 0;
    for (int attempt = 0;; attempt++) {
        err = edgpu_mp4_mux(fCtx, cfg, es, res.bytes, EDGPU_PTR_DEVICE, units.data(), res.units, streams.data(), res.streams,
                            states.data(), bytes.data(), bytes.size(), EDGPU_PTR_HOST, rows.data(), frags.data(),
                            (uint32_t)frags.size(), &mres);
        if (err != EDGPU_OUT_OVERFLOW || attempt) break;
        bytes.resize(mres.bytes);                           // nothing was written: once more with room
    }
    edgpu_device_free(fCtx, es);
    if (err) return err;
    for (uint32_t s = 0; s < res.streams; s++) {
        const uint64_t key = ((uint64_t)streams[s].session << 32) | streams[s].track;
        bool found = false;
        for (auto& k : fMp4States) if (k.first == key) { k.second = states[s]; found = true; }
        if (!found) fMp4States.emplace_back(key, states[s]);
    }
    if (sink)
        for (uint32_t f = 0; f < mres.frags; f++)
            sink(streams[frags[f].stream], frags[f], rows.data(), bytes.data());
    return kNoErr;
}

}  // namespace edgpu_reflector
