// adapter_stats -- drives the reflector adapter's per-stream statistics from a script and prints,
// after every tick, what the adapter's getters and the C ABI's report (tests/test_gpu_stats.py).
//
// Script (stdin), one command per line:
//   S <udp_push 0|1> <sdp with "\n" written as '|'>   set up the push session
//   O <interleaved 0|1>                                add an output (so that ticks relay)
//   E <now_ms>                                         Reflector::EnableStreamStats
//   P <track> <is_rtcp 0|1> <now_ms> <hex bytes>       Reflector::PushPacket
//   T <now_ms>                                         Reflector::ReflectPackets, then one report line
// Report line: "<now> adapter <bitrate> <per track: packets bytes received jitter_scaled bitrate
// interval_bytes last_sample_ms>... abi <the same from edgpu_session_bitrate / edgpu_stream_stats_get>"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "reflector_adapter.h"

using namespace edgpu_reflector;

namespace {
struct NullSink : OutputSink {
    int WritePacket(uint32_t, uint16_t, bool, bool, const uint8_t*, uint32_t, uint32_t) override { return kNoErr; }
};

void print_tracks(const std::vector<edgpu_stream_stats>& v) {
    for (const edgpu_stream_stats& s : v)
        printf(" %llu %llu %u %u %u %u %lld", (unsigned long long)s.packets, (unsigned long long)s.bytes, s.received,
               s.jitter_scaled, s.bitrate, s.interval_bytes, (long long)s.last_sample_ms);
}
}  // namespace

int main() {
    Reflector r;
    if (r.Status()) { fprintf(stderr, "adapter_stats: no engine: %s\n", edgpu_last_error()); return 2; }
    NullSink sink;
    uint32_t session = 0;
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        char cmd;
        in >> cmd;
        int err = 0;
        if (cmd == 'S') {
            int udp;
            std::string sdp;
            in >> udp;
            std::getline(in, sdp);
            sdp.erase(0, sdp.find_first_not_of(' '));
            for (char& c : sdp) if (c == '|') c = '\n';
            err = r.SetupReflectorSession(sdp, udp != 0, &session);
        } else if (cmd == 'O') {
            int tcp;
            uint32_t handle;
            in >> tcp;
            err = r.AddOutput(session, tcp != 0, &handle);
        } else if (cmd == 'E') {
            long long now;
            in >> now;
            err = r.EnableStreamStats(session, now);
        } else if (cmd == 'P') {
            uint32_t track;
            int rtcp;
            long long now;
            std::string hex;
            in >> track >> rtcp >> now >> hex;
            std::string bytes;
            for (size_t i = 0; i + 1 < hex.size(); i += 2) bytes.push_back((char)strtoul(hex.substr(i, 2).c_str(), nullptr, 16));
            r.PushPacket(session, track, bytes.data(), (uint32_t)bytes.size(), rtcp != 0, now);
        } else if (cmd == 'T') {
            long long now;
            in >> now;
            if ((err = r.ReflectPackets(now, &sink)) == 0) {
                std::vector<edgpu_stream_stats> a, b(16);
                uint32_t n = 0, bps = 0;
                err = r.GetStreamStats(session, &a);
                const uint32_t adapter_bps = r.GetBitRate(session);
                std::lock_guard<std::mutex> g(r.EngineMutex());
                if (!err) err = edgpu_stream_stats_get(r.Context(), session, b.data(), 16, &n);
                if (!err) err = edgpu_session_bitrate(r.Context(), session, &bps);
                if (!err) {
                    b.resize(n);
                    printf("%lld adapter %u", now, adapter_bps);
                    print_tracks(a);
                    printf(" abi %u", bps);
                    print_tracks(b);
                    printf("\n");
                }
            }
        } else {
            fprintf(stderr, "adapter_stats: bad command '%c'\n", cmd);
            return 2;
        }
        if (err) { fprintf(stderr, "adapter_stats: '%c' failed: %d %s %s\n", cmd, err, edgpu_last_error(), r.LastError().c_str()); return 1; }
    }
    return 0;
}
