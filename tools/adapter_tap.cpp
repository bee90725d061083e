// adapter_tap -- drives the reflector adapter's elementary-stream tap (reflector_tap.cpp) from a
// script and records what every drain hands its sink (tests/test_gpu_adapter_tap.py).
//
//   adapter_tap <record file>
//
// Script (stdin), one command per line:
//   S <udp_push 0|1> <sdp with "\n" written as '|'>   Reflector::SetupReflectorSession; prints "session <id>"
//   R <session> <kill_outputs 0|1>                     Reflector::RemoveSession
//   O <session> <interleaved 0|1>                      Reflector::AddOutput
//   P <session> <track> <is_rtcp 0|1> <now_ms> <hex>   Reflector::PushPacket
//   T <now_ms>                                         Reflector::ReflectPackets into a null sink
//   E <session> <track>                                Reflector::EnableElementaryStream
//   D <session> <track>                                Reflector::DisableElementaryStream
//   X es  <flush 0|1> <sink 0|1>                       Reflector::DrainElementaryStreams
//   X ts  <flush 0|1> <sink 0|1> [pmt_pid video_pid tsid program flags pcr_lead pts_offset]
//                                                      Reflector::DrainTransportStreams (no numbers: no config)
//   X mp4 <flush 0|1> <sink 0|1> [time_offset max_samples default_duration]
//                                                      Reflector::DrainFragments (no numbers: no config)
// sink 0 passes an empty std::function.  A call that returns non-zero ends the run: exit status 1,
// "adapter_tap: '<cmd>' failed: <code> <edgpu_last_error()>" on stderr.  Nothing is retried here.
//
// Every X appends one record to the record file (little endian, the structs as they are in memory):
//   u32 kind (0 es, 1 ts, 2 mp4), u32 sink calls, then per sink call
//     es:  edgpu_tap_stream, u32 n, n edgpu_tap_unit (the stream's), u64 m, m bytes from bytes + stream.offset
//     ts:  edgpu_tap_stream, u32 n, n edgpu_ts_unit (the stream's), u64 base, u64 m, m bytes from
//          packets + base: from the stream's first row to the end of its last one
//     mp4: edgpu_tap_stream, edgpu_mp4_frag, u32 n, n edgpu_mp4_sample (the stream's, from
//          stream.unit_first: frag.unit_first - stream.unit_first is the fragment's first), u64 m,
//          m bytes from bytes + frag.offset
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

struct Record {
    std::vector<uint8_t> b;
    void put(const void* p, size_t n) { b.insert(b.end(), (const uint8_t*)p, (const uint8_t*)p + n); }
    void u32(uint32_t v) { put(&v, 4); }
    void u64(uint64_t v) { put(&v, 8); }
};
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: adapter_tap <record file> < script\n"); return 2; }
    FILE* rec = fopen(argv[1], "wb");
    if (!rec) { fprintf(stderr, "adapter_tap: cannot write %s\n", argv[1]); return 2; }
    Reflector r;
    if (r.Status()) { fprintf(stderr, "adapter_tap: no engine: %s\n", edgpu_last_error()); return 2; }
    NullSink sink;
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
            uint32_t session = 0;
            in >> udp;
            std::getline(in, sdp);
            sdp.erase(0, sdp.find_first_not_of(' '));
            for (char& c : sdp) if (c == '|') c = '\n';
            if ((err = r.SetupReflectorSession(sdp, udp != 0, &session)) == 0) {
                printf("session %u\n", session);
                fflush(stdout);
            }
        } else if (cmd == 'R') {
            uint32_t session;
            int kill;
            in >> session >> kill;
            err = r.RemoveSession(session, kill != 0);
        } else if (cmd == 'O') {
            uint32_t session, handle;
            int tcp;
            in >> session >> tcp;
            err = r.AddOutput(session, tcp != 0, &handle);
        } else if (cmd == 'P') {
            uint32_t session, track;
            int rtcp;
            long long now;
            std::string hex;
            in >> session >> track >> rtcp >> now >> hex;
            std::string bytes;
            bytes.reserve(hex.size() / 2);
            auto nib = [](char c) { return c <= '9' ? c - '0' : (c | 0x20) - 'a' + 10; };
            for (size_t i = 0; i + 1 < hex.size(); i += 2) bytes.push_back((char)(nib(hex[i]) << 4 | nib(hex[i + 1])));
            r.PushPacket(session, track, bytes.data(), (uint32_t)bytes.size(), rtcp != 0, now);
        } else if (cmd == 'T') {
            long long now;
            in >> now;
            err = r.ReflectPackets(now, &sink);
        } else if (cmd == 'E' || cmd == 'D') {
            uint32_t session, track;
            in >> session >> track;
            err = cmd == 'E' ? r.EnableElementaryStream(session, track) : r.DisableElementaryStream(session, track);
        } else if (cmd == 'X') {
            std::string kind;
            int flush, real;
            in >> kind >> flush >> real;
            std::vector<unsigned long long> v;
            for (unsigned long long x; in >> x;) v.push_back(x);
            Record out;
            uint32_t calls = 0;
            if (kind == "es" && v.empty()) {
                Reflector::TapSink fn;
                if (real)
                    fn = [&](const edgpu_tap_stream& st, const edgpu_tap_unit* units, const uint8_t* bytes) {
                        calls++;
                        out.put(&st, sizeof(st));
                        out.u32(st.unit_count);
                        out.put(units, st.unit_count * sizeof(edgpu_tap_unit));
                        out.u64(st.bytes);
                        out.put(bytes + st.offset, st.bytes);
                    };
                err = r.DrainElementaryStreams(fn, flush != 0);
            } else if (kind == "ts" && (v.empty() || v.size() == 7)) {
                edgpu_ts_config cfg = {};
                if (!v.empty()) {
                    cfg.pmt_pid = (uint16_t)v[0]; cfg.video_pid = (uint16_t)v[1]; cfg.tsid = (uint16_t)v[2];
                    cfg.program = (uint16_t)v[3]; cfg.flags = (uint32_t)v[4]; cfg.pcr_lead = (uint32_t)v[5];
                    cfg.pts_offset = v[6];
                }
                Reflector::TsSink fn;
                if (real)
                    fn = [&](const edgpu_tap_stream& st, const edgpu_ts_unit* units, const uint8_t* packets) {
                        calls++;
                        out.put(&st, sizeof(st));
                        out.u32(st.unit_count);
                        out.put(units, st.unit_count * sizeof(edgpu_ts_unit));
                        const uint64_t base = st.unit_count ? units[0].offset : 0;
                        const uint64_t end = st.unit_count ? units[st.unit_count - 1].offset + units[st.unit_count - 1].bytes : 0;
                        out.u64(base);
                        out.u64(end - base);
                        out.put(packets + base, end - base);
                    };
                err = r.DrainTransportStreams(fn, flush != 0, v.empty() ? nullptr : &cfg);
            } else if (kind == "mp4" && (v.empty() || v.size() == 3)) {
                edgpu_mp4_config cfg = {};
                if (!v.empty()) { cfg.time_offset = v[0]; cfg.max_samples = (uint32_t)v[1]; cfg.default_duration = (uint32_t)v[2]; }
                Reflector::Mp4Sink fn;
                if (real)
                    fn = [&](const edgpu_tap_stream& st, const edgpu_mp4_frag& fr, const edgpu_mp4_sample* samples, const uint8_t* bytes) {
                        calls++;
                        out.put(&st, sizeof(st));
                        out.put(&fr, sizeof(fr));
                        out.u32(st.unit_count);
                        out.put(samples + st.unit_first, st.unit_count * sizeof(edgpu_mp4_sample));
                        out.u64(fr.bytes);
                        out.put(bytes + fr.offset, fr.bytes);
                    };
                err = r.DrainFragments(fn, flush != 0, v.empty() ? nullptr : &cfg);
            } else {
                fprintf(stderr, "adapter_tap: bad drain '%s'\n", line.c_str());
                return 2;
            }
            if (!err) {
                const uint32_t head[2] = {kind == "es" ? 0u : kind == "ts" ? 1u : 2u, calls};
                if (fwrite(head, 4, 2, rec) != 2 || (!out.b.empty() && fwrite(out.b.data(), 1, out.b.size(), rec) != out.b.size())) {
                    fprintf(stderr, "adapter_tap: cannot write %s\n", argv[1]);
                    return 2;
                }
                fflush(rec);
            }
        } else {
            fprintf(stderr, "adapter_tap: bad command '%c'\n", cmd);
            return 2;
        }
        if (err) { fprintf(stderr, "adapter_tap: '%c' failed: %d %s %s\n", cmd, err, edgpu_last_error(), r.LastError().c_str()); return 1; }
    }
    fclose(rec);
    return 0;
}
