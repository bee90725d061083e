// edgpu_flv_header.cpp -- what stands before the tags of edgpu_flv_mux in an .flv file or an
// HTTP-FLV response: the file header, an onMetaData script tag and the AVC sequence header.  Host
// code only, no context and no device work.  The AVCDecoderConfigurationRecord, width and height
// come from edgpu_avc.h, as edgpu_mp4_init's do.
#include <stdint.h>
#include <string.h>
#include <initializer_list>
#include <vector>
#include "edgpu.h"
#include "edgpu_avc.h"

namespace {

typedef std::vector<uint8_t> Bytes;

void put8(Bytes& b, uint32_t v) { b.push_back((uint8_t)v); }
void put16(Bytes& b, uint32_t v) { put8(b, v >> 8); put8(b, v); }
void put24(Bytes& b, uint32_t v) { put8(b, v >> 16); put16(b, v); }
void put32(Bytes& b, uint32_t v) { put16(b, v >> 16); put16(b, v); }

// An AMF0 object property: BE16 name length, the name, a number marker, the big-endian double
void property(Bytes& b, const char* name, double v) {
    const size_t n = strlen(name);
    put16(b, (uint32_t)n);
    b.insert(b.end(), name, name + n);
    put8(b, 0);
    uint64_t bits;
    memcpy(&bits, &v, 8);
    put32(b, (uint32_t)(bits >> 32));
    put32(b, (uint32_t)bits);
}

// One tag and its PreviousTagSize
void tag(Bytes& b, uint32_t type, uint32_t timestamp_ms, const Bytes& data) {
    put8(b, type);
    put24(b, (uint32_t)data.size());
    put24(b, timestamp_ms & 0xFFFFFFu);
    put8(b, timestamp_ms >> 24);
    put24(b, 0);
    b.insert(b.end(), data.begin(), data.end());
    put32(b, 11 + (uint32_t)data.size());
}

}  // namespace

extern "C" int edgpu_flv_header(const uint8_t* sps, uint32_t sps_len, const uint8_t* pps, uint32_t pps_len, uint32_t timestamp_ms,
                                uint32_t parts, uint8_t* out, uint64_t cap, uint64_t* out_len) {
    if (!sps || !pps || !out_len || (!out && cap)) return EDGPU_BAD_ARGUMENT;
    if (parts & ~(EDGPU_FLV_FILE | EDGPU_FLV_META | EDGPU_FLV_SEQ)) return EDGPU_BAD_ARGUMENT;
    edgpu_avc::Sps s;
    if (!edgpu_avc::check_parameter_sets(sps, sps_len, pps, pps_len, &s)) return EDGPU_BAD_ARGUMENT;
    if (!parts) parts = EDGPU_FLV_FILE | EDGPU_FLV_META | EDGPU_FLV_SEQ;

    Bytes all;
    if (parts & EDGPU_FLV_FILE) {
        for (uint8_t v : {0x46, 0x4C, 0x56, 0x01, 0x01}) put8(all, v);     // "FLV", version 1, video only
        put32(all, 9);
        put32(all, 0);                                                      // PreviousTagSize0
    }
    if (parts & EDGPU_FLV_META) {
        Bytes d = {0x02, 0x00, 0x0A};
        for (const char* c = "onMetaData"; *c; c++) put8(d, (uint8_t)*c);
        put8(d, 0x08);                                                      // an ECMA array of three
        put32(d, 3);
        property(d, "width", (double)s.width);
        property(d, "height", (double)s.height);
        property(d, "videocodecid", 7.0);
        put24(d, 9);                                                        // the object's end
        tag(all, 0x12, 0, d);
    }
    if (parts & EDGPU_FLV_SEQ) {
        Bytes d = {0x17, 0x00, 0x00, 0x00, 0x00};                           // key frame, AVC; sequence header; composition time 0
        const Bytes rec = edgpu_avc::config_record(sps, sps_len, pps, pps_len, s);
        d.insert(d.end(), rec.begin(), rec.end());
        tag(all, 0x09, timestamp_ms, d);
    }

    *out_len = all.size();
    if (all.size() > cap) return EDGPU_OUT_OVERFLOW;
    memcpy(out, all.data(), all.size());
    return EDGPU_OK;
}
