// edgpu_mp4_init.cpp -- the initialisation segment (ftyp + moov) of the fragmented-MP4 mux: host
// code only, no context and no device work.  The boxes are those of ISO/IEC 14496-12 and the avc1 /
// avcC sample entry of 14496-15; width and height come from the SPS (H.264 7.3.2.1.1).
#include <stdint.h>
#include <string.h>
#include <initializer_list>
#include <string>
#include <vector>
#include "edgpu.h"

namespace {

typedef std::vector<uint8_t> Bytes;

void put8(Bytes& b, uint32_t v) { b.push_back((uint8_t)v); }
void put16(Bytes& b, uint32_t v) { put8(b, v >> 8); put8(b, v); }
void put32(Bytes& b, uint32_t v) { put16(b, v >> 16); put16(b, v); }
void zeros(Bytes& b, size_t n) { b.insert(b.end(), n, 0); }
void tag(Bytes& b, const char* t) { b.insert(b.end(), t, t + 4); }
void append(Bytes& b, const Bytes& a) { b.insert(b.end(), a.begin(), a.end()); }
void matrix(Bytes& b) { for (uint32_t v : {0x00010000u, 0u, 0u, 0u, 0x00010000u, 0u, 0u, 0u, 0x40000000u}) put32(b, v); }

Bytes box(const char* type, const Bytes& payload) {
    Bytes b;
    put32(b, (uint32_t)payload.size() + 8);
    tag(b, type);
    append(b, payload);
    return b;
}
Bytes boxes(const char* type, std::initializer_list<Bytes> children) {
    Bytes p;
    for (const Bytes& c : children) append(p, c);
    return box(type, p);
}

// RBSP bits, most significant first; `ok` goes false once a read runs past the end
struct Bits {
    Bytes d;
    size_t pos = 0;
    bool ok = true;
    uint32_t u(int n) {
        uint32_t v = 0;
        for (int i = 0; i < n; i++) {
            if (pos >= d.size() * 8) { ok = false; return 0; }
            v = (v << 1) | ((d[pos >> 3] >> (7 - (pos & 7))) & 1u);
            pos++;
        }
        return v;
    }
    uint32_t ue() {
        int z = 0;
        while (ok && u(1) == 0) if (++z > 31) { ok = false; return 0; }
        if (!ok) return 0;
        return z ? ((1u << z) - 1) + u(z) : 0;
    }
    int32_t se() {
        const uint32_t k = ue();
        return (k & 1) ? (int32_t)((k + 1) / 2) : -(int32_t)(k / 2);
    }
};

struct Sps {
    uint32_t profile = 0, chroma = 1, depth_luma = 8, depth_chroma = 8;
    uint32_t width = 0, height = 0;
};

bool high_syntax(uint32_t p) {
    for (uint32_t v : {100u, 110u, 122u, 244u, 44u, 83u, 86u, 118u, 128u, 138u, 139u, 134u, 135u}) if (p == v) return true;
    return false;
}

bool parse_sps(const uint8_t* nal, uint32_t len, Sps* out) {
    Bits b;
    for (uint32_t i = 1; i < len; i++) {                    // emulation prevention: 00 00 03 -> 00 00
        if (i >= 3 && nal[i] == 3 && nal[i - 1] == 0 && nal[i - 2] == 0) continue;
        b.d.push_back(nal[i]);
    }
    Sps s;
    s.profile = b.u(8);
    b.u(16);
    b.ue();                                                 // seq_parameter_set_id
    uint32_t separate = 0;
    if (high_syntax(s.profile)) {
        s.chroma = b.ue();
        if (s.chroma > 3) return false;
        if (s.chroma == 3) separate = b.u(1);
        s.depth_luma = 8 + b.ue();
        s.depth_chroma = 8 + b.ue();
        if (s.depth_luma > 14 || s.depth_chroma > 14) return false;
        b.u(1);                                             // qpprime_y_zero_transform_bypass_flag
        if (b.u(1)) {                                       // scaling lists: read and dropped
            const int lists = s.chroma != 3 ? 8 : 12;
            for (int i = 0; i < lists && b.ok; i++) {
                if (!b.u(1)) continue;
                int last = 8, next = 8;
                for (int j = 0, n = i < 6 ? 16 : 64; j < n && b.ok; j++) {
                    if (next) next = (last + b.se() + 256) % 256;
                    last = next ? next : last;
                }
            }
        }
    }
    b.ue();                                                 // log2_max_frame_num_minus4
    const uint32_t poc = b.ue();
    if (poc == 0) b.ue();
    else if (poc == 1) {
        b.u(1); b.se(); b.se();
        const uint32_t n = b.ue();
        if (n > 255) return false;
        for (uint32_t i = 0; i < n && b.ok; i++) b.se();
    } else if (poc != 2) return false;
    b.ue();                                                 // max_num_ref_frames
    b.u(1);
    const uint64_t wmbs = (uint64_t)b.ue() + 1, hmap = (uint64_t)b.ue() + 1;
    const uint32_t frame_only = b.u(1);
    if (!frame_only) b.u(1);
    b.u(1);                                                 // direct_8x8_inference_flag
    uint64_t cl = 0, cr = 0, ct = 0, cb = 0;
    if (b.u(1)) { cl = b.ue(); cr = b.ue(); ct = b.ue(); cb = b.ue(); }
    if (!b.ok) return false;
    const uint32_t array_type = separate ? 0 : s.chroma;
    const uint64_t ux = (array_type == 1 || array_type == 2) ? 2 : 1;
    const uint64_t uy = (array_type == 1 ? 2 : 1) * (2 - frame_only);
    const uint64_t w = wmbs * 16, h = (2 - frame_only) * hmap * 16;
    if (ux * (cl + cr) >= w || uy * (ct + cb) >= h) return false;
    const uint64_t cw = w - ux * (cl + cr), ch = h - uy * (ct + cb);
    if (cw > 0xFFFF || ch > 0xFFFF) return false;
    s.width = (uint32_t)cw;
    s.height = (uint32_t)ch;
    *out = s;
    return true;
}

Bytes full(uint32_t version_flags) { Bytes b; put32(b, version_flags); return b; }

}  // namespace

extern "C" int edgpu_mp4_init(const uint8_t* sps, uint32_t sps_len, const uint8_t* pps, uint32_t pps_len, uint32_t timescale,
                              uint8_t* out, uint64_t cap, uint64_t* out_len) {
    if (!sps || !pps || !out_len || (!out && cap)) return EDGPU_BAD_ARGUMENT;
    if (sps_len < 4 || sps_len > 0xFFFF || pps_len < 1 || pps_len > 0xFFFF) return EDGPU_BAD_ARGUMENT;
    if ((sps[0] & 0x1F) != 7 || (pps[0] & 0x1F) != 8) return EDGPU_BAD_ARGUMENT;
    Sps s;
    if (!parse_sps(sps, sps_len, &s)) return EDGPU_BAD_ARGUMENT;
    if (!timescale) timescale = 90000;

    Bytes ftyp;
    tag(ftyp, "iso5"); put32(ftyp, 0x200); tag(ftyp, "iso5"); tag(ftyp, "iso6"); tag(ftyp, "mp41");

    Bytes mvhd = full(0);
    put32(mvhd, 0); put32(mvhd, 0); put32(mvhd, timescale); put32(mvhd, 0);
    put32(mvhd, 0x00010000); put16(mvhd, 0x0100); zeros(mvhd, 10);
    matrix(mvhd); zeros(mvhd, 24); put32(mvhd, 2);

    Bytes tkhd = full(0x000007);
    put32(tkhd, 0); put32(tkhd, 0); put32(tkhd, 1); put32(tkhd, 0); put32(tkhd, 0); zeros(tkhd, 8);
    put16(tkhd, 0); put16(tkhd, 0); put16(tkhd, 0); put16(tkhd, 0);
    matrix(tkhd); put32(tkhd, s.width << 16); put32(tkhd, s.height << 16);

    Bytes mdhd = full(0);
    put32(mdhd, 0); put32(mdhd, 0); put32(mdhd, timescale); put32(mdhd, 0); put16(mdhd, 0x55C4); put16(mdhd, 0);

    Bytes hdlr = full(0);
    put32(hdlr, 0); tag(hdlr, "vide"); zeros(hdlr, 12);
    for (const char* c = "VideoHandler"; *c; c++) put8(hdlr, (uint8_t)*c);
    put8(hdlr, 0);

    Bytes vmhd = full(1);
    zeros(vmhd, 8);

    Bytes dref = full(0);
    put32(dref, 1);
    append(dref, box("url ", full(1)));

    Bytes avcc;
    put8(avcc, 1); put8(avcc, sps[1]); put8(avcc, sps[2]); put8(avcc, sps[3]); put8(avcc, 0xFF);
    put8(avcc, 0xE1); put16(avcc, sps_len); avcc.insert(avcc.end(), sps, sps + sps_len);
    put8(avcc, 1); put16(avcc, pps_len); avcc.insert(avcc.end(), pps, pps + pps_len);
    if (s.profile == 100 || s.profile == 110 || s.profile == 122 || s.profile == 144) {
        put8(avcc, 0xFC | s.chroma); put8(avcc, 0xF8 | (s.depth_luma - 8)); put8(avcc, 0xF8 | (s.depth_chroma - 8)); put8(avcc, 0);
    }

    Bytes avc1;
    zeros(avc1, 6); put16(avc1, 1); zeros(avc1, 16);
    put16(avc1, s.width); put16(avc1, s.height); put32(avc1, 0x00480000); put32(avc1, 0x00480000);
    put32(avc1, 0); put16(avc1, 1); zeros(avc1, 32); put16(avc1, 0x0018); put16(avc1, 0xFFFF);
    append(avc1, box("avcC", avcc));

    Bytes stsd = full(0);
    put32(stsd, 1);
    append(stsd, box("avc1", avc1));
    Bytes empty = full(0);
    put32(empty, 0);
    Bytes stsz = full(0);
    put32(stsz, 0); put32(stsz, 0);

    Bytes trex = full(0);
    put32(trex, 1); put32(trex, 1); put32(trex, 0); put32(trex, 0); put32(trex, 0);

    const Bytes stbl = boxes("stbl", {box("stsd", stsd), box("stts", empty), box("stsc", empty), box("stsz", stsz), box("stco", empty)});
    const Bytes minf = boxes("minf", {box("vmhd", vmhd), boxes("dinf", {box("dref", dref)}), stbl});
    const Bytes mdia = boxes("mdia", {box("mdhd", mdhd), box("hdlr", hdlr), minf});
    const Bytes trak = boxes("trak", {box("tkhd", tkhd), mdia});
    const Bytes moov = boxes("moov", {box("mvhd", mvhd), trak, boxes("mvex", {box("trex", trex)})});
    Bytes all = box("ftyp", ftyp);
    append(all, moov);

    *out_len = all.size();
    if (all.size() > cap) return EDGPU_OUT_OVERFLOW;
    memcpy(out, all.data(), all.size());
    return EDGPU_OK;
}
