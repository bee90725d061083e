// edgpu_mp4_init.cpp -- the initialisation segment (ftyp + moov) of the fragmented-MP4 mux: host
// code only, no context and no device work.  The boxes are those of ISO/IEC 14496-12 and the avc1 /
// avcC sample entry of 14496-15; the avcC payload, width and height come from edgpu_avc.h.
#include <stdint.h>
#include <string.h>
#include <initializer_list>
#include <string>
#include <vector>
#include "edgpu.h"
#include "edgpu_avc.h"

namespace {

using edgpu_avc::Sps;
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

Bytes full(uint32_t version_flags) { Bytes b; put32(b, version_flags); return b; }

}  // namespace

extern "C" int edgpu_mp4_init(const uint8_t* sps, uint32_t sps_len, const uint8_t* pps, uint32_t pps_len, uint32_t timescale,
                              uint8_t* out, uint64_t cap, uint64_t* out_len) {
    if (!sps || !pps || !out_len || (!out && cap)) return EDGPU_BAD_ARGUMENT;
    Sps s;
    if (!edgpu_avc::check_parameter_sets(sps, sps_len, pps, pps_len, &s)) return EDGPU_BAD_ARGUMENT;
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

    const Bytes avcc = edgpu_avc::config_record(sps, sps_len, pps, pps_len, s);

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
