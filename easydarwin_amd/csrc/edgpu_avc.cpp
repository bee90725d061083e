// edgpu_avc.cpp -- the SPS parse and the AVCDecoderConfigurationRecord (edgpu_avc.h): host code only.
#include "edgpu_avc.h"
#include <stddef.h>
#include <initializer_list>

namespace edgpu_avc {
namespace {

typedef std::vector<uint8_t> Bytes;

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

bool high_syntax(uint32_t p) {
    for (uint32_t v : {100u, 110u, 122u, 244u, 44u, 83u, 86u, 118u, 128u, 138u, 139u, 134u, 135u}) if (p == v) return true;
    return false;
}

}  // namespace

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

Bytes config_record(const uint8_t* sps, uint32_t sps_len, const uint8_t* pps, uint32_t pps_len, const Sps& s) {
    Bytes r = {1, sps[1], sps[2], sps[3], 0xFF, 0xE1, (uint8_t)(sps_len >> 8), (uint8_t)sps_len};
    r.insert(r.end(), sps, sps + sps_len);
    r.insert(r.end(), {1, (uint8_t)(pps_len >> 8), (uint8_t)pps_len});
    r.insert(r.end(), pps, pps + pps_len);
    if (s.profile == 100 || s.profile == 110 || s.profile == 122 || s.profile == 144)
        r.insert(r.end(), {(uint8_t)(0xFC | s.chroma), (uint8_t)(0xF8 | (s.depth_luma - 8)), (uint8_t)(0xF8 | (s.depth_chroma - 8)), 0});
    return r;
}

bool check_parameter_sets(const uint8_t* sps, uint32_t sps_len, const uint8_t* pps, uint32_t pps_len, Sps* out) {
    if (sps_len < 4 || sps_len > 0xFFFF || pps_len < 1 || pps_len > 0xFFFF) return false;
    if ((sps[0] & 0x1F) != 7 || (pps[0] & 0x1F) != 8) return false;
    return parse_sps(sps, sps_len, out);
}

}  // namespace edgpu_avc
