// edgpu_avc.h -- what the container headers need from an H.264 SPS and PPS (host code): the fields
// of the SPS that give the picture size (H.264 7.3.2.1.1) and the AVCDecoderConfigurationRecord of
// ISO/IEC 14496-15.  edgpu_mp4_init (the avcC box, tkhd, the sample entry) and edgpu_flv_header (the
// AVC sequence header, onMetaData) both take them from here.
#pragma once
#include <stdint.h>
#include <vector>

namespace edgpu_avc {

struct Sps {
    uint32_t profile = 0, chroma = 1, depth_luma = 8, depth_chroma = 8;
    uint32_t width = 0, height = 0;
};

// `nal` is one SPS NAL without start code.  False when it does not parse.
bool parse_sps(const uint8_t* nal, uint32_t len, Sps* out);

// The record: version 1, profile / compatibility / level from SPS bytes 1..3, 4-byte lengths, the
// SPS, the PPS and, for profile_idc 100, 110, 122 and 144, chroma_format_idc and the bit depths.
std::vector<uint8_t> config_record(const uint8_t* sps, uint32_t sps_len, const uint8_t* pps, uint32_t pps_len, const Sps& s);

// The argument checks edgpu_mp4_init and edgpu_flv_header share: the lengths, the NAL types, the parse.
bool check_parameter_sets(const uint8_t* sps, uint32_t sps_len, const uint8_t* pps, uint32_t pps_len, Sps* out);

}  // namespace edgpu_avc
