// edgpu_aac_config.cpp -- edgpu_aac_config_parse: the RFC 3640 parameters of an SDP media section's
// a=fmtp line, as the audio tap needs them.  Host only: no context, nothing is launched.
#include <ctype.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include <map>
#include <string>
#include "edgpu.h"

namespace {

std::string lower(std::string s) {
    for (char& c : s) c = (char)tolower((unsigned char)c);
    return s;
}

std::string trim(const std::string& s) {
    size_t a = 0, b = s.size();
    while (a < b && isspace((unsigned char)s[a])) a++;
    while (b > a && isspace((unsigned char)s[b - 1])) b--;
    return s.substr(a, b - a);
}

// The decimal value of `s`, or -1
long number(const std::string& s) {
    if (s.empty() || s.size() > 9) return -1;
    for (char c : s) if (!isdigit((unsigned char)c)) return -1;
    return atol(s.c_str());
}

int hexval(char c) {
    return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
}

}  // namespace

extern "C" int edgpu_aac_config_parse(const char* sdp, uint32_t sdp_len, uint32_t track, edgpu_aac_config* out) {
    if (!sdp || !out) return EDGPU_BAD_ARGUMENT;
    // the track-th media section's first a=fmtp line
    std::string fmtp;
    bool found = false;
    int64_t section = -1;
    for (size_t at = 0; at < sdp_len && !found;) {
        size_t eol = at;
        while (eol < sdp_len && sdp[eol] != '\n' && sdp[eol] != '\r') eol++;
        const std::string line(sdp + at, eol - at);
        if (line.compare(0, 2, "m=") == 0) section++;
        else if (section == (int64_t)track && strncasecmp(line.c_str(), "a=fmtp:", 7) == 0) { fmtp = line.substr(7); found = true; }
        at = eol;
        while (at < sdp_len && (sdp[at] == '\n' || sdp[at] == '\r')) at++;
    }
    if (!found) return EDGPU_BAD_ARGUMENT;
    // "<payload type> key=value; key=value; ..."
    fmtp = trim(fmtp);
    size_t sp = 0;
    while (sp < fmtp.size() && !isspace((unsigned char)fmtp[sp])) sp++;
    std::map<std::string, std::string> kv;
    for (size_t at = sp; at < fmtp.size();) {
        size_t semi = fmtp.find(';', at);
        if (semi == std::string::npos) semi = fmtp.size();
        const std::string item = fmtp.substr(at, semi - at);
        const size_t eq = item.find('=');
        if (eq != std::string::npos) kv[lower(trim(item.substr(0, eq)))] = trim(item.substr(eq + 1));
        at = semi + 1;
    }
    const std::string mode = lower(kv.count("mode") ? kv["mode"] : "");
    const long size = number(kv["sizelength"]), index = number(kv["indexlength"]), delta = number(kv["indexdeltalength"]);
    edgpu_aac_config c;
    memset(&c, 0, sizeof(c));
    if (mode == "aac-hbr" && size == 13 && index == 3 && delta == 3) c.mode = EDGPU_AAC_HBR;
    else if (mode == "aac-lbr" && size == 6 && index == 2 && delta == 2) c.mode = EDGPU_AAC_LBR;
    else return EDGPU_BAD_ARGUMENT;
    for (const char* k : {"auxiliarydatasizelength", "ctsdeltalength", "dtsdeltalength", "randomaccessindication", "streamstateindication"})
        if (kv.count(k) && number(kv[k]) != 0) return EDGPU_BAD_ARGUMENT;
    // the first 13 bits of the AudioSpecificConfig: 5 object type, 4 frequency index, 4 channels
    const std::string hex = kv["config"];
    if (hex.size() < 4 || hex.size() % 2) return EDGPU_BAD_ARGUMENT;
    for (char ch : hex) if (hexval(ch) < 0) return EDGPU_BAD_ARGUMENT;
    const uint32_t v = (uint32_t)((hexval(hex[0]) << 12) | (hexval(hex[1]) << 8) | (hexval(hex[2]) << 4) | hexval(hex[3]));
    c.object_type = v >> 11;
    c.freq_index = (v >> 7) & 15u;
    c.channels = (v >> 3) & 15u;
    if (c.object_type < 1 || c.object_type > 4 || c.freq_index > 12 || c.channels < 1 || c.channels > 7) return EDGPU_BAD_ARGUMENT;
    *out = c;
    return EDGPU_OK;
}
