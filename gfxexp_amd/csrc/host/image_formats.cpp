// image_formats.cpp -- see image_formats.h.  The readers here take untrusted bytes: every header field is bounded before it enters
// any size arithmetic, and every read is checked against the length of the input.
#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include "image_formats.h"
#include "image_codecs.h"
#include "../bc/bc_decode.hip.h"        // gfx::bc::block_bytes (plain C++ under a host compiler)

namespace gfx_img {

bool dds_parse(const uint8_t* data, size_t bytes, gfxh_dds_info& info, std::string& err) {
    auto fail = [&](const std::string& why) { err = why; return false; };
    std::memset(&info, 0, sizeof(info));
    const uint8_t* d = data;
    if (bytes < 128 || std::memcmp(d, "DDS ", 4) != 0) return fail("not a DDS file");
    auto u32 = [&](size_t at) { uint32_t v; std::memcpy(&v, d + at, 4); return v; };   // at + 4 <= 128 <= bytes, or checked below
    const uint32_t flags = u32(8), height = u32(12), width = u32(16), depth = u32(24), mips = u32(28);
    const uint32_t pfFlags = u32(80), bitCount = u32(88), rMask = u32(92), gMask = u32(96), bMask = u32(100), aMask = u32(104), caps2 = u32(112);
    if (caps2 & 0xFE00u) return fail("cube maps are not handled");
    if ((caps2 & 0x200000u) || ((flags & 0x800000u) && depth > 1)) return fail("volume textures are not handled");
    size_t offset = 128;
    enum { kNone = 0xFFu, kRGBA = 0x100u, kBGRA = 0x101u };
    uint32_t fmt = kNone;
    bool srgb = false;
    if ((pfFlags & 0x4u) && std::memcmp(d + 84, "DX10", 4) == 0) {
        if (bytes < 148) return fail("truncated DX10 header");
        const uint32_t dxgi = u32(128), dimension = u32(132), misc = u32(136), arraySize = u32(140);
        offset = 148;
        if (misc & 0x4u) return fail("cube maps are not handled");
        if (dimension != 3) return fail("only two-dimensional textures are handled");
        if (arraySize > 1) return fail("texture arrays are not handled");
        switch (dxgi) {
        case 71: case 72: fmt = GFX_BC1; break;
        case 74: case 75: fmt = GFX_BC2; break;
        case 77: case 78: fmt = GFX_BC3; break;
        case 80: fmt = GFX_BC4_UNORM; break;
        case 81: fmt = GFX_BC4_SNORM; break;
        case 83: fmt = GFX_BC5_UNORM; break;
        case 84: fmt = GFX_BC5_SNORM; break;
        case 98: case 99: fmt = GFX_BC7; break;
        case 28: case 29: fmt = kRGBA; break;
        case 87: case 91: fmt = kBGRA; break;
        case 95: case 96: return fail("BC6H (HDR) blocks are not decoded; convert with the asset's authoring tool to .pfm");
        default: return fail("DXGI format " + std::to_string(dxgi) + " is not handled");
        }
        srgb = dxgi == 72 || dxgi == 75 || dxgi == 78 || dxgi == 99 || dxgi == 29 || dxgi == 91;   // translate: the _SRGB formats only
    }
    else if (pfFlags & 0x4u) {
        static const struct { const char* code; uint32_t fmt; } kFourCC[] = {
            { "DXT1", GFX_BC1 }, { "DXT3", GFX_BC2 }, { "DXT5", GFX_BC3 }, { "BC4U", GFX_BC4_UNORM }, { "ATI1", GFX_BC4_UNORM }, { "BC4S", GFX_BC4_SNORM },
            { "ATI2", GFX_BC5_UNORM }, { "BC5U", GFX_BC5_UNORM }, { "BC5S", GFX_BC5_SNORM } };
        for (const auto& f : kFourCC) if (std::memcmp(d + 84, f.code, 4) == 0) fmt = f.fmt;
        if (fmt == kNone) {
            std::string code;
            for (int k = 0; k < 4; ++k) code.push_back(std::isprint(d[84 + k]) ? static_cast<char>(d[84 + k]) : '?');
            return fail("FourCC '" + code + "' is not handled");
        }
    }
    else if (bitCount == 32 && rMask == 0xFFu && gMask == 0xFF00u && bMask == 0xFF0000u) fmt = kRGBA;
    else if (bitCount == 32 && rMask == 0xFF0000u && gMask == 0xFF00u && bMask == 0xFFu) fmt = kBGRA;
    else { (void)aMask; return fail("uncompressed layout with " + std::to_string(bitCount) + " bits is not handled (32-bit RGBA / BGRA only)"); }
    if (width == 0 || height == 0) return fail("empty image");
    if (width > kMaxDim || height > kMaxDim) return fail("image larger than 16384 x 16384");
    info.width = width; info.height = height; info.mipCount = mips ? mips : 1;
    info.isBlockCompressed = fmt < kRGBA ? 1u : 0u;
    info.bcFormat = fmt < kRGBA ? fmt : 0u;
    info.isBGRA = fmt == kBGRA ? 1u : 0u;
    info.isSRGB = srgb ? 1u : 0u;
    info.dataOffset = offset;
    info.dataBytes = fmt < kRGBA ? static_cast<uint64_t>((width + 3) / 4) * ((height + 3) / 4) * gfx::bc::block_bytes(fmt) : 4ull * width * height;
    if (info.dataBytes > bytes - offset) return fail("the file ends before level 0 does");
    return true;
}

namespace {
// the input as the readers below address it
struct Bytes {
    const uint8_t* p; size_t n;
    size_t size() const { return n; }
    const uint8_t* data() const { return p; }
    uint8_t operator[](size_t i) const { return p[i]; }
};
// next whitespace-separated token of a Netpbm header ('#' comments skipped)
bool pnm_token(const Bytes& d, size_t& at, std::string& tok) {
    tok.clear();
    while (at < d.size()) {
        if (d[at] == '#') { while (at < d.size() && d[at] != '\n') ++at; }
        else if (std::isspace(d[at])) ++at;
        else break;
    }
    while (at < d.size() && !std::isspace(d[at])) tok.push_back(static_cast<char>(d[at++]));
    return !tok.empty();
}
// ---- OpenEXR (the format the reference reads "-env-texture" from: loadEnvTexture -> tinyexr LoadEXR, common_host.cpp:2674): single-part
// scanline files, channels R G B A (or Y) stored as HALF / FLOAT / UINT, compression NONE, RLE, ZIPS, ZIP -- what OpenEXR's own tools and
// most exporters write by default besides PIZ, which this reader names and refuses.  The file layout follows the OpenEXR file-layout
// document (magic, version, attribute list, chunk offset table, chunks of 1 / 16 scanlines each stored channel by channel in
// alphabetical order); ZIP / RLE chunks are a zlib stream (RFC 1950 / 1951, inflated below) or run lengths over the chunk's bytes
// after a byte-delta predictor and an even / odd byte split.
// (inflate_zlib for the ZIP / ZIPS chunks lives in image_codecs.cpp, next to the PNG reader that shares it)
inline float half_to_float(uint16_t h) {
    const uint32_t sign = static_cast<uint32_t>(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3FFu;
    uint32_t bits;
    if (e == 0) {
        if (m == 0) bits = sign;
        else { int shift = 0; uint32_t mm = m; while (!(mm & 0x400u)) { mm <<= 1; ++shift; } bits = sign | ((113u - shift) << 23) | ((mm & 0x3FFu) << 13); }
    }
    else if (e == 31) bits = sign | 0x7F800000u | (m << 13);
    else bits = sign | ((e + 112u) << 23) | (m << 13);
    float f; std::memcpy(&f, &bits, 4);
    return f;
}
bool decode_exr(const Bytes& d, Image& img, std::string& err) {
    auto fail = [&](const std::string& what) { err = "EXR: " + what; return false; };
    size_t at = 8;
    const uint32_t version = d[4] | (d[5] << 8) | (d[6] << 16) | (static_cast<uint32_t>(d[7]) << 24);
    if ((version & 0xFFu) != 2u) return fail("unknown file version");
    if (version & 0x1A00u) return fail("tiled, deep and multi-part files are not read (single-part scanline only)");
    struct Channel { std::string name; int type; };
    std::vector<Channel> channels;
    int compression = -1;
    int32_t win[4] = { 0, 0, -1, -1 };
    bool haveWindow = false;
    auto rd_i32 = [&](size_t o) { int32_t v; std::memcpy(&v, d.data() + o, 4); return v; };
    for (;;) {
        if (at >= d.size()) return fail("truncated header");
        if (d[at] == 0) { ++at; break; }
        std::string name, type;
        while (at < d.size() && d[at]) name.push_back(static_cast<char>(d[at++]));
        ++at;
        while (at < d.size() && d[at]) type.push_back(static_cast<char>(d[at++]));
        ++at;
        if (at + 4 > d.size()) return fail("truncated header");
        const int32_t size = rd_i32(at); at += 4;
        if (size < 0 || at + static_cast<size_t>(size) > d.size()) return fail("truncated header");
        if (name == "channels") {
            size_t c = at;
            const size_t end = at + size;
            while (c < end && d[c]) {
                Channel ch;
                while (c < end && d[c]) ch.name.push_back(static_cast<char>(d[c++]));
                ++c;
                if (c + 16 > end) return fail("truncated channel list");
                ch.type = rd_i32(c);
                if (rd_i32(c + 8) != 1 || rd_i32(c + 12) != 1) return fail("subsampled channels are not read");
                if (ch.type < 0 || ch.type > 2) return fail("unknown pixel type");
                c += 16;
                channels.push_back(ch);
            }
        }
        else if (name == "compression" && size == 1) compression = d[at];
        else if (name == "dataWindow" && size == 16) { for (int k = 0; k < 4; ++k) win[k] = rd_i32(at + 4 * k); haveWindow = true; }
        at += size;
    }
    if (channels.empty() || !haveWindow || compression < 0) return fail("header without channels / dataWindow / compression");
    static const char* names[] = { "NONE", "RLE", "ZIPS", "ZIP", "PIZ", "PXR24", "B44", "B44A", "DWAA", "DWAB" };
    if (compression > 3) return fail(std::string("compression ") + (compression < 10 ? names[compression] : "?") + " is not read (NONE, RLE, ZIPS, ZIP are; re-save the file)");
    const int64_t w64 = static_cast<int64_t>(win[2]) - win[0] + 1, h64 = static_cast<int64_t>(win[3]) - win[1] + 1;
    if (w64 <= 0 || h64 <= 0 || w64 > kMaxDim || h64 > kMaxDim) return fail("image larger than 16384 x 16384 or empty");
    const uint32_t w = static_cast<uint32_t>(w64), h = static_cast<uint32_t>(h64);
    const uint32_t linesPerChunk = compression == 3 ? 16u : 1u;
    const uint32_t numChunks = (h + linesPerChunk - 1) / linesPerChunk;
    if (at + 8ull * numChunks > d.size()) return fail("truncated offset table");
    size_t lineBytes = 0;
    for (const Channel& c : channels) lineBytes += (c.type == 1 ? 2ull : 4ull) * w;
    // which file channel feeds which of R G B A (a lone Y feeds R, G and B)
    int src[4] = { -1, -1, -1, -1 };
    for (size_t c = 0; c < channels.size(); ++c) {
        const std::string& nm = channels[c].name;
        if (nm == "R") src[0] = static_cast<int>(c); else if (nm == "G") src[1] = static_cast<int>(c);
        else if (nm == "B") src[2] = static_cast<int>(c); else if (nm == "A") src[3] = static_cast<int>(c);
    }
    if (src[0] < 0 && src[1] < 0 && src[2] < 0)
        for (size_t c = 0; c < channels.size(); ++c) if (channels[c].name == "Y") src[0] = src[1] = src[2] = static_cast<int>(c);
    if (src[0] < 0 && src[1] < 0 && src[2] < 0) return fail("no R, G, B or Y channel");
    // The offset table and the chunk headers are checked BEFORE the 16 w h bytes of the image are asked for: a compressed file has no
    // size bound of its own, so a crafted header must not be able to make a tiny file allocate gigabytes (and an allocation that still
    // fails is an error return, not an exception through the extern "C" loader).
    for (uint32_t k = 0; k < numChunks; ++k) {
        uint64_t off; std::memcpy(&off, d.data() + at + 8ull * k, 8);
        if (off > d.size() || d.size() - off < 8) return fail("chunk offset outside the file");
        const int32_t y0 = rd_i32(off), size = rd_i32(off + 4);
        const int64_t row0 = static_cast<int64_t>(y0) - win[1];
        if (size < 0 || static_cast<uint64_t>(size) > d.size() - off - 8 || row0 < 0 || row0 >= h) return fail("malformed chunk");
        if (row0 % linesPerChunk != 0) return fail("chunk that does not start on a multiple of its line count (it would overlap its neighbours)");
    }
    // every scan line costs the file at least a byte or two (ZIP / RLE shrink a constant line by ~1000 : 1 at best)
    if (static_cast<uint64_t>(lineBytes) * h / 4096u > d.size()) return fail("image far larger than its file can hold");
    img.w = w; img.h = h; img.isFloat = true;
    try { img.rgba32f.assign(4ull * w * h, 0.0f); }
    catch (const std::bad_alloc&) { return fail("out of memory for the image"); }
    for (size_t i = 0; i < static_cast<size_t>(w) * h; ++i) img.rgba32f[4 * i + 3] = 1.0f;
    std::vector<uint8_t> raw, tmp;
    for (uint32_t k = 0; k < numChunks; ++k) {
        uint64_t off; std::memcpy(&off, d.data() + at + 8ull * k, 8);
        if (off > d.size() || d.size() - off < 8) return fail("chunk offset outside the file");            // (no off + 8: the field is untrusted)
        const int32_t y0 = rd_i32(off), size = rd_i32(off + 4);
        const int64_t row0 = static_cast<int64_t>(y0) - win[1];
        if (size < 0 || static_cast<uint64_t>(size) > d.size() - off - 8 || row0 < 0 || row0 >= h) return fail("malformed chunk");
        const uint32_t lines = std::min<uint32_t>(linesPerChunk, h - static_cast<uint32_t>(row0));
        const size_t want = lineBytes * lines;
        const uint8_t* body = d.data() + off + 8;
        if (compression == 0 || static_cast<size_t>(size) == want) {       // a chunk that did not shrink is stored as it is
            if (static_cast<size_t>(size) != want) return fail("chunk of the wrong size");
            raw.assign(body, body + want);
        }
        else {
            if (compression == 1) {                                           // run lengths: n < 0 -> -n literal bytes, else n + 1 copies of the next
                tmp.clear();
                size_t i = 0;
                while (i < static_cast<size_t>(size)) {
                    const int n = static_cast<int8_t>(body[i++]);
                    if (n < 0) { if (i + static_cast<size_t>(-n) > static_cast<size_t>(size)) return fail("malformed RLE chunk"); tmp.insert(tmp.end(), body + i, body + i - n); i += static_cast<size_t>(-n); }
                    else { if (i >= static_cast<size_t>(size)) return fail("malformed RLE chunk"); tmp.insert(tmp.end(), static_cast<size_t>(n) + 1, body[i++]); }
                    if (tmp.size() > want) return fail("malformed RLE chunk");
                }
                if (tmp.size() != want) return fail("malformed RLE chunk");
            }
            else if (!inflate_zlib(body, static_cast<size_t>(size), tmp, want)) return fail("malformed ZIP chunk");
            for (size_t i = 1; i < want; ++i) tmp[i] = static_cast<uint8_t>(tmp[i - 1] + tmp[i] - 128);      // byte-delta predictor
            raw.resize(want);
            const size_t half = (want + 1) / 2;
            for (size_t i = 0; i < want; ++i) raw[i] = (i & 1) ? tmp[half + i / 2] : tmp[i / 2];              // even bytes first, then odd
        }
        for (uint32_t l = 0; l < lines; ++l) {
            const uint8_t* line = raw.data() + lineBytes * l;
            float* out = img.rgba32f.data() + 4ull * (static_cast<size_t>(row0) + l) * w;
            size_t chOff = 0;
            for (size_t c = 0; c < channels.size(); ++c) {
                const int type = channels[c].type;
                for (int k4 = 0; k4 < 4; ++k4) {
                    if (src[k4] != static_cast<int>(c)) continue;
                    for (uint32_t x = 0; x < w; ++x) {
                        float v;
                        if (type == 1) { uint16_t hv; std::memcpy(&hv, line + chOff + 2ull * x, 2); v = half_to_float(hv); }
                        else if (type == 2) std::memcpy(&v, line + chOff + 4ull * x, 4);
                        else { uint32_t u; std::memcpy(&u, line + chOff + 4ull * x, 4); v = static_cast<float>(u); }
                        out[4ull * x + k4] = v;
                    }
                }
                chOff += (type == 1 ? 2ull : 4ull) * w;
            }
        }
    }
    return true;
}

bool decode_by_magic(const Bytes& d, Image& img, std::string& err) {
    if (gfx_img::sniff(d.data(), d.size()) != gfx_img::kKindNone) {      // before the TGA test below, which any FF D8 FF E0 would pass
        gfx_img::Info info;
        if (!gfx_img::decode(d.data(), d.size(), info, img.rgba8, err)) return false;
        img.w = info.width; img.h = info.height;
        return true;
    }
    if (d.size() >= 8 && d[0] == 0x76 && d[1] == 0x2f && d[2] == 0x31 && d[3] == 0x01) return decode_exr(d, img, err);
    if (d.size() >= 2 && d[0] == 'P' && (d[1] == '6' || d[1] == '5')) {
        size_t at = 2; std::string t;
        uint32_t vals[3];
        for (int k = 0; k < 3; ++k) { if (!pnm_token(d, at, t)) { err = "truncated PNM header"; return false; } vals[k] = static_cast<uint32_t>(std::strtoul(t.c_str(), nullptr, 10)); }
        ++at;   // the single whitespace after maxval
        const uint32_t ch = d[1] == '6' ? 3 : 1;
        // dimensions are bounded BEFORE any size arithmetic: header fields are untrusted and w * h * ch must not wrap
        if (vals[0] > kMaxDim || vals[1] > kMaxDim) { err = "image larger than 16384 x 16384"; return false; }
        if (vals[2] != 255 || vals[0] == 0 || vals[1] == 0 || d.size() < at + static_cast<size_t>(vals[0]) * vals[1] * ch) { err = "unsupported PNM (8-bit binary only)"; return false; }
        img.w = vals[0]; img.h = vals[1]; img.rgba8.resize(4ull * img.w * img.h);
        for (size_t i = 0; i < static_cast<size_t>(img.w) * img.h; ++i) {
            const uint8_t* px = d.data() + at + i * ch;
            img.rgba8[4 * i] = px[0]; img.rgba8[4 * i + 1] = ch == 3 ? px[1] : px[0]; img.rgba8[4 * i + 2] = ch == 3 ? px[2] : px[0]; img.rgba8[4 * i + 3] = 255;
        }
        return true;
    }
    if (d.size() >= 2 && d[0] == 'P' && (d[1] == 'F' || d[1] == 'f')) {
        size_t at = 2; std::string t;
        if (!pnm_token(d, at, t)) { err = "truncated PFM header"; return false; }
        const uint32_t w = static_cast<uint32_t>(std::strtoul(t.c_str(), nullptr, 10));
        if (!pnm_token(d, at, t)) { err = "truncated PFM header"; return false; }
        const uint32_t h = static_cast<uint32_t>(std::strtoul(t.c_str(), nullptr, 10));
        if (!pnm_token(d, at, t)) { err = "truncated PFM header"; return false; }
        const double scale = std::strtod(t.c_str(), nullptr);
        ++at;
        const uint32_t ch = d[1] == 'F' ? 3 : 1;
        if (w > kMaxDim || h > kMaxDim) { err = "image larger than 16384 x 16384"; return false; }
        if (scale == 0 || !w || !h || d.size() < at + 4ull * w * h * ch) { err = "truncated or malformed PFM"; return false; }
        const bool bigEndian = scale > 0;      // the sign of the scale line is the byte order of the samples
        img.w = w; img.h = h; img.isFloat = true; img.rgba32f.resize(4ull * w * h);
        for (uint32_t y = 0; y < h; ++y)   // PFM rows run bottom to top
            for (uint32_t x = 0; x < w; ++x) {
                float px[3] = { 0, 0, 0 };
                unsigned char raw[12];
                std::memcpy(raw, d.data() + at + 4ull * ch * (static_cast<size_t>(h - 1 - y) * w + x), 4ull * ch);
                if (bigEndian)
                    for (uint32_t c = 0; c < ch; ++c) { std::swap(raw[4 * c], raw[4 * c + 3]); std::swap(raw[4 * c + 1], raw[4 * c + 2]); }
                std::memcpy(px, raw, 4ull * ch);
                float* o = img.rgba32f.data() + 4ull * (static_cast<size_t>(y) * w + x);
                o[0] = px[0]; o[1] = ch == 3 ? px[1] : px[0]; o[2] = ch == 3 ? px[2] : px[0]; o[3] = 1.0f;
            }
        return true;
    }
    if (d.size() >= 54 && d[0] == 'B' && d[1] == 'M') {
        auto u32 = [&](size_t o) { uint32_t v; std::memcpy(&v, d.data() + o, 4); return v; };
        auto i32 = [&](size_t o) { int32_t v; std::memcpy(&v, d.data() + o, 4); return v; };
        const uint32_t off = u32(10); const int32_t w = i32(18), hh = i32(22);
        uint16_t bpp; std::memcpy(&bpp, d.data() + 28, 2);
        const uint32_t comp = u32(30);
        if (w <= 0 || hh == 0 || (bpp != 24 && bpp != 32) || (comp != 0 && comp != 3)) { err = "unsupported BMP (24 / 32 bit uncompressed only)"; return false; }
        // |hh| without negating INT_MIN; both dimensions bounded before off + stride * h is formed
        const int64_t h64 = hh < 0 ? -static_cast<int64_t>(hh) : static_cast<int64_t>(hh);
        if (w > static_cast<int32_t>(kMaxDim) || h64 > static_cast<int64_t>(kMaxDim)) { err = "image larger than 16384 x 16384"; return false; }
        const uint32_t h = static_cast<uint32_t>(h64);
        const size_t stride = (static_cast<size_t>(w) * (bpp / 8) + 3) & ~size_t(3);
        if (d.size() < static_cast<size_t>(off) + stride * h) { err = "truncated BMP"; return false; }
        img.w = static_cast<uint32_t>(w); img.h = h; img.rgba8.resize(4ull * img.w * h);
        for (uint32_t y = 0; y < h; ++y) {
            const uint8_t* row = d.data() + off + stride * (hh < 0 ? y : h - 1 - y);
            for (uint32_t x = 0; x < img.w; ++x) {
                const uint8_t* px = row + static_cast<size_t>(x) * (bpp / 8);
                uint8_t* o = img.rgba8.data() + 4ull * (static_cast<size_t>(y) * img.w + x);
                o[0] = px[2]; o[1] = px[1]; o[2] = px[0]; o[3] = bpp == 32 ? px[3] : 255;
            }
        }
        return true;
    }
    if (d.size() >= 18 && (d[2] == 2 || d[2] == 3) && d[1] == 0) {   // TGA, uncompressed true colour / grey
        const uint32_t idLen = d[0];
        uint16_t w, h; std::memcpy(&w, d.data() + 12, 2); std::memcpy(&h, d.data() + 14, 2);
        const uint32_t bpp = d[16]; const bool topDown = (d[17] & 0x20) != 0;
        const uint32_t ch = bpp / 8;
        if (!w || !h || (d[2] == 2 && ch != 3 && ch != 4) || (d[2] == 3 && ch != 1) || d.size() < 18 + idLen + static_cast<size_t>(w) * h * ch) { err = "unsupported TGA (uncompressed 8 / 24 / 32 bit only)"; return false; }
        img.w = w; img.h = h; img.rgba8.resize(4ull * w * h);
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < w; ++x) {
                const uint8_t* px = d.data() + 18 + idLen + (static_cast<size_t>(topDown ? y : h - 1 - y) * w + x) * ch;
                uint8_t* o = img.rgba8.data() + 4ull * (static_cast<size_t>(y) * w + x);
                if (ch == 1) { o[0] = o[1] = o[2] = px[0]; o[3] = 255; }
                else { o[0] = px[2]; o[1] = px[1]; o[2] = px[0]; o[3] = ch == 4 ? px[3] : 255; }
            }
        return true;
    }
    err = "unsupported image format (PNG, JPEG, PPM / PGM / PFM / BMP / TGA uncompressed, EXR)";
    return false;
}
} // namespace

bool decode_any(const uint8_t* data, size_t bytes, Image& img, std::string& err) {
    try { return decode_by_magic(Bytes{ data, bytes }, img, err); }
    catch (const std::bad_alloc&) { err = "out of memory for the image"; return false; }
}

} // namespace gfx_img
