// image_output.cpp -- the output chain of the host layer: the tone mapper and the PPM / BMP / PNG / PFM / EXR writers.
#include <cstdio>
#include <cstring>
#include "host_scene.h"
#include "image_codecs.h"
#include "image_formats.h"

using gfx_host::host_error;
using gfx_img::has_ext;

// ---------------------------------------------------------------- output chain
// saveImage(float4 -> 8-bit) of common/common_host.cpp:2859-2897: tone map on the luminance, sRGB gamma, quantise.
extern "C" void gfxh_tonemap_sdr(uint32_t width, uint32_t height, const float* rgba, const gfxh_sdr_config* cfg, uint32_t* out) {
    for (uint32_t y = 0; y < height; ++y) {
        const uint32_t sy = cfg->flipY ? (height - 1 - y) : y;
        for (uint32_t x = 0; x < width; ++x) {
            const float* src = rgba + 4 * (static_cast<size_t>(sy) * width + x);
            float r = src[0], g = src[1], b = src[2], a = src[3];
            if (cfg->alphaForOverride >= 0.0f) a = cfg->alphaForOverride;
            if (cfg->applyToneMap) {
                if (!(std::isfinite(r) && std::isfinite(g) && std::isfinite(b))) { r = 0.0f; g = 0.0f; b = 0.0f; }
                const float lum = 0.2126729f * r + 0.7151522f * g + 0.0721750f * b;      // sRGB_calcLuminance
                const float lumT = 1 - std::exp(-(cfg->brightnessScale * lum));           // simpleToneMap_s
                const float s = lum > 0.0f ? lumT / lum : 0.0f;
                r *= s; g *= s; b *= s;
            }
            if (cfg->apply_sRGB_gammaCorrection) {                                        // sRGB_gamma_s
                auto gamma = [](float v) { return v <= 0.0031308f ? 12.92f * v : 1.055f * std::pow(v, 1 / 2.4f) - 0.055f; };
                r = gamma(r); g = gamma(g); b = gamma(b);
            }
            auto q = [](float v) { return v > 0.0f ? std::min<uint32_t>(static_cast<uint32_t>(std::min(v * 255, 4.0e9f)), 255u) : 0u; };
            out[static_cast<size_t>(y) * width + x] = q(r) | (q(g) << 8) | (q(b) << 16) | (q(a) << 24);
        }
    }
}


extern "C" int gfxh_save_image_sdr(const char* path, uint32_t width, uint32_t height, const float* rgba, const gfxh_sdr_config* cfg) {
    std::vector<uint32_t> px(static_cast<size_t>(width) * height);
    gfxh_tonemap_sdr(width, height, rgba, cfg, px.data());
    FILE* f = std::fopen(path, "wb");
    if (!f) { host_error() = std::string("cannot open ") + path; return 1; }
    if (has_ext(path, ".ppm")) {
        std::fprintf(f, "P6\n%u %u\n255\n", width, height);
        for (uint32_t p : px) { const unsigned char c[3] = { static_cast<unsigned char>(p), static_cast<unsigned char>(p >> 8), static_cast<unsigned char>(p >> 16) }; std::fwrite(c, 1, 3, f); }
    }
    else if (has_ext(path, ".bmp")) {
        const uint32_t rowBytes = (3 * width + 3) & ~3u, dataBytes = rowBytes * height;
        unsigned char hdr[54] = { 'B', 'M' };
        auto put32 = [&](int o, uint32_t v) { hdr[o] = v & 255; hdr[o + 1] = (v >> 8) & 255; hdr[o + 2] = (v >> 16) & 255; hdr[o + 3] = (v >> 24) & 255; };
        put32(2, 54 + dataBytes); put32(10, 54); put32(14, 40); put32(18, width); put32(22, height);
        hdr[26] = 1; hdr[28] = 24; put32(34, dataBytes);
        std::fwrite(hdr, 1, 54, f);
        std::vector<unsigned char> row(rowBytes, 0);
        for (uint32_t y = 0; y < height; ++y) {                       // bottom-up, BGR
            const uint32_t* src = px.data() + static_cast<size_t>(height - 1 - y) * width;
            for (uint32_t x = 0; x < width; ++x) { row[3 * x] = (src[x] >> 16) & 255; row[3 * x + 1] = (src[x] >> 8) & 255; row[3 * x + 2] = src[x] & 255; }
            std::fwrite(row.data(), 1, rowBytes, f);
        }
    }
    else if (has_ext(path, ".png")) {                                    // stbi_write_png of saveImage (common_host.cpp:2715-2720): 8-bit RGBA, top row first
        std::vector<uint8_t> file; std::string err;
        // px holds R | G << 8 | B << 16 | A << 24: on the little-endian hosts this library builds for that is R, G, B, A in memory
        if (!gfx_img::png_encode_rgba8(reinterpret_cast<const uint8_t*>(px.data()), width, height, file, err)) { std::fclose(f); host_error() = "gfxh_save_image_sdr: " + err; return 1; }
        if (std::fwrite(file.data(), 1, file.size(), f) != file.size()) { std::fclose(f); host_error() = std::string("gfxh_save_image_sdr: short write to ") + path; return 1; }
    }
    else { std::fclose(f); host_error() = "gfxh_save_image_sdr: .bmp or .ppm or .png"; return 1; }
    std::fclose(f);
    return 0;
}

// fp32 -> fp16, round to nearest even (what tinyexr's float_to_half_full does for the requested HALF pixel type)
static uint16_t float_to_half(float v) {
    uint32_t x; std::memcpy(&x, &v, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    const uint32_t mag = x & 0x7FFFFFFFu;
    if (mag >= 0x7F800000u) return static_cast<uint16_t>(sign | 0x7C00u | (mag > 0x7F800000u ? 0x200u : 0u));   // inf / NaN
    if (mag >= 0x477FF000u) return static_cast<uint16_t>(sign | 0x7C00u);                                        // rounds to >= 65520 -> inf
    if (mag < 0x33000001u) return static_cast<uint16_t>(sign);                                                   // below half of the smallest subnormal
    const int32_t e = static_cast<int32_t>(mag >> 23) - 127;
    uint32_t m = (mag & 0x7FFFFFu) | 0x800000u;
    uint32_t half;
    uint32_t shift;
    if (e < -14) { shift = static_cast<uint32_t>(13 + (-14 - e)); half = 0; }        // subnormal half
    else { shift = 13; half = static_cast<uint32_t>(e + 15) << 10; m &= 0x7FFFFFu; }
    const uint32_t q = m >> shift, rem = m & ((1u << shift) - 1u), halfway = 1u << (shift - 1);
    half += q;
    if (rem > halfway || (rem == halfway && (half & 1u))) ++half;                      // carries into the exponent correctly
    return static_cast<uint16_t>(sign | half);
}

// saveImageHDR (common_host.cpp:2762-2857): OpenEXR scanline file, channels A B G R stored as HALF.  The reference goes
// through tinyexr (ZIP-compressed); this writer emits the same pixels uncompressed (compression = NO_COMPRESSION).
static int save_exr(const char* path, uint32_t width, uint32_t height, float brightnessScale, const float* rgba, int flipY) {
    FILE* f = std::fopen(path, "wb");
    if (!f) { host_error() = std::string("cannot open ") + path; return 1; }
    std::vector<uint8_t> hdr;
    auto put = [&](const void* p, size_t n) { hdr.insert(hdr.end(), static_cast<const uint8_t*>(p), static_cast<const uint8_t*>(p) + n); };
    auto put_str = [&](const char* t) { put(t, std::strlen(t) + 1); };
    auto put_i32 = [&](int32_t v) { put(&v, 4); };
    auto put_f32 = [&](float v) { put(&v, 4); };
    const uint32_t magic = 20000630u, version = 2u;
    put(&magic, 4); put(&version, 4);
    put_str("channels"); put_str("chlist"); put_i32(4 * 18 + 1);
    for (const char* name : { "A", "B", "G", "R" }) { put_str(name); put_i32(1 /* HALF */); const uint8_t lin[4] = { 0, 0, 0, 0 }; put(lin, 4); put_i32(1); put_i32(1); }
    { const uint8_t z = 0; put(&z, 1); }
    put_str("compression"); put_str("compression"); put_i32(1); { const uint8_t c = 0; put(&c, 1); }
    put_str("dataWindow"); put_str("box2i"); put_i32(16); put_i32(0); put_i32(0); put_i32(static_cast<int32_t>(width) - 1); put_i32(static_cast<int32_t>(height) - 1);
    put_str("displayWindow"); put_str("box2i"); put_i32(16); put_i32(0); put_i32(0); put_i32(static_cast<int32_t>(width) - 1); put_i32(static_cast<int32_t>(height) - 1);
    put_str("lineOrder"); put_str("lineOrder"); put_i32(1); { const uint8_t c = 0; put(&c, 1); }
    put_str("pixelAspectRatio"); put_str("float"); put_i32(4); put_f32(1.0f);
    put_str("screenWindowCenter"); put_str("v2f"); put_i32(8); put_f32(0.0f); put_f32(0.0f);
    put_str("screenWindowWidth"); put_str("float"); put_i32(4); put_f32(1.0f);
    { const uint8_t z = 0; put(&z, 1); }
    std::fwrite(hdr.data(), 1, hdr.size(), f);
    const uint64_t rowBytes = 8ull + 4ull * 2ull * width;   // y, size, then A B G R planes of half
    uint64_t offset = hdr.size() + 8ull * height;
    for (uint32_t y = 0; y < height; ++y) { std::fwrite(&offset, 8, 1, f); offset += rowBytes; }
    std::vector<uint16_t> row(4ull * width);
    for (uint32_t y = 0; y < height; ++y) {
        const uint32_t sy = flipY ? (height - 1 - y) : y;
        const float* src = rgba + 4ull * static_cast<size_t>(sy) * width;
        for (uint32_t x = 0; x < width; ++x)
            for (int c = 0; c < 4; ++c) row[static_cast<size_t>(c) * width + x] = float_to_half(brightnessScale * src[4 * x + (3 - c)]);   // A, B, G, R planes
        const int32_t yy = static_cast<int32_t>(y), size = static_cast<int32_t>(8ull * width);
        std::fwrite(&yy, 4, 1, f); std::fwrite(&size, 4, 1, f);
        std::fwrite(row.data(), 2, row.size(), f);
    }
    std::fclose(f);
    return 0;
}

extern "C" int gfxh_save_image_hdr(const char* path, uint32_t width, uint32_t height, float brightnessScale, const float* rgba, int flipY) {
    if (has_ext(path, ".exr")) return save_exr(path, width, height, brightnessScale, rgba, flipY);
    if (!has_ext(path, ".pfm")) { host_error() = "gfxh_save_image_hdr: .exr or .pfm"; return 1; }
    FILE* f = std::fopen(path, "wb");
    if (!f) { host_error() = std::string("cannot open ") + path; return 1; }
    std::fprintf(f, "PF\n%u %u\n-1.0\n", width, height);              // little endian, rows bottom to top
    std::vector<float> row(3 * static_cast<size_t>(width));
    for (uint32_t y = 0; y < height; ++y) {
        const uint32_t top = height - 1 - y;                            // the image row this file row holds
        const uint32_t sy = flipY ? (height - 1 - top) : top;
        for (uint32_t x = 0; x < width; ++x)
            for (int c = 0; c < 3; ++c) row[3 * x + c] = brightnessScale * rgba[4 * (static_cast<size_t>(sy) * width + x) + c];
        std::fwrite(row.data(), sizeof(float), row.size(), f);
    }
    std::fclose(f);
    return 0;
}
