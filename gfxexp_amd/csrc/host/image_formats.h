// image_formats.h -- the readers of the uncompressed image formats and of OpenEXR, the DDS header parser, and the dispatch by magic
// over them and the PNG / JPEG readers of image_codecs.h.  Same contract as image_codecs.h: plain C++17, no HIP header, no global
// state, nothing throws -- so the translation unit builds alone for the sanitizer driver in tests/native/image_fuzz.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include "../../../include/gfxexp_host.h"

namespace gfx_img {

// Decoded image: 8-bit RGBA (stbi_load(..., 4) in the reference, common_host.cpp:1211-1226) or float RGBA (.pfm).
struct Image { uint32_t w = 0, h = 0; bool isFloat = false; std::vector<uint8_t> rgba8; std::vector<float> rgba32f; };

// By magic, not by extension: PNG and JPEG (image_codecs.cpp: the bytes stbi_load(..., 4) gives the reference, common_host.cpp:1210-1229),
// OpenEXR, and the uncompressed formats binary PPM / PGM (8 bit), PFM, BMP 24 / 32 bit, TGA types 2 / 3 (24 / 32 / 8 bit).
// No third-party decoder in this build.  false + err (without the file's name, which the caller knows) on anything refused.
bool decode_any(const uint8_t* data, size_t bytes, Image& img, std::string& err);

// dds::load (common/dds_loader.cpp:207-346) as far as the header goes; every read is checked against `bytes` first.  `info` is
// zeroed, then filled; false + err when the file is refused.
bool dds_parse(const uint8_t* data, size_t bytes, gfxh_dds_info& info, std::string& err);

// the one extension test of the host layer (case-sensitive; a .dds file is named ".dds" or ".DDS", common_host.cpp:1185-1186)
inline bool has_ext(const char* path, const char* ext) {
    const size_t n = std::strlen(path), m = std::strlen(ext);
    return n >= m && std::strcmp(path + n - m, ext) == 0;
}
inline bool is_dds_path(const char* path) { return has_ext(path, ".dds") || has_ext(path, ".DDS"); }

} // namespace gfx_img
