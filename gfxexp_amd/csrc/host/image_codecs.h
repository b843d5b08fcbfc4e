// image_codecs.h -- PNG and JPEG readers and a PNG writer of the host layer (plain C++17: no HIP header, no global state, so the
// translation unit also builds alone for the sanitizer driver in tests/native/image_fuzz.cpp; image_formats.h holds the other readers).
//
// Output contract of both readers: exactly the bytes stbi_load(file, &w, &h, &n, 4) of the reference's ext/stb_image.h (v2.25)
// returns -- 8-bit RGBA, row 0 first -- plus n, the channel count of the file.  DESIGN.md section 13 lists what that pins.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace gfx_img {

constexpr uint32_t kMaxDim = 16384;      // TexDimInfo packs 14 bits per dimension: every reader and the scene container refuse a larger one before any arithmetic

enum Kind : uint32_t { kKindNone = 0, kKindPng = 1, kKindJpeg = 2 };

struct Info { uint32_t width = 0, height = 0, channels = 0, kind = kKindNone; };

// PNG signature / FF D8 FF at the start of the file
Kind sniff(const uint8_t* data, size_t bytes);

// Header only (PNG: up to the first IDAT, because a tRNS chunk changes the channel count; JPEG: up to the frame header).
bool png_info(const uint8_t* data, size_t bytes, Info& info, std::string& err);
bool jpeg_info(const uint8_t* data, size_t bytes, Info& info, std::string& err);

// Whole image -> rgba (4 * width * height bytes).  false + err on anything refused; never throws.
bool png_decode(const uint8_t* data, size_t bytes, Info& info, std::vector<uint8_t>& rgba, std::string& err);
bool jpeg_decode(const uint8_t* data, size_t bytes, Info& info, std::vector<uint8_t>& rgba, std::string& err);

// sniff + the matching reader; a file of neither kind is refused
bool info(const uint8_t* data, size_t bytes, Info& info, std::string& err);
bool decode(const uint8_t* data, size_t bytes, Info& info, std::vector<uint8_t>& rgba, std::string& err);

// 8-bit RGBA -> PNG file bytes (colour type 6, filter 0 on every row, one zlib stream of fixed-Huffman blocks with a short
// hash-chain match search, CRC-32 per chunk, Adler-32 of the stream).
bool png_encode_rgba8(const uint8_t* rgba, uint32_t width, uint32_t height, std::vector<uint8_t>& file, std::string& err);

// zlib stream (RFC 1950 / 1951) -> exactly `want` bytes; false on any malformed input.  Also inflates the ZIP chunks of OpenEXR.
bool inflate_zlib(const uint8_t* src, size_t n, std::vector<uint8_t>& out, size_t want);

} // namespace gfx_img
