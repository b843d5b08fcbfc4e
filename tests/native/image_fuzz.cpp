// image_fuzz.cpp -- the image readers of the host layer alone under AddressSanitizer + UndefinedBehaviorSanitizer (host code only;
// built by tests/native/build_image_fuzz.py from image_codecs.cpp and image_formats.cpp into an executable of its own, never into
// the GPU library).
//
//   image_fuzz [-m N] <file>...   for the k-th file: every prefix, then N (default 2000) single-byte mutations drawn from xorshift64*
//                                 seeded with 0x9E3779B97F4A7C15 + k -- the schedule of tests/image_fixtures.py, which the in-library
//                                 tests replay.  Every input is handed over in a heap block of exactly its size and goes the way
//                                 gfxh_scene_load_texture sends it: a name ending in .dds / .DDS to dds_parse, every other to
//                                 decode_any (and, as a header-only pass, to gfx_img::info).
// Prints one line per file: "<name> prefixes <decoded> <refused> mutations <decoded> <refused> crc <CRC-32 of what the whole file
// decodes to, 8 hex digits>" -- the bytes of the one decoded buffer, or level 0 of a .dds after the BGRA swap.  Exits 1 if a decode
// reports a side outside 1 .. 16384, anything but one buffer of 4 w h elements, or a DDS level 0 that ends after the file.  A memory
// error ends the process through the sanitizer.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>
#include "../../gfxexp_amd/csrc/host/image_codecs.h"
#include "../../gfxexp_amd/csrc/host/image_formats.h"

namespace {

struct XorShift {
    uint64_t s;
    uint64_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return s * 0x2545F4914F6CDD1Dull; }
};

bool g_failed = false;

uint32_t crc32(const void* data, size_t n) {   // the CRC-32 of zlib.crc32 (reflected 0xEDB88320)
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) {
        c ^= static_cast<const uint8_t*>(data)[i];
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    }
    return ~c;
}

void bad(const char* what, uint32_t w, uint32_t h, size_t n) {
    std::fprintf(stderr, "bad result (%s): %u x %u, %zu\n", what, w, h, n);
    g_failed = true;
}

// 1 decoded, 0 refused; *crc, when asked for: the checksum of what was decoded
int run_one(bool dds, const uint8_t* data, size_t n, uint32_t* crc) {
    std::unique_ptr<uint8_t[]> exact(new uint8_t[n ? n : 1]);
    if (n) std::memcpy(exact.get(), data, n);
    std::string err;
    if (dds) {
        gfxh_dds_info info;
        if (!gfx_img::dds_parse(exact.get(), n, info, err)) return 0;
        if (info.width == 0 || info.height == 0 || info.width > gfx_img::kMaxDim || info.height > gfx_img::kMaxDim) bad("dds extent", info.width, info.height, n);
        if (info.dataOffset > n || info.dataBytes > n - info.dataOffset) { bad("dds level 0 ends after the file", info.width, info.height, n); return 1; }
        if (crc) {
            std::vector<uint8_t> level0(exact.get() + info.dataOffset, exact.get() + info.dataOffset + info.dataBytes);
            if (!info.isBlockCompressed && info.isBGRA) for (size_t i = 0; i + 3 < level0.size(); i += 4) std::swap(level0[i], level0[i + 2]);
            *crc = crc32(level0.data(), level0.size());
        }
        return 1;
    }
    gfx_img::Info head;
    gfx_img::info(exact.get(), n, head, err);
    gfx_img::Image img;
    if (!gfx_img::decode_any(exact.get(), n, img, err)) return 0;
    const size_t want = 4ull * img.w * img.h;
    if (img.w == 0 || img.h == 0 || img.w > gfx_img::kMaxDim || img.h > gfx_img::kMaxDim) bad("extent", img.w, img.h, n);
    if (img.isFloat ? (img.rgba32f.size() != want || !img.rgba8.empty()) : (img.rgba8.size() != want || !img.rgba32f.empty())) bad("buffers", img.w, img.h, img.rgba8.size() + img.rgba32f.size());
    if (crc) *crc = img.isFloat ? crc32(img.rgba32f.data(), 4 * img.rgba32f.size()) : crc32(img.rgba8.data(), img.rgba8.size());
    return 1;
}

} // namespace

int main(int argc, char** argv) {
    int first = 1, numMutations = 2000;
    if (argc > 2 && std::strcmp(argv[1], "-m") == 0) { numMutations = std::atoi(argv[2]); first = 3; }
    for (int k = first; k < argc; ++k) {
        std::vector<uint8_t> file;
        FILE* f = std::fopen(argv[k], "rb");
        if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[k]); return 2; }
        uint8_t buf[4096];
        for (size_t got; (got = std::fread(buf, 1, sizeof(buf), f)) > 0;) file.insert(file.end(), buf, buf + got);
        std::fclose(f);
        if (file.empty()) { std::fprintf(stderr, "%s is empty\n", argv[k]); return 2; }
        const bool dds = gfx_img::is_dds_path(argv[k]);
        uint32_t crc = 0;
        if (!run_one(dds, file.data(), file.size(), &crc)) { std::fprintf(stderr, "%s itself is refused\n", argv[k]); return 2; }
        int prefix[2] = { 0, 0 }, mutated[2] = { 0, 0 };
        for (size_t n = 0; n < file.size(); ++n) ++prefix[run_one(dds, file.data(), n, nullptr)];
        XorShift rng{ 0x9E3779B97F4A7C15ull + static_cast<uint64_t>(k - first) };
        for (int m = 0; m < numMutations; ++m) {
            const size_t pos = static_cast<size_t>((rng.next() >> 16) % file.size());
            uint8_t val = static_cast<uint8_t>((rng.next() >> 24) & 255u);
            if (val == file[pos]) val ^= 0xFF;
            const uint8_t keep = file[pos];
            file[pos] = val;
            ++mutated[run_one(dds, file.data(), file.size(), nullptr)];
            file[pos] = keep;
        }
        const char* slash = std::strrchr(argv[k], '/');
        std::printf("%s prefixes %d %d mutations %d %d crc %08x\n", slash ? slash + 1 : argv[k], prefix[1], prefix[0], mutated[1], mutated[0], crc);
    }
    return g_failed ? 1 : 0;
}
