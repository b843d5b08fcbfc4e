// image_fuzz.cpp -- the PNG / JPEG readers alone under AddressSanitizer + UndefinedBehaviorSanitizer (host code only; built by
// tests/native/build_image_fuzz.py into an executable of its own, never into the GPU library).
//
//   image_fuzz <file>...     for the k-th file: every prefix, then 2000 single-byte mutations drawn from xorshift64* seeded with
//                            0x9E3779B97F4A7C15 + k -- the schedule of tests/image_fixtures.py, which the in-library test replays
//                            through the C ABI.  Every input is handed over in a heap block of exactly its size.
// Prints one line per file: "<name> prefixes <decoded> <refused> mutations <decoded> <refused>"; exits 1 if a decode reports a
// side above 16384 or a buffer of the wrong size.  A memory error ends the process through the sanitizer.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "../../gfxexp_amd/csrc/host/image_codecs.h"

namespace {

struct XorShift {
    uint64_t s;
    uint64_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return s * 0x2545F4914F6CDD1Dull; }
};

bool g_failed = false;

// 1 decoded, 0 refused
int run_one(const uint8_t* data, size_t n) {
    std::unique_ptr<uint8_t[]> exact(new uint8_t[n ? n : 1]);
    if (n) std::memcpy(exact.get(), data, n);
    gfx_img::Info head, info;
    std::vector<uint8_t> rgba;
    std::string err;
    gfx_img::info(exact.get(), n, head, err);
    if (!gfx_img::decode(exact.get(), n, info, rgba, err)) return 0;
    if (info.width == 0 || info.height == 0 || info.width > gfx_img::kMaxDim || info.height > gfx_img::kMaxDim || rgba.size() != 4ull * info.width * info.height) {
        std::fprintf(stderr, "bad result: %u x %u, %zu bytes\n", info.width, info.height, rgba.size());
        g_failed = true;
    }
    return 1;
}

} // namespace

int main(int argc, char** argv) {
    for (int k = 1; k < argc; ++k) {
        std::vector<uint8_t> file;
        FILE* f = std::fopen(argv[k], "rb");
        if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[k]); return 2; }
        uint8_t buf[4096];
        for (size_t got; (got = std::fread(buf, 1, sizeof(buf), f)) > 0;) file.insert(file.end(), buf, buf + got);
        std::fclose(f);
        if (file.empty()) { std::fprintf(stderr, "%s is empty\n", argv[k]); return 2; }
        int prefix[2] = { 0, 0 }, mutated[2] = { 0, 0 };
        for (size_t n = 0; n < file.size(); ++n) ++prefix[run_one(file.data(), n)];
        XorShift rng{ 0x9E3779B97F4A7C15ull + static_cast<uint64_t>(k - 1) };
        for (int m = 0; m < 2000; ++m) {
            const size_t pos = static_cast<size_t>((rng.next() >> 16) % file.size());
            uint8_t val = static_cast<uint8_t>((rng.next() >> 24) & 255u);
            if (val == file[pos]) val ^= 0xFF;
            const uint8_t keep = file[pos];
            file[pos] = val;
            ++mutated[run_one(file.data(), file.size())];
            file[pos] = keep;
        }
        const char* slash = std::strrchr(argv[k], '/');
        std::printf("%s prefixes %d %d mutations %d %d\n", slash ? slash + 1 : argv[k], prefix[1], prefix[0], mutated[1], mutated[0]);
    }
    return g_failed ? 1 : 0;
}
