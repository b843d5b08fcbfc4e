// bc_host.cpp -- gfxexp_amd/csrc/bc/bc_decode.hip.h compiled for the host: the decode functions the expansion kernels call, run
// on the CPU so that every format is checked against tools/dds_convert.py without a GPU (tests/bc_host.py builds and loads it).
#include <cstdint>
#include "bc/bc_decode.hip.h"

using namespace gfx::bc;

template <uint32_t F>
static void decode_image(const uint8_t* blocks, uint32_t w, uint32_t h, uint32_t* out) {
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) out[static_cast<uint64_t>(y) * w + x] = image_texel<F>(blocks, w, x, y);
}

// blocks: ceil(w / 4) * ceil(h / 4) blocks, row-major; out: w * h RGBA8 texels.  Returns 1 for an unknown format.
extern "C" int bc_host_decode(uint32_t format, const uint8_t* blocks, uint32_t w, uint32_t h, uint32_t* out) {
    switch (format) {
    case kBC1: decode_image<kBC1>(blocks, w, h, out); return 0;
    case kBC2: decode_image<kBC2>(blocks, w, h, out); return 0;
    case kBC3: decode_image<kBC3>(blocks, w, h, out); return 0;
    case kBC4U: decode_image<kBC4U>(blocks, w, h, out); return 0;
    case kBC4S: decode_image<kBC4S>(blocks, w, h, out); return 0;
    case kBC5U: decode_image<kBC5U>(blocks, w, h, out); return 0;
    case kBC5S: decode_image<kBC5S>(blocks, w, h, out); return 0;
    case kBC7: decode_image<kBC7>(blocks, w, h, out); return 0;
    default: return 1;
    }
}

extern "C" uint32_t bc_host_block_bytes(uint32_t format) { return block_bytes(format); }
