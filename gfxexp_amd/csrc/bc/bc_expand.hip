// bc_expand.hip -- block-compressed textures expanded on the device into the texel formats the software tex2DLod samples
// (texture.hip.h), and the table of resident block buffers behind gfx_texture_set_bc (bc_textures.h).
//
// k_bc_expand<BC, CH>: one lane per 4 x 4 block.  A lane loads its block with one 8- or 16-byte load (contiguous across the wave),
// decodes the header once (bc_decode.hip.h) and stores four rows; lanes of a wave hold neighbouring blocks of one block row, so a
// row store of the wave covers one contiguous segment (64 lanes x 16 bytes for RGBA8).  CH is the channel count of the pool texel:
// R8 / RG8 keep the first one / two channels of the RGBA8 texel, the host loader's rule for 8-bit images; sRGB and UNORM store the
// same bytes.  The pool packs rows tightly, so whole-row vector stores are aligned only when width is a multiple of four; any other
// width takes the per-texel path, which also clips the partial blocks at the right edge.  Rows below `height` are skipped in both.
#include <map>
#include <mutex>
#include <utility>
#include "../internal.h"
#include "bc_decode.hip.h"
#include "bc_textures.h"

namespace gfx {

#define GFX_BC_SAME(a, b) (static_cast<uint32_t>(a) == static_cast<uint32_t>(b))
static_assert(GFX_BC_SAME(GFX_BC1, bc::kBC1) && GFX_BC_SAME(GFX_BC2, bc::kBC2) && GFX_BC_SAME(GFX_BC3, bc::kBC3) && GFX_BC_SAME(GFX_BC4_UNORM, bc::kBC4U) &&
              GFX_BC_SAME(GFX_BC4_SNORM, bc::kBC4S) && GFX_BC_SAME(GFX_BC5_UNORM, bc::kBC5U) && GFX_BC_SAME(GFX_BC5_SNORM, bc::kBC5S) && GFX_BC_SAME(GFX_BC7, bc::kBC7),
              "bc::Format restates enum gfx_bc_format");
#undef GFX_BC_SAME

template <uint32_t CH> struct BcStore;
template <> struct BcStore<4> {
    static __device__ void row(uint8_t* p, uint32_t t0, uint32_t t1, uint32_t t2, uint32_t t3) { *reinterpret_cast<uint4*>(p) = make_uint4(t0, t1, t2, t3); }
    static __device__ void texel(uint8_t* p, uint32_t t) { *reinterpret_cast<uint32_t*>(p) = t; }
};
template <> struct BcStore<2> {
    static __device__ void row(uint8_t* p, uint32_t t0, uint32_t t1, uint32_t t2, uint32_t t3) {
        *reinterpret_cast<uint2*>(p) = make_uint2((t0 & 0xFFFFu) | (t1 << 16), (t2 & 0xFFFFu) | (t3 << 16));
    }
    static __device__ void texel(uint8_t* p, uint32_t t) { *reinterpret_cast<uint16_t*>(p) = static_cast<uint16_t>(t); }
};
template <> struct BcStore<1> {
    static __device__ void row(uint8_t* p, uint32_t t0, uint32_t t1, uint32_t t2, uint32_t t3) {
        *reinterpret_cast<uint32_t*>(p) = (t0 & 0xFFu) | ((t1 & 0xFFu) << 8) | ((t2 & 0xFFu) << 16) | (t3 << 24);
    }
    static __device__ void texel(uint8_t* p, uint32_t t) { *p = static_cast<uint8_t>(t); }
};

template <uint32_t BC, uint32_t CH>
__global__ __launch_bounds__(256) void k_bc_expand(const uint8_t* __restrict__ blocks, uint32_t width, uint32_t height, uint32_t blocksPerRow,
                                                   uint32_t numBlocks, uint8_t* __restrict__ out) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= numBlocks) return;
    uint64_t lo, hi = 0;
    if (bc::block_bytes(BC) == 8u) lo = reinterpret_cast<const uint64_t*>(blocks)[b];
    else { const ulonglong2 v = reinterpret_cast<const ulonglong2*>(blocks)[b]; lo = v.x; hi = v.y; }
    const bc::Decoder<BC> d(lo, hi);
    const uint32_t by = b / blocksPerRow, bx = b - by * blocksPerRow;
    const uint32_t x0 = bx * 4u, y0 = by * 4u;
    if ((width & 3u) == 0u) {
#pragma unroll
        for (uint32_t r = 0; r < 4u; ++r) {
            if (y0 + r >= height) break;
            BcStore<CH>::row(out + (static_cast<size_t>(y0 + r) * width + x0) * CH, d.texel(4u * r), d.texel(4u * r + 1u), d.texel(4u * r + 2u), d.texel(4u * r + 3u));
        }
    }
    else {
#pragma unroll
        for (uint32_t r = 0; r < 4u; ++r) {
            if (y0 + r >= height) break;
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k)
                if (x0 + k < width) BcStore<CH>::texel(out + (static_cast<size_t>(y0 + r) * width + x0 + k) * CH, d.texel(4u * r + k));
        }
    }
}

template <uint32_t BC>
static void launch_format(hipStream_t stream, const void* dBlocks, uint32_t width, uint32_t height, uint32_t format, void* dTexels) {
    const uint32_t perRow = (width + 3u) / 4u, n = perRow * ((height + 3u) / 4u);   // <= 4096 * 4096
    const dim3 grid((n + 255u) / 256u), block(256);
    const uint8_t* in = static_cast<const uint8_t*>(dBlocks);
    uint8_t* out = static_cast<uint8_t*>(dTexels);
    switch (format) {
    case GFX_TEX_RGBA8_SRGB: case GFX_TEX_RGBA8_UNORM: hipLaunchKernelGGL((k_bc_expand<BC, 4>), grid, block, 0, stream, in, width, height, perRow, n, out); break;
    case GFX_TEX_RG8_UNORM: hipLaunchKernelGGL((k_bc_expand<BC, 2>), grid, block, 0, stream, in, width, height, perRow, n, out); break;
    case GFX_TEX_R8_UNORM: hipLaunchKernelGGL((k_bc_expand<BC, 1>), grid, block, 0, stream, in, width, height, perRow, n, out); break;
    default: throw HipError("bc_expand: a block-compressed texture expands into an 8-bit format");
    }
    GFX_HIP(hipGetLastError());
}

void bc_expand_launch(hipStream_t stream, uint32_t bcFormat, const void* dBlocks, uint32_t width, uint32_t height, uint32_t format, void* dTexels) {
    if (width == 0 || height == 0 || width > 16384 || height > 16384) throw HipError("bc_expand: bad size");
    switch (bcFormat) {
    case GFX_BC1: launch_format<bc::kBC1>(stream, dBlocks, width, height, format, dTexels); break;
    case GFX_BC2: launch_format<bc::kBC2>(stream, dBlocks, width, height, format, dTexels); break;
    case GFX_BC3: launch_format<bc::kBC3>(stream, dBlocks, width, height, format, dTexels); break;
    case GFX_BC4_UNORM: launch_format<bc::kBC4U>(stream, dBlocks, width, height, format, dTexels); break;
    case GFX_BC4_SNORM: launch_format<bc::kBC4S>(stream, dBlocks, width, height, format, dTexels); break;
    case GFX_BC5_UNORM: launch_format<bc::kBC5U>(stream, dBlocks, width, height, format, dTexels); break;
    case GFX_BC5_SNORM: launch_format<bc::kBC5S>(stream, dBlocks, width, height, format, dTexels); break;
    case GFX_BC7: launch_format<bc::kBC7>(stream, dBlocks, width, height, format, dTexels); break;
    default: throw HipError("bc_expand: unknown block-compressed format");
    }
}

// ---------------------------------------------------------------- resident blocks, keyed by (context, slot)
namespace {
struct BcEntry { uint32_t bcFormat = 0; void* dBlocks = nullptr; size_t bytes = 0; };
std::mutex g_bcMutex;
std::map<std::pair<const Context*, uint32_t>, BcEntry> g_bcTextures;
}

void bc_texture_store(Context& ctx, uint32_t texSlot, uint32_t bcFormat, const void* blocks, size_t bytes) {
    BcEntry e;
    e.bcFormat = bcFormat; e.bytes = bytes;
    GFX_HIP(hipMalloc(&e.dBlocks, bytes));
    const hipError_t rc = hipMemcpy(e.dBlocks, blocks, bytes, hipMemcpyHostToDevice);
    if (rc != hipSuccess) { (void)hipFree(e.dBlocks); throw HipError(std::string("gfx_texture_set_bc: copying the blocks: ") + hipGetErrorString(rc)); }
    std::lock_guard<std::mutex> lock(g_bcMutex);
    BcEntry& slot = g_bcTextures[std::make_pair(&ctx, texSlot)];
    if (slot.dBlocks) (void)hipFree(slot.dBlocks);   // hipFree waits for an expansion that still reads it
    slot = e;
}

void bc_texture_forget(Context& ctx, uint32_t texSlot) {
    std::lock_guard<std::mutex> lock(g_bcMutex);
    auto it = g_bcTextures.find(std::make_pair(&ctx, texSlot));
    if (it == g_bcTextures.end()) return;
    (void)hipFree(it->second.dBlocks);
    g_bcTextures.erase(it);
}

bool bc_texture_is(const Context& ctx, uint32_t texSlot) {
    std::lock_guard<std::mutex> lock(g_bcMutex);
    return g_bcTextures.count(std::make_pair(&ctx, texSlot)) != 0;
}

void bc_textures_drop(Context& ctx) {
    std::lock_guard<std::mutex> lock(g_bcMutex);
    auto it = g_bcTextures.lower_bound(std::make_pair(static_cast<const Context*>(&ctx), 0u));
    while (it != g_bcTextures.end() && it->first.first == &ctx) { (void)hipFree(it->second.dBlocks); it = g_bcTextures.erase(it); }
}

void bc_texture_expand(Context& ctx, hipStream_t stream, uint32_t texSlot, uint32_t width, uint32_t height, uint32_t format, void* dTexels) {
    BcEntry e;
    {
        std::lock_guard<std::mutex> lock(g_bcMutex);
        auto it = g_bcTextures.find(std::make_pair(static_cast<const Context*>(&ctx), texSlot));
        if (it == g_bcTextures.end()) throw HipError("bc_texture_expand: the slot holds no blocks");
        e = it->second;
    }
    const size_t need = static_cast<size_t>((width + 3u) / 4u) * ((height + 3u) / 4u) * bc::block_bytes(e.bcFormat);
    if (need != e.bytes) throw HipError("bc_texture_expand: the slot's extent does not match its blocks");
    bc_expand_launch(stream, e.bcFormat, e.dBlocks, width, height, format, dTexels);
}

} // namespace gfx
