// bc_decode.hip.h -- block-compressed texture formats BC1, BC2, BC3, BC4 (unsigned / signed), BC5 (unsigned / signed) and BC7:
// one texel of one 4 x 4 block -> RGBA8, packed r | g << 8 | b << 16 | a << 24.
//
// The reference leaves the decode to the texture unit (common/common_host.cpp:766-886 maps the BC format to an array type).  Here
// it is written arithmetic, and where the format specification leaves a choice the contract is tools/dds_convert.py:
//     BC1 palette (2 a + b) / 3, (a + b) / 2 with integer division; 3-colour index 3 = (0, 0, 0, 0); BC2 / BC3 colour always
//     four-colour; BC2 alpha nibble * 17; one-channel formats fill (v, v, v, 255), two-channel (x, y, 0, 255); the reserved BC7
//     mode decodes to (0, 0, 0, 0).
// BC3 alpha / BC4 / BC5 round floor(v + 0.5) of the interpolated value.  Unsigned: the integer form (2 num + d) / (2 d) equals the
// float64 expression of dds_convert._alpha_block for every endpoint pair and index.  Signed: exact rational rounding does NOT (53 of
// the 524 288 cases are .5 ties that the float64 evaluation lands just below), so the signed palette evaluates the same double
// expression in the same order; it needs IEEE double division and no contraction (the build's -ffp-contract=off).
//
// Plain C++17: no HIP intrinsics, tables as static constexpr arrays inside the functions (device code cannot refer to a
// namespace-scope host table, and a non-static one is copied into a private array per lane).  Every decoder splits into a header decoded once per block (the constructor) and texel(t), t = 4 y + x, so that an
// expansion kernel pays the header once per lane and a sampler can address single texels.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>          // the function attributes below; a host compiler needs no HIP header
#define GFX_BC_FN __host__ __device__ __forceinline__
#else
#define GFX_BC_FN inline
#endif

namespace gfx {
namespace bc {

// the values of enum gfx_bc_format (include/gfxexp.h)
enum Format : uint32_t { kBC1 = 0, kBC2 = 1, kBC3 = 2, kBC4U = 3, kBC4S = 4, kBC5U = 5, kBC5S = 6, kBC7 = 7, kNumFormats = 8 };

GFX_BC_FN uint32_t block_bytes(uint32_t format) { return format == kBC1 || format == kBC4U || format == kBC4S ? 8u : (format < kNumFormats ? 16u : 0u); }

GFX_BC_FN uint32_t pack_rgba(uint32_t r, uint32_t g, uint32_t b, uint32_t a) { return r | (g << 8) | (b << 16) | (a << 24); }

// ---------------------------------------------------------------- BC1 / BC2 / BC3 colour half: two RGB565 endpoints + sixteen 2-bit indices
struct ColorBlock {
    uint32_t pal0, pal1, pal2, pal3;
    uint32_t indices;
    GFX_BC_FN ColorBlock(uint64_t bits, bool fourColourOnly) {
        const uint32_t c0 = static_cast<uint32_t>(bits) & 0xFFFFu, c1 = static_cast<uint32_t>(bits >> 16) & 0xFFFFu;
        indices = static_cast<uint32_t>(bits >> 32);
        const uint32_t r0 = (c0 >> 11) & 31u, g0 = (c0 >> 5) & 63u, b0 = c0 & 31u;
        const uint32_t r1 = (c1 >> 11) & 31u, g1 = (c1 >> 5) & 63u, b1 = c1 & 31u;
        const uint32_t R0 = (r0 << 3) | (r0 >> 2), G0 = (g0 << 2) | (g0 >> 4), B0 = (b0 << 3) | (b0 >> 2);
        const uint32_t R1 = (r1 << 3) | (r1 >> 2), G1 = (g1 << 2) | (g1 >> 4), B1 = (b1 << 3) | (b1 >> 2);
        pal0 = pack_rgba(R0, G0, B0, 255u);
        pal1 = pack_rgba(R1, G1, B1, 255u);
        if (c0 > c1 || fourColourOnly) {
            pal2 = pack_rgba((2u * R0 + R1) / 3u, (2u * G0 + G1) / 3u, (2u * B0 + B1) / 3u, 255u);
            pal3 = pack_rgba((R0 + 2u * R1) / 3u, (G0 + 2u * G1) / 3u, (B0 + 2u * B1) / 3u, 255u);
        }
        else {
            pal2 = pack_rgba((R0 + R1) / 2u, (G0 + G1) / 2u, (B0 + B1) / 2u, 255u);
            pal3 = 0u;
        }
    }
    GFX_BC_FN uint32_t texel(uint32_t t) const {
        const uint32_t i = (indices >> (2u * t)) & 3u;
        return i == 0u ? pal0 : (i == 1u ? pal1 : (i == 2u ? pal2 : pal3));
    }
};

// ---------------------------------------------------------------- BC3 alpha / BC4 / one half of BC5: two 8-bit endpoints + sixteen 3-bit indices
GFX_BC_FN uint32_t snorm_to_byte(double v) {   // dds_convert._alpha_block: floor((v / 127 * 0.5 + 0.5) * 255 + 0.5), clipped
    const double s = (v / 127.0 * 0.5 + 0.5) * 255.0 + 0.5;
    const int32_t f = static_cast<int32_t>(s);   // s >= 0.5: truncation is floor
    return static_cast<uint32_t>(f < 0 ? 0 : (f > 255 ? 255 : f));
}

struct AlphaBlock {
    uint64_t palette;   // eight values, one byte each
    uint64_t indices;   // 48 bits
    GFX_BC_FN AlphaBlock(uint64_t bits, bool isSigned) {
        indices = bits >> 16;
        uint64_t pal = 0;
        if (!isSigned) {
            const uint32_t a0 = static_cast<uint32_t>(bits) & 0xFFu, a1 = static_cast<uint32_t>(bits >> 8) & 0xFFu;
            pal = a0 | (static_cast<uint64_t>(a1) << 8);
            if (a0 > a1) {
                for (uint32_t k = 1; k <= 6; ++k)
                    pal |= static_cast<uint64_t>((2u * ((7u - k) * a0 + k * a1) + 7u) / 14u) << (8u * (1u + k));
            }
            else {
                for (uint32_t k = 1; k <= 4; ++k)
                    pal |= static_cast<uint64_t>((2u * ((5u - k) * a0 + k * a1) + 5u) / 10u) << (8u * (1u + k));
                pal |= static_cast<uint64_t>(255u) << 56;   // index 6 = 0, index 7 = 255
            }
        }
        else {
            int32_t a0 = static_cast<int32_t>(static_cast<int8_t>(bits & 0xFFu)), a1 = static_cast<int32_t>(static_cast<int8_t>((bits >> 8) & 0xFFu));
            a0 = a0 < -127 ? -127 : a0;
            a1 = a1 < -127 ? -127 : a1;
            pal = snorm_to_byte(static_cast<double>(a0)) | (static_cast<uint64_t>(snorm_to_byte(static_cast<double>(a1))) << 8);
            if (a0 > a1) {
                for (int32_t k = 1; k <= 6; ++k)
                    pal |= static_cast<uint64_t>(snorm_to_byte(static_cast<double>((7 - k) * a0 + k * a1) / 7.0)) << (8 * (1 + k));
            }
            else {
                for (int32_t k = 1; k <= 4; ++k)
                    pal |= static_cast<uint64_t>(snorm_to_byte(static_cast<double>((5 - k) * a0 + k * a1) / 5.0)) << (8 * (1 + k));
                pal |= static_cast<uint64_t>(255u) << 56;   // index 6 = -127 -> 0, index 7 = 127 -> 255
            }
        }
        palette = pal;
    }
    GFX_BC_FN uint32_t texel(uint32_t t) const {
        const uint32_t i = static_cast<uint32_t>(indices >> (3u * t)) & 7u;
        return static_cast<uint32_t>(palette >> (8u * i)) & 0xFFu;
    }
};

// ---------------------------------------------------------------- BC7
// n <= 8 bits at bit `pos` of the 128-bit block (lo = bits 0..63)
GFX_BC_FN uint32_t bits128(uint64_t lo, uint64_t hi, uint32_t pos, uint32_t n) {
    const uint64_t v = pos < 64u ? ((lo >> pos) | (pos ? (hi << (64u - pos)) : 0ull)) : (hi >> (pos - 64u));
    return static_cast<uint32_t>(v) & ((1u << n) - 1u);
}

GFX_BC_FN uint32_t bc7_weight(uint32_t indexBits, uint32_t i) {
    static constexpr uint8_t w2[4] = { 0, 21, 43, 64 };
    static constexpr uint8_t w3[8] = { 0, 9, 18, 27, 37, 46, 55, 64 };
    static constexpr uint8_t w4[16] = { 0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64 };
    return indexBits == 2u ? w2[i & 3u] : (indexBits == 3u ? w3[i & 7u] : w4[i & 15u]);
}

GFX_BC_FN uint32_t bc7_partition2(uint32_t part) {   // bit t = subset of texel t
    static constexpr uint16_t table[64] = {
        0xCCCC, 0x8888, 0xEEEE, 0xECC8, 0xC880, 0xFEEC, 0xFEC8, 0xEC80,
        0xC800, 0xFFEC, 0xFE80, 0xE800, 0xFFE8, 0xFF00, 0xFFF0, 0xF000,
        0xF710, 0x008E, 0x7100, 0x08CE, 0x008C, 0x7310, 0x3100, 0x8CCE,
        0x088C, 0x3110, 0x6666, 0x366C, 0x17E8, 0x0FF0, 0x718E, 0x399C,
        0xAAAA, 0xF0F0, 0x5A5A, 0x33CC, 0x3C3C, 0x55AA, 0x9696, 0xA55A,
        0x73CE, 0x13C8, 0x324C, 0x3BDC, 0x6996, 0xC33C, 0x9966, 0x0660,
        0x0272, 0x04E4, 0x4E40, 0x2720, 0xC936, 0x936C, 0x39C6, 0x639C,
        0x9336, 0x9CC6, 0x817E, 0xE718, 0xCCF0, 0x0FCC, 0x7744, 0xEE22 };
    return table[part & 63u];
}

GFX_BC_FN uint32_t bc7_partition3(uint32_t part) {   // bits 2 t, 2 t + 1 = subset of texel t
    static constexpr uint32_t table[64] = {
        0xAA685050u, 0x6A5A5040u, 0x5A5A4200u, 0x5450A0A8u, 0xA5A50000u, 0xA0A05050u, 0x5555A0A0u, 0x5A5A5050u,
        0xAA550000u, 0xAA555500u, 0xAAAA5500u, 0x90909090u, 0x94949494u, 0xA4A4A4A4u, 0xA9A59450u, 0x2A0A4250u,
        0xA5945040u, 0x0A425054u, 0xA5A5A500u, 0x55A0A0A0u, 0xA8A85454u, 0x6A6A4040u, 0xA4A45000u, 0x1A1A0500u,
        0x0050A4A4u, 0xAAA59090u, 0x14696914u, 0x69691400u, 0xA08585A0u, 0xAA821414u, 0x50A4A450u, 0x6A5A0200u,
        0xA9A58000u, 0x5090A0A8u, 0xA8A09050u, 0x24242424u, 0x00AA5500u, 0x24924924u, 0x24499224u, 0x50A50A50u,
        0x500AA550u, 0xAAAA4444u, 0x66660000u, 0xA5A0A5A0u, 0x50A050A0u, 0x69286928u, 0x44AAAA44u, 0x66666600u,
        0xAA444444u, 0x54A854A8u, 0x95809580u, 0x96969600u, 0xA85454A8u, 0x80959580u, 0xAA141414u, 0x96960000u,
        0xAAAA1414u, 0xA05050A0u, 0xA0A5A5A0u, 0x96000000u, 0x40804080u, 0xA9A8A9A8u, 0xAAAAAA44u, 0x2A4A5254u };
    return table[part & 63u];
}

// anchor texels (their index is stored with one bit less): which = 0: second subset of a 2-subset partition,
// 1 / 2: second / third subset of a 3-subset partition
GFX_BC_FN uint32_t bc7_anchor(uint32_t which, uint32_t part) {
    static constexpr uint8_t table[3][64] = {
        { 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 2, 8, 2, 2, 8, 8, 15, 2, 8, 2, 2, 8, 8, 2, 2,
          15, 15, 6, 8, 2, 8, 15, 15, 2, 8, 2, 2, 2, 15, 15, 6, 6, 2, 6, 8, 15, 15, 2, 2, 15, 15, 15, 15, 15, 2, 2, 15 },
        { 3, 3, 15, 15, 8, 3, 15, 15, 8, 8, 6, 6, 6, 5, 3, 3, 3, 3, 8, 15, 3, 3, 6, 10, 5, 8, 8, 6, 8, 5, 15, 15,
          8, 15, 3, 5, 6, 10, 8, 15, 15, 3, 15, 5, 15, 15, 15, 15, 3, 15, 5, 5, 5, 8, 5, 10, 5, 10, 8, 13, 15, 12, 3, 3 },
        { 15, 8, 8, 3, 15, 15, 3, 8, 15, 15, 15, 15, 15, 15, 15, 8, 15, 8, 15, 3, 15, 8, 15, 8, 3, 15, 6, 10, 15, 15, 10, 8,
          15, 3, 15, 10, 10, 8, 9, 10, 6, 15, 8, 15, 3, 6, 6, 8, 15, 3, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 3, 15, 15, 8 } };
    return table[which][part & 63u];
}

struct Bc7Block {
    uint64_t lo, hi;
    // endpoints expanded to 8 bits per channel, subset s owns 2 s and 2 s + 1.  Subsets 0 and 1 share a 64-bit word per side and
    // are picked with a shift: a chain of selects over six members is turned into a run-time index into the object by the
    // compiler, which then keeps the whole decoder in memory instead of registers
    uint64_t first01, second01;              // endpoint 0 | endpoint 2 << 32, endpoint 1 | endpoint 3 << 32
    uint32_t ep4, ep5;
    uint32_t subsets;                        // 2 bits per texel
    uint32_t numSubsets;                     // 0: the reserved mode
    uint32_t anchor1, anchor2;               // 16 = none
    uint32_t rotation, indexSelection;
    uint32_t indexBits, indexBits2;          // indexBits2 = 0: one index per texel
    uint32_t indexStart, indexStart2;

    GFX_BC_FN Bc7Block(uint64_t lo_, uint64_t hi_) : lo(lo_), hi(hi_) {
        // per mode: subsets, partition bits, rotation bits, index-selection bits, colour bits, alpha bits, endpoint p-bits, shared p-bits,
        // index bits, second index bits
        static constexpr uint8_t modes[8][10] = {
            { 3, 4, 0, 0, 4, 0, 1, 0, 3, 0 }, { 2, 6, 0, 0, 6, 0, 0, 1, 3, 0 }, { 3, 6, 0, 0, 5, 0, 0, 0, 2, 0 }, { 2, 6, 0, 0, 7, 0, 1, 0, 2, 0 },
            { 1, 0, 2, 1, 5, 6, 0, 0, 2, 3 }, { 1, 0, 2, 0, 7, 8, 0, 0, 2, 2 }, { 1, 0, 0, 0, 7, 7, 1, 0, 4, 0 }, { 2, 6, 0, 0, 5, 5, 1, 0, 2, 0 } };
        first01 = second01 = 0ull; ep4 = ep5 = 0u;
        subsets = 0u; numSubsets = 0u; anchor1 = anchor2 = 16u; rotation = indexSelection = 0u;
        indexBits = 2u; indexBits2 = 0u; indexStart = indexStart2 = 0u;
        uint32_t mode = 0;
        while (mode < 8u && !((static_cast<uint32_t>(lo_) >> mode) & 1u)) ++mode;
        if (mode == 8u) return;
        const uint32_t ns = modes[mode][0], pb = modes[mode][1], rb = modes[mode][2], isb = modes[mode][3], cb = modes[mode][4], ab = modes[mode][5];
        const uint32_t epb = modes[mode][6], spb = modes[mode][7];
        numSubsets = ns; indexBits = modes[mode][8]; indexBits2 = modes[mode][9];
        uint32_t pos = mode + 1u;
        const uint32_t part = bits128(lo_, hi_, pos, pb); pos += pb;
        rotation = bits128(lo_, hi_, pos, rb); pos += rb;
        indexSelection = bits128(lo_, hi_, pos, isb); pos += isb;
        const uint32_t ne = 2u * ns;
        const uint32_t colourAt = pos, alphaAt = pos + 3u * ne * cb, pbitAt = alphaAt + ne * ab;
        indexStart = pbitAt + (epb ? ne : (spb ? 2u : 0u));
        indexStart2 = indexStart + 16u * indexBits - ns;
        const uint32_t cbits = cb + (epb | spb), abits = ab + (ab ? epb : 0u);
        // one endpoint, expanded to 8 bits per channel; written out six times below so that nothing is indexed at run time
        auto endpoint = [=](uint32_t e) -> uint32_t {
            if (e >= ne) return 0u;
            const uint32_t p = epb ? bits128(lo_, hi_, pbitAt + e, 1u) : (spb ? bits128(lo_, hi_, pbitAt + (e >> 1), 1u) : 0u);
            uint32_t px = 0u;
            for (uint32_t ch = 0; ch < 3u; ++ch) {
                uint32_t v = bits128(lo_, hi_, colourAt + (ch * ne + e) * cb, cb);
                if (epb | spb) v = (v << 1) | p;
                v = ((v << (8u - cbits)) | (v >> (2u * cbits - 8u))) & 0xFFu;
                px |= v << (8u * ch);
            }
            uint32_t a = 255u;
            if (ab) {
                a = bits128(lo_, hi_, alphaAt + e * ab, ab);
                if (epb) a = (a << 1) | p;
                a = ((a << (8u - abits)) | (a >> (2u * abits - 8u))) & 0xFFu;
            }
            return px | (a << 24);
        };
        first01 = endpoint(0u) | (static_cast<uint64_t>(endpoint(2u)) << 32);
        second01 = endpoint(1u) | (static_cast<uint64_t>(endpoint(3u)) << 32);
        ep4 = endpoint(4u); ep5 = endpoint(5u);
        if (ns == 2u) { subsets = 0u; const uint32_t m = bc7_partition2(part); for (uint32_t t = 0; t < 16u; ++t) subsets |= ((m >> t) & 1u) << (2u * t); anchor1 = bc7_anchor(0u, part); }
        else if (ns == 3u) { subsets = bc7_partition3(part); anchor1 = bc7_anchor(1u, part); anchor2 = bc7_anchor(2u, part); }
    }

    GFX_BC_FN static uint32_t lerp(uint32_t e0, uint32_t e1, uint32_t w) { return ((64u - w) * e0 + w * e1 + 32u) >> 6; }

    GFX_BC_FN uint32_t texel(uint32_t t) const {
        if (numSubsets == 0u) return 0u;
        const uint32_t s = (subsets >> (2u * t)) & 3u;
        const uint32_t e0 = s == 2u ? ep4 : static_cast<uint32_t>(first01 >> (32u * (s & 1u)));
        const uint32_t e1 = s == 2u ? ep5 : static_cast<uint32_t>(second01 >> (32u * (s & 1u)));
        const uint32_t before = (t > 0u ? 1u : 0u) + (t > anchor1 ? 1u : 0u) + (t > anchor2 ? 1u : 0u);
        const uint32_t isAnchor = (t == 0u || t == anchor1 || t == anchor2) ? 1u : 0u;
        const uint32_t i1 = bits128(lo, hi, indexStart + t * indexBits - before, indexBits - isAnchor);
        uint32_t w1 = bc7_weight(indexBits, i1), w2 = w1;
        if (indexBits2) {
            const uint32_t i2 = bits128(lo, hi, indexStart2 + t * indexBits2 - (t > 0u ? 1u : 0u), indexBits2 - (t == 0u ? 1u : 0u));
            w2 = bc7_weight(indexBits2, i2);
        }
        const uint32_t cw = indexSelection ? w2 : w1, aw = indexSelection ? w1 : w2;
        uint32_t r = lerp(e0 & 0xFFu, e1 & 0xFFu, cw), g = lerp((e0 >> 8) & 0xFFu, (e1 >> 8) & 0xFFu, cw);
        uint32_t b = lerp((e0 >> 16) & 0xFFu, (e1 >> 16) & 0xFFu, cw), a = lerp(e0 >> 24, e1 >> 24, aw);
        if (rotation == 1u) { const uint32_t x = r; r = a; a = x; }
        else if (rotation == 2u) { const uint32_t x = g; g = a; a = x; }
        else if (rotation == 3u) { const uint32_t x = b; b = a; a = x; }
        return pack_rgba(r, g, b, a);
    }
};

// ---------------------------------------------------------------- one decoder per format: Decoder<F>(lo, hi).texel(t) -> RGBA8
// (lo, hi) = the block as two little-endian 64-bit words; the 8-byte formats ignore hi.
template <uint32_t F> struct Decoder;

template <> struct Decoder<kBC1> {
    ColorBlock c;
    GFX_BC_FN Decoder(uint64_t lo, uint64_t) : c(lo, false) {}
    GFX_BC_FN uint32_t texel(uint32_t t) const { return c.texel(t); }
};
template <> struct Decoder<kBC2> {
    ColorBlock c; uint64_t alpha;
    GFX_BC_FN Decoder(uint64_t lo, uint64_t hi) : c(hi, true), alpha(lo) {}
    GFX_BC_FN uint32_t texel(uint32_t t) const { return (c.texel(t) & 0x00FFFFFFu) | (((static_cast<uint32_t>(alpha >> (4u * t)) & 15u) * 17u) << 24); }
};
template <> struct Decoder<kBC3> {
    ColorBlock c; AlphaBlock a;
    GFX_BC_FN Decoder(uint64_t lo, uint64_t hi) : c(hi, true), a(lo, false) {}
    GFX_BC_FN uint32_t texel(uint32_t t) const { return (c.texel(t) & 0x00FFFFFFu) | (a.texel(t) << 24); }
};
template <bool Signed> struct Bc4Decoder {
    AlphaBlock a;
    GFX_BC_FN Bc4Decoder(uint64_t lo, uint64_t) : a(lo, Signed) {}
    GFX_BC_FN uint32_t texel(uint32_t t) const { const uint32_t v = a.texel(t); return pack_rgba(v, v, v, 255u); }
};
template <bool Signed> struct Bc5Decoder {
    AlphaBlock x, y;
    GFX_BC_FN Bc5Decoder(uint64_t lo, uint64_t hi) : x(lo, Signed), y(hi, Signed) {}
    GFX_BC_FN uint32_t texel(uint32_t t) const { return pack_rgba(x.texel(t), y.texel(t), 0u, 255u); }
};
template <> struct Decoder<kBC4U> : Bc4Decoder<false> { using Bc4Decoder<false>::Bc4Decoder; };
template <> struct Decoder<kBC4S> : Bc4Decoder<true> { using Bc4Decoder<true>::Bc4Decoder; };
template <> struct Decoder<kBC5U> : Bc5Decoder<false> { using Bc5Decoder<false>::Bc5Decoder; };
template <> struct Decoder<kBC5S> : Bc5Decoder<true> { using Bc5Decoder<true>::Bc5Decoder; };
template <> struct Decoder<kBC7> {
    Bc7Block b;
    GFX_BC_FN Decoder(uint64_t lo, uint64_t hi) : b(lo, hi) {}
    GFX_BC_FN uint32_t texel(uint32_t t) const { return b.texel(t); }
};

// Texel (x, y) of a width x height image of row-major, tightly packed blocks (level 0 of a DDS as it lies in the file).
template <uint32_t F>
GFX_BC_FN uint32_t image_texel(const uint8_t* blocks, uint32_t width, uint32_t x, uint32_t y) {
    const uint32_t n = block_bytes(F);
    const uint8_t* p = blocks + (static_cast<uint64_t>(y >> 2) * ((width + 3u) >> 2) + (x >> 2)) * n;
    uint64_t w[2] = { 0ull, 0ull };
    for (uint32_t k = 0; k < n; ++k) w[k >> 3] |= static_cast<uint64_t>(p[k]) << (8u * (k & 7u));
    return Decoder<F>(w[0], w[1]).texel((y & 3u) * 4u + (x & 3u));
}

} // namespace bc
} // namespace gfx
