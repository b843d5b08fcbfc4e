// image_codecs.cpp -- PNG / JPEG readers and the PNG writer (image_codecs.h).
//
// Written from the PNG specification (ISO/IEC 15948), RFC 1950 / 1951 and ITU-T T.81, and from reading the reference's decoder
// (ext/stb_image.h v2.25, cited below as stb:LINE) for every place where a decoder has a choice, because the contract is that
// decoder's output byte for byte: the renderers are bit-exact against the oracle from the texels on, so the texels have to be the
// reference's.  The choices are listed where they are made.  Headers are untrusted: dimensions are bounded by kMaxDim before any
// size arithmetic, every read is bounds-checked (the byte reader returns 0 past the end, as the reference's does), and arithmetic
// that a crafted stream could overflow is done modulo 2^32.  On a malformed file only safety is promised, not the reference's verdict.
#include "image_codecs.h"
#include <cstring>
#include <new>

namespace gfx_img {

// ---- inflate (RFC 1950 / 1951): shared by the PNG reader and the ZIP / ZIPS chunks of the OpenEXR reader in image_formats.cpp ----
namespace {
struct BitReader {
    const uint8_t* p; size_t n, at = 0; uint32_t acc = 0; int have = 0; bool bad = false;
    uint32_t bits(int k) {
        while (have < k) { if (at >= n) { bad = true; return 0; } acc |= static_cast<uint32_t>(p[at++]) << have; have += 8; }
        const uint32_t v = acc & ((k == 32) ? 0xFFFFFFFFu : ((1u << k) - 1u));
        acc = k >= 32 ? 0 : acc >> k; have -= k;
        return v;
    }
};
constexpr int kInflateFastBits = 10;
// fast[next kInflateFastBits bits of the stream] = symbol << 4 | code length for codes of at most that length, 0 otherwise
struct Huffman { uint16_t count[16]; uint16_t symbol[288]; uint16_t fast[1 << kInflateFastBits]; };
void build_huffman(Huffman& h, const uint8_t* lengths, int n) {
    std::memset(h.count, 0, sizeof(h.count));
    for (int i = 0; i < n; ++i) ++h.count[lengths[i]];
    h.count[0] = 0;
    uint16_t offs[16]; offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = static_cast<uint16_t>(offs[l] + h.count[l]);
    for (int i = 0; i < n; ++i) if (lengths[i]) h.symbol[offs[lengths[i]]++] = static_cast<uint16_t>(i);
    std::memset(h.fast, 0, sizeof(h.fast));
    uint32_t next[16], code = 0;
    for (int l = 1; l <= 15; ++l) { next[l] = code; code = (code + h.count[l]) << 1; }
    for (int i = 0; i < n; ++i) {
        const int l = lengths[i];
        if (!l) continue;
        const uint32_t c = next[l]++;
        if (l > kInflateFastBits || c >= (1u << l)) continue;              // (an over-subscribed code: left to the bit-wise walk)
        uint32_t rev = 0;                                                  // codes are packed starting from their most significant bit
        for (int b = 0; b < l; ++b) rev |= ((c >> b) & 1u) << (l - 1 - b);
        for (uint32_t k = rev; k < (1u << kInflateFastBits); k += 1u << l) h.fast[k] = static_cast<uint16_t>((i << 4) | l);
    }
}
int decode_symbol(BitReader& br, const Huffman& h) {       // table look-up for short codes; otherwise the canonical code, one bit at a time (RFC 1951 3.2.2)
    while (br.have <= 24 && br.at < br.n) { br.acc |= static_cast<uint32_t>(br.p[br.at++]) << br.have; br.have += 8; }
    const uint32_t e = h.fast[br.acc & ((1u << kInflateFastBits) - 1u)];
    if (e && static_cast<int>(e & 15u) <= br.have) { br.acc >>= (e & 15u); br.have -= static_cast<int>(e & 15u); return static_cast<int>(e >> 4); }
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= 15; ++len) {
        code |= static_cast<int>(br.bits(1));
        if (br.bad) return -1;
        const int count = h.count[len];
        if (code - count < first) return h.symbol[index + (code - first)];
        index += count; first += count; first <<= 1; code <<= 1;
    }
    return -1;
}
} // namespace
// zlib stream -> exactly `want` bytes; false on any malformed input
bool inflate_zlib(const uint8_t* src, size_t n, std::vector<uint8_t>& out, size_t want) {
    static const uint16_t lenBase[29] = { 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258 };
    static const uint16_t lenExtra[29] = { 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0 };
    static const uint16_t distBase[30] = { 1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577 };
    static const uint16_t distExtra[30] = { 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13 };
    if (n < 2 || (src[0] & 0x0F) != 8 || ((src[0] << 8) | src[1]) % 31 != 0 || (src[1] & 0x20)) return false;
    BitReader br{ src + 2, n - 2 };
    out.clear(); out.reserve(want);
    for (bool last = false; !last;) {
        last = br.bits(1) != 0;
        const uint32_t type = br.bits(2);
        if (br.bad) return false;
        if (type == 0) {
            br.at -= static_cast<size_t>(br.have >> 3);               // to the next byte boundary: whole bytes read ahead go back
            br.acc = 0; br.have = 0;
            if (br.at + 4 > br.n) return false;
            const uint32_t len = br.p[br.at] | (br.p[br.at + 1] << 8), nlen = br.p[br.at + 2] | (br.p[br.at + 3] << 8);
            br.at += 4;
            if ((len ^ 0xFFFFu) != nlen || br.at + len > br.n || out.size() + len > want) return false;
            out.insert(out.end(), br.p + br.at, br.p + br.at + len);
            br.at += len;
            continue;
        }
        if (type == 3) return false;
        Huffman lit, dist;
        uint8_t lengths[320];
        if (type == 1) {
            for (int i = 0; i < 144; ++i) lengths[i] = 8;
            for (int i = 144; i < 256; ++i) lengths[i] = 9;
            for (int i = 256; i < 280; ++i) lengths[i] = 7;
            for (int i = 280; i < 288; ++i) lengths[i] = 8;
            build_huffman(lit, lengths, 288);
            for (int i = 0; i < 30; ++i) lengths[i] = 5;
            build_huffman(dist, lengths, 30);
        }
        else {
            static const uint8_t order[19] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };
            const int nlen = static_cast<int>(br.bits(5)) + 257, ndist = static_cast<int>(br.bits(5)) + 1, ncode = static_cast<int>(br.bits(4)) + 4;
            if (br.bad || nlen > 286 || ndist > 30) return false;
            uint8_t cl[19] = { 0 };
            for (int i = 0; i < ncode; ++i) cl[order[i]] = static_cast<uint8_t>(br.bits(3));
            Huffman lc;
            build_huffman(lc, cl, 19);
            int i = 0;
            while (i < nlen + ndist) {
                const int sym = decode_symbol(br, lc);
                if (sym < 0) return false;
                if (sym < 16) { lengths[i++] = static_cast<uint8_t>(sym); continue; }
                int rep, val = 0;
                if (sym == 16) { if (i == 0) return false; val = lengths[i - 1]; rep = 3 + static_cast<int>(br.bits(2)); }
                else if (sym == 17) rep = 3 + static_cast<int>(br.bits(3));
                else rep = 11 + static_cast<int>(br.bits(7));
                if (br.bad || i + rep > nlen + ndist) return false;
                while (rep--) lengths[i++] = static_cast<uint8_t>(val);
            }
            if (lengths[256] == 0) return false;
            build_huffman(lit, lengths, nlen);
            build_huffman(dist, lengths + nlen, ndist);
        }
        for (;;) {
            const int sym = decode_symbol(br, lit);
            if (sym < 0) return false;
            if (sym < 256) { if (out.size() >= want) return false; out.push_back(static_cast<uint8_t>(sym)); continue; }
            if (sym == 256) break;
            if (sym > 285) return false;
            const uint32_t len = lenBase[sym - 257] + br.bits(lenExtra[sym - 257]);
            const int ds = decode_symbol(br, dist);
            if (ds < 0 || ds > 29) return false;
            const uint32_t d = distBase[ds] + br.bits(distExtra[ds]);
            if (br.bad || d > out.size() || out.size() + len > want) return false;
            for (uint32_t k = 0; k < len; ++k) out.push_back(out[out.size() - d]);
        }
    }
    return out.size() == want;
}

namespace {

// ---- big-endian byte reader; past the end it yields zeros (stb:1499-1640 does the same, which several loops below rely on) ----
struct Reader {
    const uint8_t* p; size_t n, at = 0;
    Reader(const uint8_t* d, size_t bytes) : p(d), n(bytes) {}
    bool eof() const { return at >= n; }
    uint32_t get8() { return at < n ? p[at++] : 0u; }
    uint32_t get16() { const uint32_t a = get8(); return (a << 8) | get8(); }
    uint32_t get32() { const uint32_t a = get16(); return (a << 16) | get16(); }
    void skip(int64_t k) { if (k < 0 || static_cast<uint64_t>(k) > n - at) at = n; else at += static_cast<size_t>(k); }
};

bool too_large(uint32_t w, uint32_t h) { return w > kMaxDim || h > kMaxDim; }
const char* kTooLarge = "image larger than 16384 x 16384";

// =====================================================================================================================
// PNG
// =====================================================================================================================
constexpr uint32_t chunk_type(char a, char b, char c, char d) {
    return (static_cast<uint32_t>(static_cast<uint8_t>(a)) << 24) | (static_cast<uint32_t>(static_cast<uint8_t>(b)) << 16) |
           (static_cast<uint32_t>(static_cast<uint8_t>(c)) << 8) | static_cast<uint32_t>(static_cast<uint8_t>(d));
}
const uint8_t kPngSignature[8] = { 0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A };

struct PngHeader {
    uint32_t w = 0, h = 0, depth = 0, colour = 0, interlace = 0;
    uint32_t samples = 0;                 // samples per pixel in the file (1 for a palette index)
    bool paletted = false, palTrans = false, keyTrans = false;
    uint32_t palLen = 0;
    uint8_t palette[256 * 4];
    uint16_t key[3] = { 0, 0, 0 };        // tRNS colour key: at 16 bit as stored, below that already scaled like the samples
    std::vector<uint8_t> idat;
    uint32_t channels() const { return paletted ? (palTrans ? 4u : 3u) : samples + (keyTrans ? 1u : 0u); }
};

// grey of depth < 8 is scaled to 0..255 by replication (stb:4475, 4611); palette indices are not
uint32_t depth_scale(uint32_t depth) { return depth == 1 ? 0xFFu : depth == 2 ? 0x55u : depth == 4 ? 0x11u : 1u; }

// Chunk walk (stb:4879-5051).  headerOnly stops at the first IDAT (a tRNS chunk before it changes the channel count).
bool png_parse(const uint8_t* data, size_t bytes, bool headerOnly, PngHeader& hd, std::string& err) {
    auto fail = [&](const char* what) { err = std::string("PNG: ") + what; return false; };
    if (bytes < 8 || std::memcmp(data, kPngSignature, 8) != 0) return fail("bad signature");
    Reader r(data, bytes);
    r.at = 8;
    bool first = true, haveIdat = false;
    std::memset(hd.palette, 0, sizeof(hd.palette));
    for (;;) {
        if (bytes - r.at < 8) return fail("the file ends before IEND");
        const uint32_t length = r.get32(), type = r.get32();
        if (length > bytes - r.at) return fail("chunk longer than the file");
        const size_t body = r.at;
        if (first && type != chunk_type('I', 'H', 'D', 'R')) return fail(type == chunk_type('C', 'g', 'B', 'I') ? "Apple CgBI files are not read" : "first chunk is not IHDR");
        switch (type) {
        case chunk_type('C', 'g', 'B', 'I'): return fail("Apple CgBI files are not read");
        case chunk_type('I', 'H', 'D', 'R'): {
            if (!first) return fail("several IHDR chunks");
            first = false;
            if (length != 13) return fail("bad IHDR length");
            hd.w = r.get32(); hd.h = r.get32();
            if (too_large(hd.w, hd.h)) return fail(kTooLarge);
            hd.depth = r.get8(); hd.colour = r.get8();
            const uint32_t comp = r.get8(), filter = r.get8();
            hd.interlace = r.get8();
            if (hd.depth != 1 && hd.depth != 2 && hd.depth != 4 && hd.depth != 8 && hd.depth != 16) return fail("bit depth is not 1 / 2 / 4 / 8 / 16");
            if (hd.colour != 0 && hd.colour != 2 && hd.colour != 3 && hd.colour != 4 && hd.colour != 6) return fail("bad colour type");
            if ((hd.colour == 3 && hd.depth == 16) || (hd.colour != 0 && hd.colour != 3 && hd.depth < 8)) return fail("bit depth not allowed for the colour type");
            if (comp || filter || hd.interlace > 1) return fail("bad compression / filter / interlace method");
            if (!hd.w || !hd.h) return fail("0-pixel image");
            hd.paletted = hd.colour == 3;
            hd.samples = hd.paletted ? 1u : ((hd.colour & 2) ? 3u : 1u) + ((hd.colour & 4) ? 1u : 0u);
            break;
        }
        case chunk_type('P', 'L', 'T', 'E'): {
            if (length > 256 * 3 || length % 3) return fail("invalid PLTE");
            hd.palLen = length / 3;
            for (uint32_t i = 0; i < hd.palLen; ++i) {
                hd.palette[4 * i] = static_cast<uint8_t>(r.get8()); hd.palette[4 * i + 1] = static_cast<uint8_t>(r.get8());
                hd.palette[4 * i + 2] = static_cast<uint8_t>(r.get8()); hd.palette[4 * i + 3] = 255;
            }
            break;
        }
        case chunk_type('t', 'R', 'N', 'S'): {
            if (haveIdat) return fail("tRNS after IDAT");
            if (hd.paletted) {
                if (!hd.palLen) return fail("tRNS before PLTE");
                if (length > hd.palLen) return fail("bad tRNS length");
                hd.palTrans = true;
                for (uint32_t i = 0; i < length; ++i) hd.palette[4 * i + 3] = static_cast<uint8_t>(r.get8());
            }
            else {
                if (!(hd.samples & 1)) return fail("tRNS with alpha");
                if (length != hd.samples * 2) return fail("bad tRNS length");
                hd.keyTrans = true;
                // 16 bit: the key as stored; otherwise its low byte times the grey scale, kept in 8 bits (stb:4961-4963)
                for (uint32_t k = 0; k < hd.samples; ++k) {
                    const uint32_t v = r.get16();
                    hd.key[k] = hd.depth == 16 ? static_cast<uint16_t>(v) : static_cast<uint16_t>(((v & 255u) * depth_scale(hd.depth)) & 255u);
                }
            }
            break;
        }
        case chunk_type('I', 'D', 'A', 'T'): {
            if (hd.paletted && !hd.palLen) return fail("no PLTE");
            if (headerOnly) return true;
            haveIdat = true;
            hd.idat.insert(hd.idat.end(), data + body, data + body + length);
            break;
        }
        case chunk_type('I', 'E', 'N', 'D'): {
            if (!haveIdat && !headerOnly) return fail("no IDAT");
            return true;
        }
        default:
            if (!(type & (1u << 29))) return fail("unknown critical chunk");      // ancillary chunks (gAMA, sRGB, iCCP, tEXt, ...) are skipped
            break;
        }
        r.at = body + length;                     // what is left of the chunk, then its CRC (not checked, as in the reference)
        r.skip(4);
    }
}

int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    if (pa <= pb && pa <= pc) return a;
    return pb <= pc ? b : c;
}

// Undo the scanline filters of one (sub-)image in place: `rows` lines of 1 + rowBytes bytes.  bpp = bytes per complete pixel, at least 1.
bool png_unfilter(uint8_t* raw, uint32_t rows, size_t rowBytes, uint32_t bpp) {
    const uint8_t* prior = nullptr;
    for (uint32_t j = 0; j < rows; ++j) {
        const uint32_t filter = raw[0];
        uint8_t* cur = raw + 1;
        if (filter > 4) return false;
        for (size_t k = 0; k < rowBytes; ++k) {
            const int a = k >= bpp ? cur[k - bpp] : 0, b = prior ? prior[k] : 0, c = (prior && k >= bpp) ? prior[k - bpp] : 0;
            int pred = 0;
            if (filter == 1) pred = a; else if (filter == 2) pred = b; else if (filter == 3) pred = (a + b) >> 1; else if (filter == 4) pred = paeth(a, b, c);
            cur[k] = static_cast<uint8_t>(cur[k] + pred);
        }
        prior = cur;
        raw += rowBytes + 1;
    }
    return true;
}

// One unfiltered line of `n` pixels -> RGBA8 at out + 4 * (x0 + i * dx).  This is where the reference's choices sit:
//   16-bit samples: the colour key is compared at 16 bit, then every sample is reduced by >> 8 (stb:4759, 1096)
//   grey -> (g, g, g, 255), grey-alpha -> (g, g, g, a) (stb:1654); grey below 8 bit scaled by depth_scale; no gamma handling
bool png_emit_line(const PngHeader& hd, const uint8_t* line, uint32_t n, uint8_t* out, uint32_t x0, uint32_t dx) {
    const uint32_t scale = depth_scale(hd.depth);
    for (uint32_t i = 0; i < n; ++i) {
        uint8_t* o = out + 4ull * (x0 + static_cast<size_t>(i) * dx);
        if (hd.depth < 8) {
            const uint32_t bit = i * hd.depth;
            const uint32_t v = (line[bit >> 3] >> (8 - hd.depth - (bit & 7))) & ((1u << hd.depth) - 1u);
            if (hd.paletted) {
                if (v >= hd.palLen) return false;
                std::memcpy(o, hd.palette + 4 * v, 4);
            }
            else {
                const uint8_t g = static_cast<uint8_t>(v * scale);
                o[0] = o[1] = o[2] = g; o[3] = (hd.keyTrans && g == hd.key[0]) ? 0 : 255;
            }
        }
        else if (hd.depth == 8) {
            const uint8_t* s = line + static_cast<size_t>(i) * hd.samples;
            if (hd.paletted) {
                if (s[0] >= hd.palLen) return false;
                std::memcpy(o, hd.palette + 4 * s[0], 4);
            }
            else if (hd.samples == 1) { o[0] = o[1] = o[2] = s[0]; o[3] = (hd.keyTrans && s[0] == hd.key[0]) ? 0 : 255; }
            else if (hd.samples == 2) { o[0] = o[1] = o[2] = s[0]; o[3] = s[1]; }
            else {
                o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
                o[3] = hd.samples == 4 ? s[3] : ((hd.keyTrans && s[0] == hd.key[0] && s[1] == hd.key[1] && s[2] == hd.key[2]) ? 0 : 255);
            }
        }
        else {
            const uint8_t* s = line + static_cast<size_t>(i) * hd.samples * 2;
            auto s16 = [&](uint32_t k) { return static_cast<uint16_t>((s[2 * k] << 8) | s[2 * k + 1]); };
            if (hd.samples == 1) { o[0] = o[1] = o[2] = s[0]; o[3] = (hd.keyTrans && s16(0) == hd.key[0]) ? 0 : 255; }
            else if (hd.samples == 2) { o[0] = o[1] = o[2] = s[0]; o[3] = s[2]; }
            else {
                o[0] = s[0]; o[1] = s[2]; o[2] = s[4];
                o[3] = hd.samples == 4 ? s[6] : ((hd.keyTrans && s16(0) == hd.key[0] && s16(1) == hd.key[1] && s16(2) == hd.key[2]) ? 0 : 255);
            }
        }
    }
    return true;
}

bool png_decode_impl(const uint8_t* data, size_t bytes, Info& info, std::vector<uint8_t>& rgba, std::string& err) {
    PngHeader hd;
    if (!png_parse(data, bytes, false, hd, err)) return false;
    auto fail = [&](const char* what) { err = std::string("PNG: ") + what; return false; };
    info.width = hd.w; info.height = hd.h; info.channels = hd.channels(); info.kind = kKindPng;
    // Adam7: pass p holds the pixels (xo + i * xs, yo + j * ys); a non-interlaced file is the single pass (0, 0, 1, 1)
    static const uint32_t xo[7] = { 0, 4, 0, 2, 0, 1, 0 }, yo[7] = { 0, 0, 4, 0, 2, 0, 1 }, xs[7] = { 8, 8, 4, 4, 2, 2, 1 }, ys[7] = { 8, 8, 8, 4, 4, 2, 2 };
    const uint32_t passes = hd.interlace ? 7u : 1u;
    const uint32_t bitsPerPixel = hd.samples * hd.depth;
    uint32_t pw[7], ph[7]; size_t rowBytes[7], total = 0;
    for (uint32_t p = 0; p < passes; ++p) {
        pw[p] = hd.interlace ? (hd.w - xo[p] + xs[p] - 1) / xs[p] : hd.w;
        ph[p] = hd.interlace ? (hd.h - yo[p] + ys[p] - 1) / ys[p] : hd.h;
        if (hd.interlace && (hd.w <= xo[p] || hd.h <= yo[p])) pw[p] = ph[p] = 0;
        rowBytes[p] = (static_cast<size_t>(pw[p]) * bitsPerPixel + 7) >> 3;
        if (pw[p] && ph[p]) total += (rowBytes[p] + 1) * ph[p];
    }
    // deflate shrinks by at most ~1032 : 1, so a tiny file cannot honestly hold a huge image: refuse before allocating for it
    if (total / 1100u > hd.idat.size()) return fail("image far larger than its file can hold");
    std::vector<uint8_t> raw;
    if (!inflate_zlib(hd.idat.data(), hd.idat.size(), raw, total)) return fail("malformed or short IDAT stream");
    rgba.assign(4ull * hd.w * hd.h, 0);
    const uint32_t bpp = bitsPerPixel >= 8 ? bitsPerPixel / 8 : 1u;
    size_t at = 0;
    for (uint32_t p = 0; p < passes; ++p) {
        if (!pw[p] || !ph[p]) continue;
        if (!png_unfilter(raw.data() + at, ph[p], rowBytes[p], bpp)) return fail("invalid filter");
        for (uint32_t j = 0; j < ph[p]; ++j) {
            const uint32_t y = hd.interlace ? yo[p] + j * ys[p] : j;
            if (!png_emit_line(hd, raw.data() + at + (rowBytes[p] + 1) * j + 1, pw[p], rgba.data() + 4ull * hd.w * y, hd.interlace ? xo[p] : 0u, hd.interlace ? xs[p] : 1u))
                return fail("palette index outside PLTE");
        }
        at += (rowBytes[p] + 1) * ph[p];
    }
    return true;
}

// =====================================================================================================================
// JPEG (Huffman-coded, 8 bit: SOF0 / SOF1 sequential and SOF2 progressive)
// =====================================================================================================================
constexpr int kFastBits = 9;                     // prefix length of the direct-lookup table
const uint8_t kMarkerNone = 0xFF;

struct HuffTable {
    bool defined = false;
    uint8_t fast[1 << kFastBits];                // symbol index for codes of <= kFastBits bits, 255 = longer
    uint16_t code[256];
    uint8_t values[256];
    uint8_t size[257];
    uint32_t maxcode[18];                        // largest code of each length + 1, left-aligned in 16 bits
    int delta[17];                               // first symbol index - first code of each length
};

struct Component {
    uint32_t id = 0, h = 0, v = 0, tq = 0, hd = 0, ha = 0;
    uint32_t dcPred = 0;                         // modulo 2^32: a crafted stream can push the running sum past int
    uint32_t x = 0, y = 0, w2 = 0, h2 = 0;       // size in samples; w2 x h2 = size padded to whole interleaved MCUs
    std::vector<uint8_t> data;
    std::vector<int16_t> coeff;                  // progressive only: 64 coefficients per block, coeffW blocks per row
    uint32_t coeffW = 0;
    std::vector<uint8_t> linebuf;
};

struct Jpeg {
    Reader s;
    HuffTable huffDc[4], huffAc[4];
    uint16_t dequant[4][64];
    uint32_t imgX = 0, imgY = 0, imgN = 0;
    uint32_t hMax = 1, vMax = 1, mcuX = 0, mcuY = 0;
    Component comp[4];
    uint32_t codeBuffer = 0; int codeBits = 0; uint8_t marker = kMarkerNone; bool noMore = false;
    bool progressive = false;
    int specStart = 0, specEnd = 0, succHigh = 0, succLow = 0, eobRun = 0;
    bool jfif = false; int app14Transform = -1; uint32_t rgbIds = 0;
    int scanN = 0, order[4] = { 0, 0, 0, 0 };
    uint32_t restartInterval = 0; int64_t todo = 0;
    std::string err;
    Jpeg(const uint8_t* d, size_t n) : s(d, n) { std::memset(dequant, 0, sizeof(dequant)); }
    bool fail(const char* what) { err = std::string("JPEG: ") + what; return false; }
};

// zig-zag position -> row-major position; runs of a corrupt stream may step past 63 and land on the last coefficient
const uint8_t kDezigzag[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63 };
inline uint32_t dezigzag(int k) { return kDezigzag[k < 64 ? k : 63]; }

bool build_huffman(HuffTable& h, const int* count) {
    int k = 0;
    for (int i = 0; i < 16; ++i)
        for (int j = 0; j < count[i]; ++j) { if (k >= 256) return false; h.size[k++] = static_cast<uint8_t>(i + 1); }
    h.size[k] = 0;
    const int total = k;
    uint32_t code = 0;
    k = 0;
    for (int j = 1; j <= 16; ++j) {
        h.delta[j] = k - static_cast<int>(code);
        if (h.size[k] == j) {
            while (h.size[k] == j) h.code[k++] = static_cast<uint16_t>(code++);
            if (code - 1 >= (1u << j)) return false;                 // more codes of this length than fit
        }
        h.maxcode[j] = code << (16 - j);
        code <<= 1;
    }
    h.maxcode[17] = 0xFFFFFFFFu;
    std::memset(h.fast, 255, sizeof(h.fast));
    for (int i = 0; i < total; ++i) {
        const int s = h.size[i];
        if (s <= kFastBits) {
            const int c = h.code[i] << (kFastBits - s), m = 1 << (kFastBits - s);
            for (int j = 0; j < m; ++j) h.fast[c + j] = static_cast<uint8_t>(i);
        }
    }
    h.defined = true;
    return true;
}

// Refill the bit buffer up to 25..32 bits.  FF 00 is a stuffed FF; FF followed by anything else is a marker: it is remembered
// and the stream reads as zeros from there on (stb:1971-1987), which is what the end of every scan and restart interval sees.
void grow_buffer(Jpeg& j) {
    do {
        const uint32_t b = j.noMore ? 0u : j.s.get8();
        if (b == 0xFF) {
            uint32_t c = j.s.get8();
            while (c == 0xFF) c = j.s.get8();
            if (c != 0) { j.marker = static_cast<uint8_t>(c); j.noMore = true; return; }
        }
        j.codeBuffer |= b << (24 - j.codeBits);
        j.codeBits += 8;
    } while (j.codeBits <= 24);
}
inline uint32_t low_mask(int n) { return (1u << n) - 1u; }

int huff_decode(Jpeg& j, const HuffTable& h) {
    if (j.codeBits < 16) grow_buffer(j);
    const uint32_t c = (j.codeBuffer >> (32 - kFastBits)) & low_mask(kFastBits);
    int k = h.fast[c];
    if (k < 255) {
        const int s = h.size[k];
        if (s > j.codeBits) return -1;
        j.codeBuffer <<= s; j.codeBits -= s;
        return h.values[k];
    }
    const uint32_t temp = j.codeBuffer >> 16;
    for (k = kFastBits + 1; ; ++k) if (temp < h.maxcode[k]) break;
    if (k == 17) { j.codeBits -= 16; return -1; }
    if (k > j.codeBits) return -1;
    const int sym = static_cast<int>((j.codeBuffer >> (32 - k)) & low_mask(k)) + h.delta[k];
    if (sym < 0 || sym > 255) return -1;
    j.codeBits -= k; j.codeBuffer <<= k;
    return h.values[sym];
}
inline uint32_t rotl(uint32_t x, int n) { return n ? (x << n) | (x >> (32 - n)) : x; }
// n bits, sign-extended the JPEG way (T.81 F.2.2.1 RECEIVE + EXTEND); n in 1..15
int extend_receive(Jpeg& j, int n) {
    if (j.codeBits < n) grow_buffer(j);
    const bool negative = !(j.codeBuffer & 0x80000000u);
    uint32_t k = rotl(j.codeBuffer, n);
    j.codeBuffer = k & ~low_mask(n);
    k &= low_mask(n);
    j.codeBits -= n;
    return static_cast<int>(k) + (negative ? 1 - (1 << n) : 0);
}
int get_bits(Jpeg& j, int n) {
    if (j.codeBits < n) grow_buffer(j);
    uint32_t k = rotl(j.codeBuffer, n);
    j.codeBuffer = k & ~low_mask(n);
    k &= low_mask(n);
    j.codeBits -= n;
    return static_cast<int>(k);
}
bool get_bit(Jpeg& j) {
    if (j.codeBits < 1) grow_buffer(j);
    const uint32_t k = j.codeBuffer;
    j.codeBuffer <<= 1; --j.codeBits;
    return (k & 0x80000000u) != 0;
}
inline int16_t wrap16(uint32_t v) { return static_cast<int16_t>(static_cast<uint16_t>(v)); }

// One block of a sequential scan, de-quantised as it is decoded (stb:2102)
bool decode_block(Jpeg& j, int16_t* data, const HuffTable& hdc, const HuffTable& hac, Component& c, const uint16_t* dq) {
    const int t = huff_decode(j, hdc);
    if (t < 0 || t > 15) return j.fail("bad huffman code");
    std::memset(data, 0, 64 * sizeof(int16_t));
    const uint32_t diff = t ? static_cast<uint32_t>(extend_receive(j, t)) : 0u;
    c.dcPred += diff;
    data[0] = wrap16(c.dcPred * dq[0]);
    int k = 1;
    do {
        const int rs = huff_decode(j, hac);
        if (rs < 0) return j.fail("bad huffman code");
        const int s = rs & 15, r = rs >> 4;
        if (s == 0) {
            if (rs != 0xF0) break;
            k += 16;
        }
        else {
            k += r;
            const uint32_t zig = dezigzag(k++);
            data[zig] = wrap16(static_cast<uint32_t>(extend_receive(j, s)) * dq[zig]);
        }
    } while (k < 64);
    return true;
}
// Progressive: DC first scan / refinement (stb:2154), AC first scan / refinement (stb:2181); coefficients stay quantised until finish
bool decode_block_prog_dc(Jpeg& j, int16_t* data, const HuffTable& hdc, Component& c) {
    if (j.specEnd != 0) return j.fail("can't merge dc and ac");
    if (j.succHigh == 0) {
        std::memset(data, 0, 64 * sizeof(int16_t));
        const int t = huff_decode(j, hdc);
        if (t < 0 || t > 15) return j.fail("bad huffman code");
        const uint32_t diff = t ? static_cast<uint32_t>(extend_receive(j, t)) : 0u;
        c.dcPred += diff;
        data[0] = wrap16(c.dcPred * (1u << j.succLow));
    }
    else if (get_bit(j)) data[0] = wrap16(static_cast<uint32_t>(data[0]) + (1u << j.succLow));
    return true;
}
bool decode_block_prog_ac(Jpeg& j, int16_t* data, const HuffTable& hac) {
    if (j.specStart == 0) return j.fail("can't merge dc and ac");
    auto refine = [&](int16_t& p, int bit) {         // one correction bit for a coefficient that is already non-zero
        if (get_bit(j) && (p & bit) == 0) p = wrap16(static_cast<uint32_t>(p) + static_cast<uint32_t>(p > 0 ? bit : -bit));
    };
    if (j.succHigh == 0) {
        if (j.eobRun) { --j.eobRun; return true; }
        int k = j.specStart;
        do {
            const int rs = huff_decode(j, hac);
            if (rs < 0) return j.fail("bad huffman code");
            const int s = rs & 15, r = rs >> 4;
            if (s == 0) {
                if (r < 15) {
                    j.eobRun = 1 << r;
                    if (r) j.eobRun += get_bits(j, r);
                    --j.eobRun;
                    break;
                }
                k += 16;
            }
            else {
                k += r;
                const uint32_t zig = dezigzag(k++);
                data[zig] = wrap16(static_cast<uint32_t>(extend_receive(j, s)) * (1u << j.succLow));
            }
        } while (k <= j.specEnd);
    }
    else {
        const int bit = 1 << j.succLow;
        if (j.eobRun) {
            --j.eobRun;
            for (int k = j.specStart; k <= j.specEnd; ++k) { int16_t& p = data[dezigzag(k)]; if (p != 0) refine(p, bit); }
        }
        else {
            int k = j.specStart;
            do {
                const int rs = huff_decode(j, hac);
                if (rs < 0) return j.fail("bad huffman code");
                int s = rs & 15, r = rs >> 4;
                if (s == 0) {
                    if (r < 15) {
                        j.eobRun = (1 << r) - 1;
                        if (r) j.eobRun += get_bits(j, r);
                        r = 64;                      // end of block: only corrections follow
                    }
                    // r == 15: sixteen zeros = a run of 15 and a new value of 0
                }
                else {
                    if (s != 1) return j.fail("bad huffman code");
                    s = get_bit(j) ? bit : -bit;
                }
                while (k <= j.specEnd) {
                    int16_t& p = data[dezigzag(k++)];
                    if (p != 0) refine(p, bit);
                    else {
                        if (r == 0) { p = static_cast<int16_t>(s); break; }
                        --r;
                    }
                }
            } while (k <= j.specEnd);
        }
    }
    return true;
}

// ---- inverse DCT: the 12-bit fixed-point "islow" butterfly with the reference's rounding (stb:2311-2409).  Constants are
// (int)(c * 4096 + 0.5) of the float literal; the column pass keeps two extra bits (+512 >> 10) and takes a shortcut for a column
// whose AC terms are all zero (4 * DC, no rounding term -- not the same number as the full path would give); the row pass rounds
// with 65536 + (128 << 17) >> 17 and clamps.  All in uint32_t so that crafted coefficients wrap and do not overflow.
constexpr uint32_t fix12(float x) { return static_cast<uint32_t>(static_cast<int>(x * 4096 + 0.5)); }
struct Idct1D { uint32_t x0, x1, x2, x3, t0, t1, t2, t3; };
inline Idct1D idct_1d(uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3, uint32_t s4, uint32_t s5, uint32_t s6, uint32_t s7) {
    Idct1D o;
    uint32_t p1 = (s2 + s6) * fix12(0.5411961f);
    uint32_t t2 = p1 + s6 * fix12(-1.847759065f);
    uint32_t t3 = p1 + s2 * fix12(0.765366865f);
    uint32_t t0 = (s0 + s4) * 4096u;
    uint32_t t1 = (s0 - s4) * 4096u;
    o.x0 = t0 + t3; o.x3 = t0 - t3; o.x1 = t1 + t2; o.x2 = t1 - t2;
    t0 = s7; t1 = s5; t2 = s3; t3 = s1;
    uint32_t p3 = t0 + t2, p4 = t1 + t3;
    p1 = t0 + t3;
    uint32_t p2 = t1 + t2;
    const uint32_t p5 = (p3 + p4) * fix12(1.175875602f);
    t0 *= fix12(0.298631336f); t1 *= fix12(2.053119869f); t2 *= fix12(3.072711026f); t3 *= fix12(1.501321110f);
    p1 = p5 + p1 * fix12(-0.899976223f);
    p2 = p5 + p2 * fix12(-2.562915447f);
    p3 *= fix12(-1.961570560f);
    p4 *= fix12(-0.390180644f);
    o.t3 = t3 + p1 + p4; o.t2 = t2 + p2 + p3; o.t1 = t1 + p2 + p4; o.t0 = t0 + p1 + p3;
    return o;
}
inline uint32_t sext16(int16_t v) { return static_cast<uint32_t>(static_cast<int32_t>(v)); }
inline uint32_t sar(uint32_t v, int n) { return static_cast<uint32_t>(static_cast<int32_t>(v) >> n); }
inline uint8_t clamp8(uint32_t v) { const int32_t x = static_cast<int32_t>(v); return x < 0 ? 0 : x > 255 ? 255 : static_cast<uint8_t>(x); }
void idct_block(uint8_t* out, size_t stride, const int16_t* d) {
    uint32_t val[64];
    for (int i = 0; i < 8; ++i) {
        uint32_t* v = val + i;
        const int16_t* c = d + i;
        if (c[8] == 0 && c[16] == 0 && c[24] == 0 && c[32] == 0 && c[40] == 0 && c[48] == 0 && c[56] == 0) {
            const uint32_t dc = sext16(c[0]) * 4u;
            v[0] = v[8] = v[16] = v[24] = v[32] = v[40] = v[48] = v[56] = dc;
        }
        else {
            Idct1D o = idct_1d(sext16(c[0]), sext16(c[8]), sext16(c[16]), sext16(c[24]), sext16(c[32]), sext16(c[40]), sext16(c[48]), sext16(c[56]));
            o.x0 += 512; o.x1 += 512; o.x2 += 512; o.x3 += 512;
            v[0] = sar(o.x0 + o.t3, 10); v[56] = sar(o.x0 - o.t3, 10);
            v[8] = sar(o.x1 + o.t2, 10); v[48] = sar(o.x1 - o.t2, 10);
            v[16] = sar(o.x2 + o.t1, 10); v[40] = sar(o.x2 - o.t1, 10);
            v[24] = sar(o.x3 + o.t0, 10); v[32] = sar(o.x3 - o.t0, 10);
        }
    }
    for (int i = 0; i < 8; ++i) {
        const uint32_t* v = val + 8 * i;
        uint8_t* o8 = out + stride * i;
        Idct1D o = idct_1d(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
        const uint32_t bias = 65536u + (128u << 17);
        o.x0 += bias; o.x1 += bias; o.x2 += bias; o.x3 += bias;
        o8[0] = clamp8(sar(o.x0 + o.t3, 17)); o8[7] = clamp8(sar(o.x0 - o.t3, 17));
        o8[1] = clamp8(sar(o.x1 + o.t2, 17)); o8[6] = clamp8(sar(o.x1 - o.t2, 17));
        o8[2] = clamp8(sar(o.x2 + o.t1, 17)); o8[5] = clamp8(sar(o.x2 - o.t1, 17));
        o8[3] = clamp8(sar(o.x3 + o.t0, 17)); o8[4] = clamp8(sar(o.x3 - o.t0, 17));
    }
}

uint8_t get_marker(Jpeg& j) {
    if (j.marker != kMarkerNone) { const uint8_t x = j.marker; j.marker = kMarkerNone; return x; }
    uint32_t x = j.s.get8();
    if (x != 0xFF) return kMarkerNone;
    while (x == 0xFF) x = j.s.get8();
    return static_cast<uint8_t>(x);
}
inline bool is_restart(uint8_t m) { return m >= 0xD0 && m <= 0xD7; }
void reset_entropy(Jpeg& j) {
    j.codeBits = 0; j.codeBuffer = 0; j.noMore = false;
    for (Component& c : j.comp) c.dcPred = 0;
    j.marker = kMarkerNone;
    j.todo = j.restartInterval ? static_cast<int64_t>(j.restartInterval) : 0x7FFFFFFF;
    j.eobRun = 0;
}
// after each MCU: at the end of a restart interval the next marker has to be RSTn; if it is not, the scan ends there
// with what was decoded (stb:2854-2860).  Returns false when the scan is over.
inline bool count_restart(Jpeg& j) {
    if (--j.todo <= 0) {
        if (j.codeBits < 24) grow_buffer(j);
        if (!is_restart(j.marker)) return false;
        reset_entropy(j);
    }
    return true;
}

bool parse_entropy_coded_data(Jpeg& z) {
    reset_entropy(z);
    int16_t block[64];
    if (z.scanN == 1) {
        // one component: its blocks in raster order, as many as its own size needs (not padded to interleaved MCUs)
        Component& c = z.comp[z.order[0]];
        const uint32_t w = (c.x + 7) >> 3, h = (c.y + 7) >> 3;
        for (uint32_t j = 0; j < h; ++j)
            for (uint32_t i = 0; i < w; ++i) {
                if (!z.progressive) {
                    if (!decode_block(z, block, z.huffDc[c.hd], z.huffAc[c.ha], c, z.dequant[c.tq])) return false;
                    idct_block(c.data.data() + static_cast<size_t>(c.w2) * j * 8 + i * 8, c.w2, block);
                }
                else {
                    int16_t* data = c.coeff.data() + 64ull * (i + static_cast<size_t>(j) * c.coeffW);
                    if (z.specStart == 0) { if (!decode_block_prog_dc(z, data, z.huffDc[c.hd], c)) return false; }
                    else if (!decode_block_prog_ac(z, data, z.huffAc[c.ha])) return false;
                }
                if (!count_restart(z)) return true;
            }
        return true;
    }
    for (uint32_t j = 0; j < z.mcuY; ++j)
        for (uint32_t i = 0; i < z.mcuX; ++i) {
            for (int k = 0; k < z.scanN; ++k) {
                Component& c = z.comp[z.order[k]];
                for (uint32_t y = 0; y < c.v; ++y)
                    for (uint32_t x = 0; x < c.h; ++x) {
                        const size_t bx = static_cast<size_t>(i) * c.h + x, by = static_cast<size_t>(j) * c.v + y;
                        if (!z.progressive) {
                            if (!decode_block(z, block, z.huffDc[c.hd], z.huffAc[c.ha], c, z.dequant[c.tq])) return false;
                            idct_block(c.data.data() + c.w2 * by * 8 + bx * 8, c.w2, block);
                        }
                        else if (!decode_block_prog_dc(z, c.coeff.data() + 64ull * (bx + by * c.coeffW), z.huffDc[c.hd], c)) return false;
                    }
            }
            if (!count_restart(z)) return true;
        }
    return true;
}

// progressive: de-quantise at the end, in 16 bits as the reference does (stb:2958-2981), then the inverse DCT
void finish_progressive(Jpeg& z) {
    for (uint32_t n = 0; n < z.imgN; ++n) {
        Component& c = z.comp[n];
        const uint32_t w = (c.x + 7) >> 3, h = (c.y + 7) >> 3;
        for (uint32_t j = 0; j < h; ++j)
            for (uint32_t i = 0; i < w; ++i) {
                int16_t* data = c.coeff.data() + 64ull * (i + static_cast<size_t>(j) * c.coeffW);
                for (int k = 0; k < 64; ++k) data[k] = wrap16(sext16(data[k]) * z.dequant[c.tq][k]);
                idct_block(c.data.data() + static_cast<size_t>(c.w2) * j * 8 + i * 8, c.w2, data);
            }
    }
}

bool process_marker(Jpeg& z, int m) {
    int L;
    switch (m) {
    case kMarkerNone: return z.fail("expected marker");
    case 0xDD:
        if (z.s.get16() != 4) return z.fail("bad DRI len");
        z.restartInterval = z.s.get16();
        return true;
    case 0xDB:
        L = static_cast<int>(z.s.get16()) - 2;
        while (L > 0) {
            const uint32_t q = z.s.get8(), p = q >> 4, t = q & 15;
            if (p > 1) return z.fail("bad DQT type");
            if (t > 3) return z.fail("bad DQT table");
            for (int i = 0; i < 64; ++i) z.dequant[t][kDezigzag[i]] = static_cast<uint16_t>(p ? z.s.get16() : z.s.get8());
            L -= p ? 129 : 65;
        }
        if (L != 0) return z.fail("bad DQT len");
        return true;
    case 0xC4:
        L = static_cast<int>(z.s.get16()) - 2;
        while (L > 0) {
            int sizes[16], n = 0;
            const uint32_t q = z.s.get8(), tc = q >> 4, th = q & 15;
            if (tc > 1 || th > 3) return z.fail("bad DHT header");
            for (int i = 0; i < 16; ++i) { sizes[i] = static_cast<int>(z.s.get8()); n += sizes[i]; }
            if (n > 256) return z.fail("bad code lengths");
            L -= 17;
            HuffTable& h = tc == 0 ? z.huffDc[th] : z.huffAc[th];
            if (!build_huffman(h, sizes)) return z.fail("bad code lengths");
            for (int i = 0; i < n; ++i) h.values[i] = static_cast<uint8_t>(z.s.get8());
            L -= n;
        }
        if (L != 0) return z.fail("bad DHT len");
        return true;
    }
    if ((m >= 0xE0 && m <= 0xEF) || m == 0xFE) {
        L = static_cast<int>(z.s.get16());
        if (L < 2) return z.fail(m == 0xFE ? "bad COM len" : "bad APP len");
        L -= 2;
        if (m == 0xE0 && L >= 5) {                   // JFIF APP0
            static const uint8_t tag[5] = { 'J', 'F', 'I', 'F', 0 };
            bool ok = true;
            for (int i = 0; i < 5; ++i) if (z.s.get8() != tag[i]) ok = false;
            L -= 5;
            if (ok) z.jfif = true;
        }
        else if (m == 0xEE && L >= 12) {             // Adobe APP14: the colour transform byte
            static const uint8_t tag[6] = { 'A', 'd', 'o', 'b', 'e', 0 };
            bool ok = true;
            for (int i = 0; i < 6; ++i) if (z.s.get8() != tag[i]) ok = false;
            L -= 6;
            if (ok) { z.s.get8(); z.s.get16(); z.s.get16(); z.app14Transform = static_cast<int>(z.s.get8()); L -= 6; }
        }
        z.s.skip(L);
        return true;
    }
    // SOF3, SOF5..SOF15 (lossless, hierarchical, arithmetic) and everything else
    return z.fail("unknown marker (arithmetic-coded, lossless and hierarchical JPEG are not read)");
}

bool process_scan_header(Jpeg& z) {
    const int Ls = static_cast<int>(z.s.get16());
    z.scanN = static_cast<int>(z.s.get8());
    if (z.scanN < 1 || z.scanN > 4 || z.scanN > static_cast<int>(z.imgN)) return z.fail("bad SOS component count");
    if (Ls != 6 + 2 * z.scanN) return z.fail("bad SOS len");
    for (int i = 0; i < z.scanN; ++i) {
        const uint32_t id = z.s.get8(), q = z.s.get8();
        uint32_t which = 0;
        for (; which < z.imgN; ++which) if (z.comp[which].id == id) break;
        if (which == z.imgN) return z.fail("SOS names an unknown component");
        z.comp[which].hd = q >> 4; if (z.comp[which].hd > 3) return z.fail("bad DC huff");
        z.comp[which].ha = q & 15; if (z.comp[which].ha > 3) return z.fail("bad AC huff");
        z.order[i] = static_cast<int>(which);
    }
    z.specStart = static_cast<int>(z.s.get8());
    z.specEnd = static_cast<int>(z.s.get8());
    const uint32_t aa = z.s.get8();
    z.succHigh = static_cast<int>(aa >> 4); z.succLow = static_cast<int>(aa & 15);
    if (z.progressive) {
        if (z.specStart > 63 || z.specEnd > 63 || z.specStart > z.specEnd || z.succHigh > 13 || z.succLow > 13) return z.fail("bad SOS");
    }
    else {
        if (z.specStart != 0 || z.succHigh != 0 || z.succLow != 0) return z.fail("bad SOS");
        z.specEnd = 63;
    }
    // a scan must not use a table no DHT has defined (the reference would decode with whatever its memory holds)
    for (int i = 0; i < z.scanN; ++i) {
        const Component& c = z.comp[z.order[i]];
        const bool needDc = !z.progressive || (z.specStart == 0 && z.succHigh == 0), needAc = !z.progressive || z.specStart != 0;
        if ((needDc && !z.huffDc[c.hd].defined) || (needAc && !z.huffAc[c.ha].defined)) return z.fail("scan uses an undefined Huffman table");
    }
    return true;
}

bool process_frame_header(Jpeg& z, bool headerOnly) {
    Reader& s = z.s;
    const uint32_t Lf = s.get16(); if (Lf < 11) return z.fail("bad SOF len");
    const uint32_t p = s.get8(); if (p != 8) return z.fail("only 8-bit samples are read");
    z.imgY = s.get16(); z.imgX = s.get16();
    if (too_large(z.imgX, z.imgY)) return z.fail(kTooLarge);
    if (z.imgY == 0) return z.fail("no header height");
    if (z.imgX == 0) return z.fail("0 width");
    const uint32_t c = s.get8();
    if (c != 3 && c != 1 && c != 4) return z.fail("bad component count");
    z.imgN = c;
    if (Lf != 8 + 3 * c) return z.fail("bad SOF len");
    z.rgbIds = 0;
    for (uint32_t i = 0; i < c; ++i) {
        static const uint8_t rgb[3] = { 'R', 'G', 'B' };
        Component& k = z.comp[i];
        k.id = s.get8();
        if (c == 3 && k.id == rgb[i]) ++z.rgbIds;
        const uint32_t q = s.get8();
        k.h = q >> 4; if (!k.h || k.h > 4) return z.fail("bad H");
        k.v = q & 15; if (!k.v || k.v > 4) return z.fail("bad V");
        k.tq = s.get8(); if (k.tq > 3) return z.fail("bad TQ");
    }
    if (headerOnly) return true;
    // every 8 x 8 block costs a sequential scan two bits and a progressive one one bit at the very least: ~512 pixels per byte.
    // A file far below that cannot hold the image its header claims, so it does not get the memory either.
    if (static_cast<uint64_t>(z.imgX) * z.imgY / 1024u > s.n) return z.fail("image far larger than its file can hold");
    z.hMax = z.vMax = 1;
    for (uint32_t i = 0; i < c; ++i) { if (z.comp[i].h > z.hMax) z.hMax = z.comp[i].h; if (z.comp[i].v > z.vMax) z.vMax = z.comp[i].v; }
    z.mcuX = (z.imgX + z.hMax * 8 - 1) / (z.hMax * 8);
    z.mcuY = (z.imgY + z.vMax * 8 - 1) / (z.vMax * 8);
    for (uint32_t i = 0; i < c; ++i) {
        Component& k = z.comp[i];
        k.x = (z.imgX * k.h + z.hMax - 1) / z.hMax;
        k.y = (z.imgY * k.v + z.vMax - 1) / z.vMax;
        k.w2 = z.mcuX * k.h * 8;
        k.h2 = z.mcuY * k.v * 8;
        // + a line of slack: with sampling factors that do not divide (3 : 2) the up-sampler reads a full image width from a narrower row
        k.data.assign(static_cast<size_t>(k.w2) * k.h2 + z.imgX + 16, 0);
        if (z.progressive) { k.coeffW = k.w2 / 8; k.coeff.assign(static_cast<size_t>(k.w2) * k.h2, 0); }
    }
    return true;
}

bool decode_header(Jpeg& z, bool headerOnly) {
    z.jfif = false; z.app14Transform = -1; z.marker = kMarkerNone;
    int m = get_marker(z);
    if (m != 0xD8) return z.fail("no SOI");
    m = get_marker(z);
    while (m != 0xC0 && m != 0xC1 && m != 0xC2) {
        if (!process_marker(z, m)) return false;
        m = get_marker(z);
        while (m == kMarkerNone) {                   // padding between segments
            if (z.s.eof()) return z.fail("no SOF");
            m = get_marker(z);
        }
    }
    z.progressive = m == 0xC2;
    return process_frame_header(z, headerOnly);
}

bool decode_image(Jpeg& z) {
    z.restartInterval = 0;
    if (!decode_header(z, false)) return false;
    int m = get_marker(z), scans = 0;
    while (m != 0xD9) {
        if (m == 0xDA) {
            if (++scans > 1024) return z.fail("more than 1024 scans");
            if (!process_scan_header(z)) return false;
            if (!parse_entropy_coded_data(z)) return false;
            if (z.marker == kMarkerNone) {
                // bytes between the entropy-coded data and the next marker are skipped (stb:3279-3289)
                while (!z.s.eof()) { if (z.s.get8() == 255) { z.marker = static_cast<uint8_t>(z.s.get8()); break; } }
            }
        }
        else if (m == 0xDC) {
            const uint32_t Ld = z.s.get16(), NL = z.s.get16();
            if (Ld != 4) return z.fail("bad DNL len");
            if (NL != z.imgY) return z.fail("bad DNL height");
        }
        else if (!process_marker(z, m)) return false;
        m = get_marker(z);
    }
    if (z.progressive) finish_progressive(z);
    return true;
}

// ---- up-sampling: the "JFIF-centred" triangle filters across block borders (stb:3305-3511).  `near` is the source row the
// output row lies closer to.  Each returns the row to read: `out`, or `near` itself where nothing has to be done.
typedef const uint8_t* (*ResampleFn)(uint8_t* out, const uint8_t* near, const uint8_t* far, uint32_t w, uint32_t hs);
const uint8_t* resample_1(uint8_t*, const uint8_t* near, const uint8_t*, uint32_t, uint32_t) { return near; }
const uint8_t* resample_v2(uint8_t* out, const uint8_t* near, const uint8_t* far, uint32_t w, uint32_t) {
    for (uint32_t i = 0; i < w; ++i) out[i] = static_cast<uint8_t>((3 * near[i] + far[i] + 2) >> 2);
    return out;
}
const uint8_t* resample_h2(uint8_t* out, const uint8_t* in, const uint8_t*, uint32_t w, uint32_t) {
    if (w == 1) { out[0] = out[1] = in[0]; return out; }
    out[0] = in[0];
    out[1] = static_cast<uint8_t>((in[0] * 3 + in[1] + 2) >> 2);
    uint32_t i;
    for (i = 1; i + 1 < w; ++i) {
        const int n = 3 * in[i] + 2;
        out[i * 2] = static_cast<uint8_t>((n + in[i - 1]) >> 2);
        out[i * 2 + 1] = static_cast<uint8_t>((n + in[i + 1]) >> 2);
    }
    out[i * 2] = static_cast<uint8_t>((in[w - 2] * 3 + in[w - 1] + 2) >> 2);
    out[i * 2 + 1] = in[w - 1];
    return out;
}
const uint8_t* resample_hv2(uint8_t* out, const uint8_t* near, const uint8_t* far, uint32_t w, uint32_t) {
    if (w == 1) { out[0] = out[1] = static_cast<uint8_t>((3 * near[0] + far[0] + 2) >> 2); return out; }
    int t1 = 3 * near[0] + far[0];
    out[0] = static_cast<uint8_t>((t1 + 2) >> 2);
    for (uint32_t i = 1; i < w; ++i) {
        const int t0 = t1;
        t1 = 3 * near[i] + far[i];
        out[i * 2 - 1] = static_cast<uint8_t>((3 * t0 + t1 + 8) >> 4);
        out[i * 2] = static_cast<uint8_t>((3 * t1 + t0 + 8) >> 4);
    }
    out[w * 2 - 1] = static_cast<uint8_t>((t1 + 2) >> 2);
    return out;
}
const uint8_t* resample_generic(uint8_t* out, const uint8_t* near, const uint8_t*, uint32_t w, uint32_t hs) {
    for (uint32_t i = 0; i < w; ++i) for (uint32_t j = 0; j < hs; ++j) out[i * hs + j] = near[i];      // replication
    return out;
}

// YCbCr -> RGB in 20-bit fixed point (stb:3513-3539): constants (int)(c * 4096 + 0.5) << 8, the Cb term of green masked to its
// upper 16 bits before it is added
constexpr int fix20(float x) { return static_cast<int>(x * 4096.0f + 0.5f) << 8; }
inline uint8_t clamp_px(int v) { return v < 0 ? 0 : v > 255 ? 255 : static_cast<uint8_t>(v); }
void ycbcr_to_rgba(uint8_t* out, const uint8_t* y, const uint8_t* pcb, const uint8_t* pcr, uint32_t count) {
    for (uint32_t i = 0; i < count; ++i, out += 4) {
        const int yFixed = (y[i] << 20) + (1 << 19);
        const int cr = pcr[i] - 128, cb = pcb[i] - 128;
        const int r = yFixed + cr * fix20(1.40200f);
        const int g = yFixed + cr * -fix20(0.71414f) + static_cast<int>(static_cast<uint32_t>(cb * -fix20(0.34414f)) & 0xFFFF0000u);
        const int b = yFixed + cb * fix20(1.77200f);
        out[0] = clamp_px(r >> 20); out[1] = clamp_px(g >> 20); out[2] = clamp_px(b >> 20); out[3] = 255;
    }
}
inline uint8_t mul8(uint32_t x, uint32_t y) { const uint32_t t = x * y + 128; return static_cast<uint8_t>((t + (t >> 8)) >> 8); }     // round(x y / 255)

// stb:3721-3878 with req_comp = 4
bool jpeg_to_rgba(Jpeg& z, std::vector<uint8_t>& rgba) {
    // three components are R, G, B when their ids say so, or when an Adobe marker says "no transform" and there is no JFIF marker
    const bool isRgb = z.imgN == 3 && (z.rgbIds == 3 || (z.app14Transform == 0 && !z.jfif));
    struct Resample { ResampleFn fn; const uint8_t* line0; const uint8_t* line1; uint32_t hs, vs, wLores, ystep, ypos; } res[4];
    for (uint32_t k = 0; k < z.imgN; ++k) {
        Component& c = z.comp[k];
        Resample& r = res[k];
        c.linebuf.assign(static_cast<size_t>(z.imgX) + 3, 0);
        r.hs = z.hMax / c.h; r.vs = z.vMax / c.v;
        r.ystep = r.vs >> 1;
        r.wLores = (z.imgX + r.hs - 1) / r.hs;
        r.ypos = 0;
        r.line0 = r.line1 = c.data.data();
        if (r.hs == 1 && r.vs == 1) r.fn = resample_1;
        else if (r.hs == 1 && r.vs == 2) r.fn = resample_v2;
        else if (r.hs == 2 && r.vs == 1) r.fn = resample_h2;
        else if (r.hs == 2 && r.vs == 2) r.fn = resample_hv2;
        else r.fn = resample_generic;
    }
    rgba.assign(4ull * z.imgX * z.imgY, 0);
    const uint8_t* co[4] = { nullptr, nullptr, nullptr, nullptr };
    for (uint32_t j = 0; j < z.imgY; ++j) {
        uint8_t* out = rgba.data() + 4ull * z.imgX * j;
        for (uint32_t k = 0; k < z.imgN; ++k) {
            Resample& r = res[k];
            // the output row lies in the lower half of its source row's span when ystep >= vs / 2: then line1 is the near one
            const bool yBot = r.ystep >= (r.vs >> 1);
            co[k] = r.fn(z.comp[k].linebuf.data(), yBot ? r.line1 : r.line0, yBot ? r.line0 : r.line1, r.wLores, r.hs);
            if (++r.ystep >= r.vs) {
                r.ystep = 0;
                r.line0 = r.line1;
                if (++r.ypos < z.comp[k].y) r.line1 += z.comp[k].w2;
            }
        }
        if (z.imgN == 3) {
            if (isRgb) for (uint32_t i = 0; i < z.imgX; ++i, out += 4) { out[0] = co[0][i]; out[1] = co[1][i]; out[2] = co[2][i]; out[3] = 255; }
            else ycbcr_to_rgba(out, co[0], co[1], co[2], z.imgX);
        }
        else if (z.imgN == 4) {
            if (z.app14Transform == 0) {             // CMYK (stored inverted, as Adobe writes it): colour times K
                for (uint32_t i = 0; i < z.imgX; ++i, out += 4) {
                    const uint32_t m = co[3][i];
                    out[0] = mul8(co[0][i], m); out[1] = mul8(co[1][i], m); out[2] = mul8(co[2][i], m); out[3] = 255;
                }
            }
            else {
                ycbcr_to_rgba(out, co[0], co[1], co[2], z.imgX);
                if (z.app14Transform == 2)               // YCCK; any other value: the fourth channel is ignored
                    for (uint32_t i = 0; i < z.imgX; ++i, out += 4) {
                        const uint32_t m = co[3][i];
                        out[0] = mul8(255u - out[0], m); out[1] = mul8(255u - out[1], m); out[2] = mul8(255u - out[2], m);
                    }
            }
        }
        else for (uint32_t i = 0; i < z.imgX; ++i, out += 4) { out[0] = out[1] = out[2] = co[0][i]; out[3] = 255; }
    }
    return true;
}

// =====================================================================================================================
// PNG writer
// =====================================================================================================================
uint32_t crc32_update(uint32_t crc, const uint8_t* p, size_t n) {
    uint32_t table[256];                             // built per call (three calls per file): no state outside the function
    for (uint32_t i = 0; i < 256; ++i) { uint32_t c = i; for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1; table[i] = c; }
    for (size_t i = 0; i < n; ++i) crc = table[(crc ^ p[i]) & 255u] ^ (crc >> 8);
    return crc;
}
void put32(std::vector<uint8_t>& f, uint32_t v) { f.push_back(static_cast<uint8_t>(v >> 24)); f.push_back(static_cast<uint8_t>(v >> 16)); f.push_back(static_cast<uint8_t>(v >> 8)); f.push_back(static_cast<uint8_t>(v)); }
void put_chunk(std::vector<uint8_t>& f, const char* type, const uint8_t* body, size_t n) {
    put32(f, static_cast<uint32_t>(n));
    const size_t at = f.size();
    f.insert(f.end(), type, type + 4);
    if (n) f.insert(f.end(), body, body + n);
    put32(f, crc32_update(0xFFFFFFFFu, f.data() + at, n + 4) ^ 0xFFFFFFFFu);
}
struct BitWriter {
    std::vector<uint8_t>& out; uint32_t acc = 0; int have = 0;
    explicit BitWriter(std::vector<uint8_t>& o) : out(o) {}
    void bits(uint32_t v, int n) { acc |= v << have; have += n; while (have >= 8) { out.push_back(static_cast<uint8_t>(acc)); acc >>= 8; have -= 8; } }
    void code(uint32_t c, int n) { uint32_t r = 0; for (int i = 0; i < n; ++i) r |= ((c >> i) & 1u) << (n - 1 - i); bits(r, n); }     // Huffman codes go in MSB first
    void flush() { if (have) { out.push_back(static_cast<uint8_t>(acc)); acc = 0; have = 0; } }
};
// one deflate stream of a single fixed-Huffman block (RFC 1951 3.2.6); matches from a one-entry hash table of 3-byte strings
void deflate_fixed(const uint8_t* src, size_t n, std::vector<uint8_t>& out) {
    static const uint16_t lenBase[29] = { 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258 };
    static const uint8_t lenExtra[29] = { 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0 };
    static const uint16_t distBase[30] = { 1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577 };
    static const uint8_t distExtra[30] = { 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13 };
    BitWriter bw(out);
    bw.bits(1, 1); bw.bits(1, 2);                    // BFINAL, BTYPE = 01
    auto literal = [&](uint32_t v) {
        if (v < 144) bw.code(0x30 + v, 8); else if (v < 256) bw.code(0x190 + v - 144, 9);
        else if (v < 280) bw.code(v - 256, 7); else bw.code(0xC0 + v - 280, 8);
    };
    constexpr uint32_t kHashBits = 15;
    std::vector<uint32_t> head(1u << kHashBits, 0xFFFFFFFFu);
    size_t i = 0;
    while (i < n) {
        size_t len = 0, dist = 0;
        if (i + 3 <= n) {
            const uint32_t h = ((src[i] | (src[i + 1] << 8) | (static_cast<uint32_t>(src[i + 2]) << 16)) * 2654435761u) >> (32 - kHashBits);
            const uint32_t cand = head[h];
            head[h] = static_cast<uint32_t>(i);
            if (cand != 0xFFFFFFFFu && i - cand <= 32768) {
                const size_t maxLen = n - i < 258 ? n - i : 258;
                while (len < maxLen && src[cand + len] == src[i + len]) ++len;
                dist = i - cand;
            }
        }
        if (len >= 3) {
            int lc = 28; while (lenBase[lc] > len) --lc;
            literal(257 + lc); bw.bits(static_cast<uint32_t>(len - lenBase[lc]), lenExtra[lc]);
            int dc = 29; while (distBase[dc] > dist) --dc;
            bw.code(dc, 5); bw.bits(static_cast<uint32_t>(dist - distBase[dc]), distExtra[dc]);
            i += len;
        }
        else literal(src[i++]);
    }
    literal(256);
    bw.flush();
}

} // namespace

// =====================================================================================================================
// entry points: nothing throws past them
// =====================================================================================================================
Kind sniff(const uint8_t* data, size_t bytes) {
    if (bytes >= 8 && std::memcmp(data, kPngSignature, 8) == 0) return kKindPng;
    if (bytes >= 3 && data[0] == 0xFF && data[1] == 0xD8 && data[2] == 0xFF) return kKindJpeg;
    return kKindNone;
}

bool png_info(const uint8_t* data, size_t bytes, Info& info, std::string& err) {
    try {
        PngHeader hd;
        if (!png_parse(data, bytes, true, hd, err)) return false;
        info.width = hd.w; info.height = hd.h; info.channels = hd.channels(); info.kind = kKindPng;
        return true;
    }
    catch (const std::exception& e) { err = std::string("PNG: ") + e.what(); return false; }
}
bool png_decode(const uint8_t* data, size_t bytes, Info& info, std::vector<uint8_t>& rgba, std::string& err) {
    try { return png_decode_impl(data, bytes, info, rgba, err); }
    catch (const std::bad_alloc&) { err = "PNG: out of memory for the image"; return false; }
    catch (const std::exception& e) { err = std::string("PNG: ") + e.what(); return false; }
}
bool jpeg_info(const uint8_t* data, size_t bytes, Info& info, std::string& err) {
    try {
        Jpeg z(data, bytes);
        if (!decode_header(z, true)) { err = z.err; return false; }
        info.width = z.imgX; info.height = z.imgY; info.channels = z.imgN >= 3 ? 3u : 1u; info.kind = kKindJpeg;
        return true;
    }
    catch (const std::exception& e) { err = std::string("JPEG: ") + e.what(); return false; }
}
bool jpeg_decode(const uint8_t* data, size_t bytes, Info& info, std::vector<uint8_t>& rgba, std::string& err) {
    try {
        Jpeg z(data, bytes);
        if (!decode_image(z)) { err = z.err; return false; }
        info.width = z.imgX; info.height = z.imgY; info.channels = z.imgN >= 3 ? 3u : 1u; info.kind = kKindJpeg;     // CMYK reports 3, as the reference does
        return jpeg_to_rgba(z, rgba);
    }
    catch (const std::bad_alloc&) { err = "JPEG: out of memory for the image"; return false; }
    catch (const std::exception& e) { err = std::string("JPEG: ") + e.what(); return false; }
}
bool info(const uint8_t* data, size_t bytes, Info& out, std::string& err) {
    switch (sniff(data, bytes)) {
    case kKindPng: return png_info(data, bytes, out, err);
    case kKindJpeg: return jpeg_info(data, bytes, out, err);
    default: err = "neither a PNG nor a JPEG file"; return false;
    }
}
bool decode(const uint8_t* data, size_t bytes, Info& out, std::vector<uint8_t>& rgba, std::string& err) {
    switch (sniff(data, bytes)) {
    case kKindPng: return png_decode(data, bytes, out, rgba, err);
    case kKindJpeg: return jpeg_decode(data, bytes, out, rgba, err);
    default: err = "neither a PNG nor a JPEG file"; return false;
    }
}

bool png_encode_rgba8(const uint8_t* rgba, uint32_t width, uint32_t height, std::vector<uint8_t>& file, std::string& err) {
    if (!width || !height || too_large(width, height)) { err = "PNG: image empty or larger than 16384 x 16384"; return false; }
    try {
        const size_t row = 4ull * width;
        std::vector<uint8_t> raw((row + 1) * height);
        uint32_t a = 1, b = 0;                       // Adler-32 of the filtered lines
        for (uint32_t y = 0; y < height; ++y) {
            uint8_t* line = raw.data() + (row + 1) * y;
            line[0] = 0;                                 // filter type None
            std::memcpy(line + 1, rgba + row * y, row);
        }
        for (size_t i = 0; i < raw.size();) {
            const size_t end = raw.size() - i < 5552 ? raw.size() : i + 5552;     // the longest run that cannot overflow 32 bits
            for (; i < end; ++i) { a += raw[i]; b += a; }
            a %= 65521u; b %= 65521u;
        }
        std::vector<uint8_t> z;
        z.reserve(raw.size() / 2 + 64);
        z.push_back(0x78); z.push_back(0x01);
        deflate_fixed(raw.data(), raw.size(), z);
        put32(z, (b << 16) | a);
        file.clear();
        file.insert(file.end(), kPngSignature, kPngSignature + 8);
        uint8_t ihdr[13] = { static_cast<uint8_t>(width >> 24), static_cast<uint8_t>(width >> 16), static_cast<uint8_t>(width >> 8), static_cast<uint8_t>(width),
                             static_cast<uint8_t>(height >> 24), static_cast<uint8_t>(height >> 16), static_cast<uint8_t>(height >> 8), static_cast<uint8_t>(height), 8, 6, 0, 0, 0 };
        put_chunk(file, "IHDR", ihdr, 13);
        put_chunk(file, "IDAT", z.data(), z.size());
        put_chunk(file, "IEND", nullptr, 0);
        return true;
    }
    catch (const std::exception& e) { err = std::string("PNG: ") + e.what(); return false; }
}

} // namespace gfx_img
