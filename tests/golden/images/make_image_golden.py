"""Generate tests/golden/images/image_inputs.npz and image_expected.npz: PNG / JPEG files and what the reference's decoder makes of them.

Run at development time only (needs the reference tree, g++ and Pillow):
    python tests/golden/images/make_image_golden.py
It writes the input files (Pillow where Pillow can write the variant; a small PNG packer and a baseline JPEG writer of this file for
the rest), writes a short driver of its own that calls stbi_load(path, &w, &h, &n, 4), compiles it in a temporary directory against
the reference's ext/ directory -- once as it is, once with -DSTBI_NO_SIMD, asserting that both give the same bytes -- and stores per
file w, h, n and the RGBA bytes, or the refusal.  The committed .npz files are data only: neither the driver, nor its binary, nor
any text of the reference is stored.

image_inputs.npz     <name> -> the bytes of the file (uint8)
image_expected.npz   <name>.whn -> (w, h, n); <name>.rgba -> uint8 [h, w, 4]   for a file the reference decodes
                     <name>.refused -> the reference's reason (str)                for a file it refuses
                     <name>.oversize -> (w, h, n)  for a file the reference decodes but the library refuses (a side above 16384)
"""
import io
import os
import struct
import subprocess
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_EXT = os.environ.get("GFX_REFERENCE_EXT", "/root/reference/ext")

# `driver files...` decodes each file and writes <file>.rgba; `driver --time files...` prints the best of five decode times in seconds
# instead (tools/bench_image_decode.py builds this same text with -O2)
DRIVER = r"""
#define STB_IMAGE_IMPLEMENTATION
#include "stb_image.h"
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
int main(int argc, char** argv) {
    const bool timing = argc > 1 && !std::strcmp(argv[1], "--time");
    for (int i = timing ? 2 : 1; i < argc; ++i) {
        int w = 0, h = 0, n = 0;
        double best = 1e30;
        unsigned char* px = nullptr;
        for (int k = 0; k < (timing ? 5 : 1); ++k) {
            if (px) stbi_image_free(px);
            const auto t0 = std::chrono::steady_clock::now();
            px = stbi_load(argv[i], &w, &h, &n, 4);
            const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (s < best) best = s;
        }
        if (!px) { std::printf("%s\tREFUSED\t%s\n", argv[i], stbi_failure_reason()); continue; }
        if (timing) std::printf("%s\tTIME\t%.6f\n", argv[i], best);
        else {
            std::printf("%s\tOK\t%d %d %d\n", argv[i], w, h, n);
            FILE* f = std::fopen((std::string(argv[i]) + ".rgba").c_str(), "wb");
            std::fwrite(px, 1, (size_t)w * h * 4, f);
            std::fclose(f);
        }
        stbi_image_free(px);
    }
    return 0;
}
"""


# ------------------------------------------------------------------------------------------------------------------ test pictures
def picture(w, h, seed=1):
    """float RGBA in 0..1: smooth ramps, a hard edge, a little noise -- so that every filter, the chroma up-samplers and both the
    flat and the busy paths of the inverse DCT see something"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    u, v = x / max(w - 1, 1), y / max(h - 1, 1)
    img = np.stack([u, 0.5 + 0.5 * np.sin(6.0 * v + 3.0 * u), (u * v) ** 0.5, 1.0 - 0.8 * u * (1 - v)], axis=-1)
    img[h // 3: h // 2, w // 4: w // 2, :3] = (0.9, 0.1, 0.2)
    img[..., :3] += rng.normal(0, 0.04, (h, w, 3))
    return np.clip(img, 0, 1)


# --------------------------------------------------------------------------------------------------------------------- PNG packer
def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def _filter_line(ftype, line, prior, bpp):
    line = np.frombuffer(line, np.uint8).astype(np.int32)
    prior = np.frombuffer(prior, np.uint8).astype(np.int32)
    a = np.concatenate([np.zeros(bpp, np.int32), line[:-bpp]]) if len(line) > bpp else np.zeros(len(line), np.int32)
    c = np.concatenate([np.zeros(bpp, np.int32), prior[:-bpp]]) if len(line) > bpp else np.zeros(len(line), np.int32)
    if ftype == 0 or ftype > 4:
        pred = 0
    elif ftype == 1:
        pred = a
    elif ftype == 2:
        pred = prior
    elif ftype == 3:
        pred = (a + prior) >> 1
    else:
        p = a + prior - c
        pa, pb, pc = abs(p - a), abs(p - prior), abs(p - c)
        pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, prior, c))
    return bytes([ftype]) + ((line - pred) & 255).astype(np.uint8).tobytes()


def _pack_lines(samples, depth):
    """samples: int array [h, w, ch] of `depth`-bit values -> one bytes object per line"""
    h, w, ch = samples.shape
    out = []
    for y in range(h):
        flat = samples[y].reshape(-1)
        if depth == 16:
            out.append(flat.astype(">u2").tobytes())
        elif depth == 8:
            out.append(flat.astype(np.uint8).tobytes())
        else:
            per = 8 // depth
            pad = (-len(flat)) % per
            f = np.concatenate([flat, np.zeros(pad, flat.dtype)]).reshape(-1, per).astype(np.uint32)
            shifts = np.arange(per - 1, -1, -1) * depth
            out.append((f << shifts).sum(axis=1).astype(np.uint8).tobytes())
    return out


def pack_png(samples, depth, colour, filters=(0,), interlace=False, palette=None, trns=None, level=6, idat_split=0, extra=()):
    """samples [h, w, ch] ints.  filters: cycled over the lines (a value above 4 is written as it is, for the refusal group)."""
    h, w, ch = samples.shape
    bpp = max(1, ch * depth // 8)
    raw = b""
    passes = [(0, 0, 1, 1)] if not interlace else [(0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)]
    k = 0
    for xo, yo, xs, ys in passes:
        sub = samples[yo::ys, xo::xs]
        if sub.shape[0] == 0 or sub.shape[1] == 0:
            continue
        lines = _pack_lines(sub, depth)
        prior = bytes(len(lines[0]))
        for line in lines:
            raw += _filter_line(filters[k % len(filters)], line, prior, bpp)
            prior = line
            k += 1
    z = zlib.compress(raw, level)
    out = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour, 0, 0, 1 if interlace else 0))
    for kind, body in extra:
        out += _chunk(kind, body)
    if palette is not None:
        out += _chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes())
    if trns is not None:
        out += _chunk(b"tRNS", trns)
    if idat_split:
        for i in range(0, len(z), idat_split):
            out += _chunk(b"IDAT", z[i:i + idat_split])
    else:
        out += _chunk(b"IDAT", z)
    return out + _chunk(b"IEND", b"")


def quant(img, depth):
    return np.round(img * ((1 << depth) - 1)).astype(np.int64)


def make_pngs():
    from PIL import Image
    W, H = 53, 37
    pic = picture(W, H)
    files = {}

    def pil(name, im, **kw):
        b = io.BytesIO()
        im.save(b, "PNG", **kw)
        files[name] = b.getvalue()

    rgb8 = quant(pic[..., :3], 8)
    rgba8 = quant(pic, 8)
    g8 = quant(pic[..., 1:2], 8)
    pil("rgb8.png", Image.fromarray(rgb8.astype(np.uint8), "RGB"))
    pil("rgba8.png", Image.fromarray(rgba8.astype(np.uint8), "RGBA"))
    pil("g8.png", Image.fromarray(g8[..., 0].astype(np.uint8), "L"))
    pil("la8.png", Image.fromarray(np.concatenate([g8, rgba8[..., 3:]], -1).astype(np.uint8), "LA"))
    pal_im = Image.fromarray(rgb8.astype(np.uint8), "RGB").quantize(200)
    pil("pal8.png", pal_im)
    pil("g1.png", Image.fromarray((pic[..., 1] > 0.5).astype(np.uint8) * 255, "L").convert("1"))
    pil("g16.png", Image.fromarray(quant(pic[..., 1], 16).astype(np.uint16)))
    # own packer: palettes of 2 / 4 / 16 entries, low-depth grey, 16 bit, every filter, stored deflate, tRNS, tiny sizes, Adam7
    rng = np.random.default_rng(7)
    for bits in (1, 2, 4):
        pal = rng.integers(0, 256, (1 << bits, 3))
        idx = quant(pic[..., 0:1], bits)
        files["pal%d.png" % bits] = pack_png(idx, bits, 3, palette=pal, filters=(0, 1, 2, 3, 4))
    pal16 = rng.integers(0, 256, (16, 3))
    idx4 = quant(pic[..., 2:3], 4)
    files["pal4_trns.png"] = pack_png(idx4, 4, 3, palette=pal16, trns=bytes(rng.integers(0, 256, 11).astype(np.uint8)), filters=(4, 2))
    files["g2.png"] = pack_png(quant(pic[..., 1:2], 2), 2, 0, filters=(1, 3))
    files["g4.png"] = pack_png(quant(pic[..., 1:2], 4), 4, 0, filters=(4,), extra=[(b"gAMA", struct.pack(">I", 45455)), (b"tEXt", b"Comment\0ancillary chunks are skipped")])
    files["ga16.png"] = pack_png(quant(pic[..., [1, 3]], 16), 16, 4, filters=(0, 1, 2, 3, 4))
    files["rgb16.png"] = pack_png(quant(pic[..., :3], 16), 16, 2, filters=(3, 4))
    files["rgba16.png"] = pack_png(quant(pic, 16), 16, 6, filters=(4, 3, 2, 1), idat_split=97)
    for f in range(5):
        files["rgb8_filter%d.png" % f] = pack_png(rgb8, 8, 2, filters=(f,))
    files["rgb8_stored.png"] = pack_png(rgb8, 8, 2, filters=(0, 1), level=0)
    files["g8_trns.png"] = pack_png(g8, 8, 0, trns=struct.pack(">H", int(g8[5, 5, 0])), filters=(2,))
    files["g4_trns.png"] = pack_png(quant(pic[..., 1:2], 4), 4, 0, trns=struct.pack(">H", int(quant(pic[..., 1:2], 4)[5, 5, 0])), filters=(1,))
    files["rgb8_trns.png"] = pack_png(rgb8, 8, 2, trns=struct.pack(">HHH", *[int(c) for c in rgb8[H // 3 + 1, W // 4 + 1]]), filters=(1,))
    rgb16 = quant(pic[..., :3], 16)
    rgb16[2:9, 3:11] = rgb16[2, 3]            # a patch of the key colour, and next to it one that differs in the low byte only
    rgb16[12:15, 3:11] = rgb16[2, 3] ^ 1
    files["rgb16_trns.png"] = pack_png(rgb16, 16, 2, trns=struct.pack(">HHH", *[int(c) for c in rgb16[2, 3]]), filters=(4,))
    files["rgb8_1x1.png"] = pack_png(rgb8[:1, :1], 8, 2, filters=(4,))
    files["rgba8_3x5.png"] = pack_png(rgba8[:5, :3], 8, 6, filters=(3, 4, 1))
    p23 = picture(23, 19, seed=3)               # 23 x 19: every Adam7 pass has a partial edge
    files["adam7_g2.png"] = pack_png(quant(p23[..., 1:2], 2), 2, 0, filters=(0, 1, 2, 3, 4), interlace=True)
    files["adam7_g4.png"] = pack_png(quant(p23[..., 1:2], 4), 4, 0, filters=(4, 3), interlace=True)
    files["adam7_ga16.png"] = pack_png(quant(p23[..., [1, 3]], 16), 16, 4, filters=(1, 2, 3, 4), interlace=True)
    files["adam7_rgb8.png"] = pack_png(quant(p23[..., :3], 8), 8, 2, filters=(4, 3, 2, 1, 0), interlace=True)
    files["adam7_rgb16.png"] = pack_png(quant(p23[..., :3], 16), 16, 2, filters=(3,), interlace=True)
    files["adam7_rgba16.png"] = pack_png(quant(p23, 16), 16, 6, filters=(4,), interlace=True, idat_split=61)
    files["adam7_pal4_trns.png"] = pack_png(quant(p23[..., 2:3], 4), 4, 3, palette=pal16, trns=bytes(rng.integers(0, 256, 16).astype(np.uint8)), filters=(2, 4), interlace=True)
    files["adam7_rgb8_2x3.png"] = pack_png(quant(p23[:3, :2, :3], 8), 8, 2, filters=(1,), interlace=True)      # several passes are empty
    return files


# ------------------------------------------------------------------------------------------------------------ baseline JPEG writer
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


def parse_dht(jpeg):
    """{(class, id): (counts[16], values)} of a finished file: the writer below borrows the standard tables from a Pillow file"""
    tables, at = {}, 2
    while at < len(jpeg):
        assert jpeg[at] == 0xFF
        m, L = jpeg[at + 1], struct.unpack(">H", jpeg[at + 2:at + 4])[0]
        if m == 0xC4:
            p, end = at + 4, at + 2 + L
            while p < end:
                tc, th = jpeg[p] >> 4, jpeg[p] & 15
                counts = list(jpeg[p + 1:p + 17])
                n = sum(counts)
                tables[(tc, th)] = (counts, list(jpeg[p + 17:p + 17 + n]))
                p += 17 + n
        if m == 0xDA:
            break
        at += 2 + L
    return tables


def _codes(counts, values):
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[values[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def write_jpeg(planes, width, height, tables, qtable, jfif=True, sof=0xC0):
    """planes: [(id, h, v, samples uint8 [rows, cols] at the component's own resolution)], one interleaved baseline scan.
    Component 0 uses tables 0, the others tables 1; every component uses quantisation table 0."""
    hmax, vmax = max(p[1] for p in planes), max(p[2] for p in planes)
    mx, my = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    k = np.arange(8)
    D = np.sqrt(2 / 8) * np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16)
    D[0] /= np.sqrt(2)
    coeffs = []
    for _, h, v, s in planes:
        pad = np.pad(s.astype(np.float64), ((0, my * v * 8 - s.shape[0]), (0, mx * h * 8 - s.shape[1])), mode="edge") - 128.0
        blocks = pad.reshape(my * v, 8, mx * h, 8).transpose(0, 2, 1, 3)
        c = np.einsum("ij,abjk,lk->abil", D, blocks, D)
        coeffs.append(np.round(c / qtable.reshape(8, 8)).astype(np.int64).reshape(my * v, mx * h, 64)[..., ZIGZAG])
    enc = {key: _codes(*tab) for key, tab in tables.items()}
    bits = []

    def put(code, length):
        bits.append(format(code, "0%db" % length) if length else "")

    def magnitude(vv):
        size = int(abs(vv)).bit_length()
        return size, (vv if vv >= 0 else vv + (1 << size) - 1)

    pred = [0] * len(planes)
    for j in range(my):
        for i in range(mx):
            for ci, (_, h, v, _s) in enumerate(planes):
                t = 0 if ci == 0 else 1
                for y in range(v):
                    for x in range(h):
                        zz = coeffs[ci][j * v + y, i * h + x]
                        size, extra = magnitude(int(zz[0]) - pred[ci])
                        pred[ci] = int(zz[0])
                        put(*enc[(0, t)][size]); put(extra, size)
                        run = 0
                        last = max([q for q in range(1, 64) if zz[q]], default=0)
                        for q in range(1, last + 1):
                            if zz[q] == 0:
                                run += 1
                                continue
                            while run > 15:
                                put(*enc[(1, t)][0xF0]); run -= 16
                            size, extra = magnitude(int(zz[q]))
                            put(*enc[(1, t)][(run << 4) | size]); put(extra, size)
                            run = 0
                        if last < 63:
                            put(*enc[(1, t)][0x00])
    s = "".join(bits)
    s += "1" * ((-len(s)) % 8)
    data = bytes(int(s[i:i + 8], 2) for i in range(0, len(s), 8)).replace(b"\xff", b"\xff\x00")
    out = b"\xff\xd8"
    if jfif:
        out += b"\xff\xe0" + struct.pack(">H", 16) + b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0"
    out += b"\xff\xdb" + struct.pack(">HB", 67, 0) + bytes(int(q) for q in qtable[ZIGZAG])
    out += bytes([0xFF, sof]) + struct.pack(">HBHHB", 8 + 3 * len(planes), 8, height, width, len(planes))
    for cid, h, v, _ in planes:
        out += bytes([cid, (h << 4) | v, 0])
    for (tc, th), (counts, values) in sorted(tables.items()):
        out += b"\xff\xc4" + struct.pack(">HB", 19 + len(values), (tc << 4) | th) + bytes(counts) + bytes(values)
    out += b"\xff\xda" + struct.pack(">HB", 6 + 2 * len(planes), len(planes))
    for ci, (cid, _, _, _) in enumerate(planes):
        out += bytes([cid, 0x00 if ci == 0 else 0x11])
    return out + b"\x00\x3f\x00" + data + b"\xff\xd9"


def box_down(a, fy, fx):
    h, w = a.shape
    a = np.pad(a, ((0, (-h) % fy), (0, (-w) % fx)), mode="edge")
    return np.round(a.reshape(a.shape[0] // fy, fy, a.shape[1] // fx, fx).mean(axis=(1, 3))).astype(np.uint8)


def make_jpegs():
    from PIL import Image
    W, H = 53, 37
    pic = picture(W, H, seed=2)
    rgb = Image.fromarray(quant(pic[..., :3], 8).astype(np.uint8), "RGB")
    big = Image.fromarray(quant(picture(64, 64, seed=4)[..., :3], 8).astype(np.uint8), "RGB")
    files = {}

    def pil(name, im, **kw):
        b = io.BytesIO()
        im.save(b, "JPEG", **kw)
        files[name] = b.getvalue()

    pil("base444.jpg", rgb, quality=85, subsampling=0)
    pil("base422.jpg", rgb, quality=85, subsampling=1)
    pil("base420.jpg", rgb, quality=85, subsampling=2)
    pil("prog444.jpg", rgb, quality=85, subsampling=0, progressive=True)
    pil("prog420.jpg", rgb, quality=85, subsampling=2, progressive=True)
    pil("prog422_64.jpg", big, quality=90, subsampling=1, progressive=True)
    pil("optimised.jpg", rgb, quality=85, subsampling=2, optimize=True)
    pil("restart3.jpg", rgb, quality=85, subsampling=2, restart_marker_blocks=3)
    pil("q30.jpg", rgb, quality=30, subsampling=2)
    pil("q100.jpg", rgb, quality=100, subsampling=0)
    pil("grey_base.jpg", rgb.convert("L"), quality=85)
    pil("grey_prog.jpg", rgb.convert("L"), quality=85, progressive=True)
    pil("cmyk_adobe.jpg", rgb.convert("CMYK"), quality=85)
    pil("base420_1x1.jpg", rgb.crop((0, 0, 1, 1)), quality=85, subsampling=2)
    pil("base420_9x17.jpg", rgb.crop((0, 0, 9, 17)), quality=85, subsampling=2)
    pil("base420_16x16.jpg", rgb.crop((0, 0, 16, 16)), quality=85, subsampling=2)
    pil("prog420_restart2.jpg", rgb, quality=75, subsampling=2, progressive=True, restart_marker_blocks=2)
    # what Pillow cannot write: 4:4:0 (the vertical-only up-sampler), luma 4 x 1 (the replicating one), R G B component ids without a
    # JFIF marker (no colour transform), and SOF1 (a byte patch of a baseline file)
    tables = parse_dht(files["base420.jpg"])
    q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                  18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]) // 2 + 1
    ycc = np.asarray(rgb.convert("YCbCr"))
    Y, Cb, Cr = ycc[..., 0], ycc[..., 1], ycc[..., 2]
    files["own_440.jpg"] = write_jpeg([(1, 1, 2, Y), (2, 1, 1, box_down(Cb, 2, 1)), (3, 1, 1, box_down(Cr, 2, 1))], W, H, tables, q)
    files["own_h4v1.jpg"] = write_jpeg([(1, 4, 1, Y), (2, 1, 1, box_down(Cb, 1, 4)), (3, 1, 1, box_down(Cr, 1, 4))], W, H, tables, q)
    files["own_h1v4_h2v2.jpg"] = write_jpeg([(1, 2, 4, Y), (2, 1, 1, box_down(Cb, 4, 2)), (3, 2, 2, box_down(Cr, 2, 1))], W, H, tables, q)
    files["own_444_1wide.jpg"] = write_jpeg([(1, 2, 2, Y[:, :1]), (2, 1, 1, Cb[::2, :1]), (3, 1, 1, Cr[::2, :1])], 1, H, tables, q)
    files["own_422_1wide.jpg"] = write_jpeg([(1, 2, 1, Y[:, :1]), (2, 1, 1, Cb[:, :1]), (3, 1, 1, Cr[:, :1])], 1, H, tables, q)
    r8 = np.asarray(rgb)
    files["own_rgb_ids.jpg"] = write_jpeg([(ord("R"), 1, 1, r8[..., 0]), (ord("G"), 1, 1, r8[..., 1]), (ord("B"), 1, 1, r8[..., 2])], W, H, tables, q, jfif=False)
    files["sof1_patch.jpg"] = files["base422.jpg"].replace(b"\xff\xc0", b"\xff\xc1", 1)
    return files


def patch_sof(jpeg, marker=None, precision=None, width=None):
    at = jpeg.index(b"\xff\xc0")
    b = bytearray(jpeg)
    if marker is not None:
        b[at + 1] = marker
    if precision is not None:
        b[at + 4] = precision
    if width is not None:
        b[at + 7:at + 9] = struct.pack(">H", width)
    return bytes(b)


def make_refusals(pngs, jpegs):
    from PIL import Image
    base = jpegs["base420.jpg"]
    files = {
        "refuse_sof3.jpg": patch_sof(base, marker=0xC3),
        "refuse_sof9.jpg": patch_sof(base, marker=0xC9),
        "refuse_12bit.jpg": patch_sof(base, precision=12),
        "refuse_zero_width.jpg": patch_sof(base, width=0),
    }
    p = bytearray(pngs["rgb8_filter0.png"])
    p[16:20] = struct.pack(">I", 0)
    files["refuse_zero_width.png"] = bytes(p)
    p = bytearray(pngs["rgb8_filter0.png"])
    p[24] = 3
    files["refuse_depth3.png"] = bytes(p)
    files["refuse_filter7.png"] = pack_png(quant(picture(9, 7)[..., :3], 8), 8, 2, filters=(0, 7))
    wide = np.zeros((1, 20000, 1), np.int64)
    wide[0, ::3] = 200
    files["oversize_20000.png"] = pack_png(wide, 8, 0)
    b = io.BytesIO()
    Image.fromarray(np.tile(wide[:, :, 0].astype(np.uint8), (8, 1)), "L").save(b, "JPEG", quality=50)
    files["oversize_20000.jpg"] = b.getvalue()
    return files


def run_reference(files):
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "driver.cpp"), "w") as f:
            f.write(DRIVER)
        results = []
        for tag, flags in (("simd", []), ("scalar", ["-DSTBI_NO_SIMD"])):
            exe = os.path.join(tmp, "driver_" + tag)
            subprocess.check_call(["g++", "-O1", "-w", "-I" + REF_EXT] + flags + [os.path.join(tmp, "driver.cpp"), "-o", exe])
            d = os.path.join(tmp, tag)
            os.makedirs(d)
            for name, data in files.items():
                with open(os.path.join(d, name), "wb") as f:
                    f.write(data)
            out = subprocess.run([exe] + [os.path.join(d, n) for n in files], capture_output=True, text=True, check=True).stdout
            res = {}
            for line in out.splitlines():
                path, verdict, rest = line.split("\t")
                name = os.path.basename(path)
                if verdict == "OK":
                    w, h, n = (int(v) for v in rest.split())
                    res[name] = ((w, h, n), np.fromfile(path + ".rgba", np.uint8).reshape(h, w, 4))
                else:
                    res[name] = rest
            results.append(res)
    simd, scalar = results
    for name in files:
        a, b = simd[name], scalar[name]
        assert type(a) is type(b), name
        if isinstance(a, str):
            assert a == b, name
        else:
            assert a[0] == b[0] and np.array_equal(a[1], b[1]), "SIMD and scalar builds of the reference differ on " + name
    return simd


def main():
    pngs, jpegs = make_pngs(), make_jpegs()
    valid = dict(pngs); valid.update(jpegs)
    refusals = make_refusals(pngs, jpegs)
    everything = dict(valid); everything.update(refusals)
    ref = run_reference(everything)
    expected = {}
    for name in valid:
        assert not isinstance(ref[name], str), "the reference refuses %s: %s" % (name, ref[name])
        expected[name + ".whn"] = np.array(ref[name][0], np.int32)
        expected[name + ".rgba"] = ref[name][1]
    for name in refusals:
        if name.startswith("oversize"):
            assert not isinstance(ref[name], str), name
            expected[name + ".oversize"] = np.array(ref[name][0], np.int32)
        else:
            assert isinstance(ref[name], str), "the reference decodes " + name
            expected[name + ".refused"] = np.array(ref[name])
    np.savez_compressed(os.path.join(HERE, "image_inputs.npz"), **{k: np.frombuffer(v, np.uint8) for k, v in everything.items()})
    np.savez_compressed(os.path.join(HERE, "image_expected.npz"), **expected)
    print("%d valid (%d PNG, %d JPEG), %d refusal-group files; inputs %d bytes, expected %d bytes raw" % (
        len(valid), len(pngs), len(jpegs), len(refusals), sum(len(v) for v in everything.values()), sum(v.nbytes for v in expected.values())))
    for name in refusals:
        print("  %-26s %s" % (name, ref[name] if isinstance(ref[name], str) else "decoded %s" % (ref[name][0],)))


if __name__ == "__main__":
    sys.exit(main())
