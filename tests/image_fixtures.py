"""Helpers of the image reader tests: the committed PNG / JPEG fixtures (tests/golden/images, written by make_image_golden.py with the
reference's own decoder), a TGA writer, an independent PNG reader (zlib + numpy), small valid files of every other format the host
layer reads (reader_seeds; tools/fuzz_loaders.py starts from the same ones), and the seeded prefix / mutation schedule that the
in-library tests and the sanitizer driver (tests/native/image_fuzz.cpp) both replay."""
import os
import struct
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "images")
MAX_DIM = 16384
FUZZ_SEEDS = ["rgba16.png", "base420.jpg", "prog420.jpg"]        # one PNG, one baseline and one progressive JPEG
FUZZ_MUTATIONS = 2000
READER_MUTATIONS = 500                                           # per reader_seeds() file of 0.3 - 2 KB, after every prefix: a test size, not a measurement

_cache = {}


def inputs():
    if "in" not in _cache:
        with np.load(os.path.join(GOLDEN, "image_inputs.npz")) as z:
            _cache["in"] = {k: z[k].tobytes() for k in z.files}
    return _cache["in"]


def expected():
    if "exp" not in _cache:
        with np.load(os.path.join(GOLDEN, "image_expected.npz")) as z:
            _cache["exp"] = {k: z[k] for k in z.files}
    return _cache["exp"]


def valid_names():
    return sorted(k[:-5] for k in expected() if k.endswith(".rgba"))


def refused_names():
    return sorted(k[:-8] for k in expected() if k.endswith(".refused"))


def oversize_names():
    return sorted(k[:-9] for k in expected() if k.endswith(".oversize"))


def golden(name):
    """(uint8 [h, w, 4], n) as the reference's stbi_load(name, &w, &h, &n, 4) returned them"""
    e = expected()
    w, h, n = (int(v) for v in e[name + ".whn"])
    rgba = e[name + ".rgba"]
    assert rgba.shape == (h, w, 4)
    return rgba, n


def write_file(directory, name, data=None):
    path = os.path.join(str(directory), name)
    with open(path, "wb") as f:
        f.write(inputs()[name] if data is None else data)
    return path


def write_tga(path, rgba):
    """uncompressed 32-bit true-colour TGA, top row first"""
    rgba = np.ascontiguousarray(rgba, np.uint8)
    h, w = rgba.shape[:2]
    with open(path, "wb") as f:
        f.write(struct.pack("<BBBHHBHHHHBB", 0, 0, 2, 0, 0, 0, 0, 0, w, h, 32, 0x28))
        f.write(np.ascontiguousarray(rgba[..., [2, 1, 0, 3]]).tobytes())


def read_png_rgba8(data):
    """An 8-bit RGBA, non-interlaced PNG whose lines all use filter 0, read with zlib and numpy alone; CRCs checked."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, idat, ihdr, kinds = 8, b"", None, []
    while at < len(data):
        n, = struct.unpack(">I", data[at:at + 4])
        kind, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        crc, = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        assert zlib.crc32(kind + body) & 0xFFFFFFFF == crc, kind
        kinds.append(kind)
        if kind == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        if kind == b"IDAT":
            idat += body
        at += 12 + n
    assert kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and at == len(data)
    w, h, depth, colour, comp, flt, lace = ihdr
    assert (depth, colour, comp, flt, lace) == (8, 6, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 4 * w + 1)       # zlib checks the Adler-32
    assert not raw[:, 0].any()
    return raw[:, 1:].reshape(h, w, 4)


def _dds(fourcc, dxgi, w, h, payload, mips=1):
    hdr = bytearray(128)
    hdr[:4] = b"DDS "
    struct.pack_into("<II", hdr, 4, 124, 0x1007 | (0x20000 if mips > 1 else 0))
    struct.pack_into("<II", hdr, 12, h, w)
    struct.pack_into("<I", hdr, 28, mips)
    struct.pack_into("<II4s", hdr, 76, 32, 0x4, fourcc)
    return bytes(hdr) + (struct.pack("<IIIII", dxgi, 3, 0, 1, 0) if fourcc == b"DX10" else b"") + payload


def reader_seeds():
    """{file name: bytes} of small valid files for the readers of host/image_formats.cpp: EXR in four compressions with HALF / FLOAT /
    UINT channels (the writer of tests/test_exr_reader.py), PFM in both byte orders, PPM, PGM, two BMP, two TGA and four DDS."""
    if "seeds" in _cache:
        return _cache["seeds"]
    from tests import test_exr_reader as X
    rng = np.random.default_rng(3)
    seeds = {}
    h, w = 9, 13
    img = rng.random((h, w)).astype(np.float32)
    for comp in (X.NONE, X.RLE, X.ZIPS, X.ZIP):
        seeds["e%d.exr" % comp] = X._exr({"R": (X.HALF, img), "G": (X.FLOAT, img * 2), "B": (X.UINT, (img * 100).astype(np.uint32)), "A": (X.HALF, img)}, comp)
    seeds["a.pfm"] = b"PF\n%d %d\n-1.0\n" % (w, h) + rng.random((h, w, 3)).astype("<f4").tobytes()
    seeds["b.pfm"] = b"Pf\n%d %d\n1.0\n" % (w, h) + rng.random((h, w)).astype(">f4").tobytes()
    seeds["a.ppm"] = b"P6\n# c\n%d %d\n255\n" % (w, h) + rng.integers(0, 255, (h, w, 3), dtype=np.uint8).tobytes()
    seeds["a.pgm"] = b"P5\n%d %d\n255\n" % (w, h) + rng.integers(0, 255, (h, w), dtype=np.uint8).tobytes()
    stride = (w * 3 + 3) & ~3
    seeds["a.bmp"] = b"BM" + struct.pack("<IHHI", 54 + stride * h, 0, 0, 54) + struct.pack("<IiiHHIIiiII", 40, w, h, 1, 24, 0, stride * h, 0, 0, 0, 0) + bytes(stride * h)
    seeds["b.bmp"] = b"BM" + struct.pack("<IHHI", 54 + 4 * w * h, 0, 0, 54) + struct.pack("<IiiHHIIiiII", 40, w, -h, 1, 32, 3, 4 * w * h, 0, 0, 0, 0) + bytes(4 * w * h)
    seeds["a.tga"] = bytes([0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0]) + struct.pack("<HH", w, h) + bytes([24, 0x20]) + bytes(3 * w * h)
    seeds["b.tga"] = bytes([3, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0]) + struct.pack("<HH", w, h) + bytes([8, 0]) + b"abc" + bytes(w * h)
    seeds["a.dds"] = _dds(b"DX10", 99, w, h, rng.integers(0, 256, 16 * 4 * 3, dtype=np.uint8).tobytes())                    # BC7 sRGB, partial blocks
    seeds["b.dds"] = _dds(b"DXT1", 0, 8, 8, rng.integers(0, 256, 8 * (4 + 1 + 1 + 1), dtype=np.uint8).tobytes(), mips=4)    # legacy FourCC with a mip chain
    seeds["c.dds"] = _dds(b"DX10", 87, w, h, rng.integers(0, 256, 4 * w * h, dtype=np.uint8).tobytes())                     # uncompressed BGRA8
    seeds["d.dds"] = _dds(b"ATI2", 0, w, h, rng.integers(0, 256, 16 * 4 * 3, dtype=np.uint8).tobytes())                     # BC5
    _cache["seeds"] = seeds
    return seeds


# ---- the mutation schedule: xorshift64* (Marsaglia / Vigna), the same few lines in tests/native/image_fuzz.cpp
class XorShift:
    def __init__(self, seed):
        self.s = seed & 0xFFFFFFFFFFFFFFFF or 1

    def next(self):
        s = self.s
        s ^= s >> 12
        s ^= (s << 25) & 0xFFFFFFFFFFFFFFFF
        s ^= s >> 27
        self.s = s
        return (s * 0x2545F4914F6CDD1D) & 0xFFFFFFFFFFFFFFFF


def mutations(data, index, count=FUZZ_MUTATIONS):
    """`count` single-byte mutations of `data`, seeded by the position of the file in its seed list"""
    rng = XorShift(0x9E3779B97F4A7C15 + index)
    for _ in range(count):
        pos = (rng.next() >> 16) % len(data)
        val = (rng.next() >> 24) & 255
        if val == data[pos]:
            val ^= 0xFF
        yield data[:pos] + bytes([val]) + data[pos + 1:]
