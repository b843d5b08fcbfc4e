"""Helpers of the PNG / JPEG tests: the committed fixtures (tests/golden/images, written by make_image_golden.py with the reference's
own decoder), a TGA writer, an independent PNG reader (zlib + numpy) and the seeded prefix / mutation schedule that the in-library
test and the sanitizer driver (tests/native/image_fuzz.cpp) both replay."""
import os
import struct
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "images")
MAX_DIM = 16384
FUZZ_SEEDS = ["rgba16.png", "base420.jpg", "prog420.jpg"]        # one PNG, one baseline and one progressive JPEG
FUZZ_MUTATIONS = 2000

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


def mutations(data, index):
    """FUZZ_MUTATIONS single-byte mutations of `data`, seeded by the position of the file in FUZZ_SEEDS"""
    rng = XorShift(0x9E3779B97F4A7C15 + index)
    for _ in range(FUZZ_MUTATIONS):
        pos = (rng.next() >> 16) % len(data)
        val = (rng.next() >> 24) & 255
        if val == data[pos]:
            val ^= 0xFF
        yield data[:pos] + bytes([val]) + data[pos + 1:]
