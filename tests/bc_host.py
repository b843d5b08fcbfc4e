"""Shared by the block-compression tests (CPU and GPU): the host build of gfxexp_amd/csrc/bc/bc_decode.hip.h (tests/bc_host.cpp,
compiled into a directory the caller provides, nothing built into the tree), synthesised .dds files, and the block sets the
checks are run on.  The yardstick for every decoded byte is tools/dds_convert.py."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dds_convert as D  # noqa: E402

SRC = os.path.join(HERE, "bc_host.cpp")
FLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-Wall", "-I" + os.path.join(ROOT, "gfxexp_amd", "csrc")]

# dds_convert's format name -> (enum gfx_bc_format, bytes per block, a legacy FourCC or None, DXGI format, its _SRGB variant or None)
FORMATS = {"BC1": (0, 8, b"DXT1", 71, 72), "BC2": (1, 16, b"DXT3", 74, 75), "BC3": (2, 16, b"DXT5", 77, 78), "BC4U": (3, 8, b"BC4U", 80, None),
           "BC4S": (4, 8, b"BC4S", 81, None), "BC5U": (5, 16, b"ATI2", 83, None), "BC5S": (6, 16, b"BC5S", 84, None), "BC7": (7, 16, None, 98, 99)}
SIZES = [(1, 1), (3, 5), (4, 4), (7, 9), (130, 66)]


def compile_host(out_dir):
    so = os.path.join(str(out_dir), "libbc_host.so")
    subprocess.check_call(["g++"] + FLAGS + [SRC, "-o", so])
    L = C.CDLL(so)
    L.bc_host_decode.restype = C.c_int
    L.bc_host_block_bytes.restype = C.c_uint32
    return L


def host_decode(L, name, blocks, w, h):
    blocks = np.ascontiguousarray(blocks, np.uint8)
    assert blocks.size == num_blocks(w, h) * FORMATS[name][1]
    out = np.zeros((h, w, 4), np.uint8)
    rc = L.bc_host_decode(C.c_uint32(FORMATS[name][0]), blocks.ctypes.data_as(C.c_void_p), C.c_uint32(w), C.c_uint32(h), out.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return out


def num_blocks(w, h):
    return ((w + 3) // 4) * ((h + 3) // 4)


def make_dds(name, w, h, payload, srgb=False, legacy=None, mips=1, dxgi=None, misc=0, array_size=1, dimension=3, caps2=0, depth=0):
    """A .dds file around `payload`.  legacy=None: the FourCC header where the format has one and sRGB is not asked for."""
    _, _, fourcc, code, code_srgb = FORMATS.get(name, (0, 0, None, 0, None))
    if dxgi is None:
        dxgi = code_srgb if srgb else code
    if legacy is None:
        legacy = fourcc is not None and not srgb
    hdr = bytearray(128)
    hdr[:4] = b"DDS "
    struct.pack_into("<II", hdr, 4, 124, 0x1007 | (0x20000 if mips > 1 else 0) | (0x800000 if depth else 0))
    struct.pack_into("<II", hdr, 12, h, w)
    struct.pack_into("<I", hdr, 24, depth)
    struct.pack_into("<I", hdr, 28, mips)
    struct.pack_into("<II4s", hdr, 76, 32, 0x4, fourcc if legacy else b"DX10")
    struct.pack_into("<II", hdr, 108, 0x1000, caps2)
    out = bytes(hdr)
    if not legacy:
        out += struct.pack("<IIIII", dxgi, dimension, misc, array_size, 0)
    return out + bytes(payload)


def reference_decode(name, blocks, w, h):
    """[h, w, 4] RGBA8 as tools/dds_convert.py decodes the blocks."""
    img, fmt = D.decode(make_dds(name, w, h, np.ascontiguousarray(blocks, np.uint8).tobytes()))
    assert fmt == name and img.shape == (h, w, 4)
    return np.ascontiguousarray(img)


def narrow(img, channels):
    """The host loader's rule for 8-bit images: R8 / RG8 keep the first one / two channels of the RGBA8 texel."""
    return np.ascontiguousarray(img[:, :, :channels])


def random_blocks(rng, name, w, h):
    return rng.integers(0, 256, (num_blocks(w, h), FORMATS[name][1]), dtype=np.uint8)


def exhaustive_alpha_blocks():
    """65 536 eight-byte blocks: every pair of endpoint bytes, and in each block every 3-bit index (texel t carries index t & 7).
    One 1024 x 1024 texture of BC4."""
    pair = np.arange(65536, dtype=np.uint32)
    b = np.zeros((65536, 8), np.uint8)
    b[:, 0], b[:, 1] = pair & 255, pair >> 8
    bits = sum((t & 7) << (3 * t) for t in range(16))
    b[:, 2:] = np.frombuffer(bits.to_bytes(6, "little"), np.uint8)
    return b


def exhaustive_blocks(rng, name):
    """The 1024 x 1024 texture of `name` whose alpha-type halves are exhaustive_alpha_blocks (BC5: the second half walks the pairs in
    reverse; BC3: the colour half is random)."""
    a = exhaustive_alpha_blocks()
    if name in ("BC4U", "BC4S"):
        return a
    if name in ("BC5U", "BC5S"):
        return np.concatenate([a, a[::-1]], 1)
    assert name == "BC3"
    return np.concatenate([a, rng.integers(0, 256, (65536, 8), dtype=np.uint8)], 1)


def bc1_edge_blocks(rng, n=512):
    """Random BC1 blocks, then blocks forced to colour0 <= colour1, to colour0 == colour1, and blocks whose sixteen indices are all 3."""
    b = rng.integers(0, 256, (4 * n, 8), dtype=np.uint8)
    c = b.view(np.uint16).reshape(-1, 4)
    lo, hi = np.minimum(c[n:2 * n, 0], c[n:2 * n, 1]), np.maximum(c[n:2 * n, 0], c[n:2 * n, 1])
    c[n:2 * n, 0], c[n:2 * n, 1] = lo, hi
    c[2 * n:3 * n, 1] = c[2 * n:3 * n, 0]
    b[3 * n:, 4:] = 255
    c[3 * n + n // 2:, 0], c[3 * n + n // 2:, 1] = lo[:n - n // 2], hi[:n - n // 2]       # all-index-3 in the 3-colour palette too
    return b


# BC7 header fields per mode: (partition bits, rotation bits, index-selection bits), from the format specification
_BC7_FIELDS = [(4, 0, 0), (6, 0, 0), (6, 0, 0), (6, 0, 0), (0, 2, 1), (0, 2, 0), (0, 0, 0), (6, 0, 0)]


def bc7_constructed_blocks(rng, per_combination=2):
    """BC7 blocks with the mode bit and the partition, rotation and index-selection fields set and every other bit random: every
    value of those fields in every mode, the same number of blocks per mode, plus reserved-mode blocks (low byte zero)."""
    per_mode = 256 * per_combination
    out = []
    for mode, (pb, rb, isb) in enumerate(_BC7_FIELDS):
        combos = 1 << (pb + rb + isb)
        for k in range(per_mode):
            v = int.from_bytes(rng.bytes(16), "little")
            head = mode + 1 + pb + rb + isb
            v = (v >> head << head) | (1 << mode) | ((k % combos) << (mode + 1))
            out.append(v.to_bytes(16, "little"))
    for _ in range(32):
        v = int.from_bytes(rng.bytes(16), "little")
        out.append((v >> 8 << 8).to_bytes(16, "little"))
    return np.frombuffer(b"".join(out), np.uint8).reshape(-1, 16).copy()


def bc7_census(blocks):
    """What a set of BC7 blocks covers, read from the blocks alone: {mode: count}, {mode: set of partition ids}, the set of
    (rotation, index selection) of mode 4, the set of rotations of mode 5."""
    modes, parts, rot4, rot5 = {}, {}, set(), set()
    for b in blocks:
        v = int.from_bytes(bytes(b), "little")
        mode = next((m for m in range(8) if (v >> m) & 1), 8)
        modes[mode] = modes.get(mode, 0) + 1
        if mode == 8:
            continue
        pb, rb, isb = _BC7_FIELDS[mode]
        at = mode + 1
        parts.setdefault(mode, set()).add((v >> at) & ((1 << pb) - 1))
        rot = (v >> (at + pb)) & ((1 << rb) - 1)
        if mode == 4:
            rot4.add((rot, (v >> (at + pb + rb)) & 1))
        if mode == 5:
            rot5.add(rot)
    return modes, parts, rot4, rot5


def assert_bc7_coverage(blocks):
    """The condition the BC7 case sets on its own inputs (not on the decoder)."""
    modes, parts, rot4, rot5 = bc7_census(blocks)
    assert len(blocks) <= 20000
    for m in range(8):
        assert modes.get(m, 0) >= 256, (m, modes)
    assert modes.get(8, 0) >= 16, modes
    assert parts[0] == set(range(16))
    for m in (1, 2, 3, 7):
        assert parts[m] == set(range(64)), m
    assert rot4 == {(r, i) for r in range(4) for i in range(2)}
    assert rot5 == set(range(4))


def bc7_texture(rng):
    """(blocks, width, height): the constructed set padded with random blocks to whole rows of 64 blocks."""
    b = bc7_constructed_blocks(rng)
    rows = (len(b) + 63) // 64
    pad = rng.integers(0, 256, (rows * 64 - len(b), 16), dtype=np.uint8)
    return np.concatenate([b, pad], 0), 256, rows * 4
