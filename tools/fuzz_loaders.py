"""Mutation fuzzing of the host loaders (gfxexp_amd/csrc/host/scene_builder.cpp: EXR / PFM / PNM / BMP / TGA decoders, the DDS parser, OBJ + MTL parser;
image_codecs.cpp: the PNG and JPEG readers, seeded with fixtures of tests/golden/images) against
the ASan + UBSan build of the library's host code (tools/asan_cpu_suite.sh builds it and runs this).  Valid files are written here (the EXR
writer of tests/test_exr_reader.py), then truncated, byte-flipped, given extreme 32-bit fields or spliced; a loader may refuse a file
(GfxError) or load it -- a sanitizer report is the failure.  usage: fuzz_loaders.py [mutations per seed file, default 400]"""
import os, sys, struct, random, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gfxexp_amd import api
from tests import test_exr_reader as X
from tests import image_fixtures as IMG
rng = random.Random(7)
nrng = np.random.default_rng(3)
tmp = tempfile.mkdtemp()
seeds = {}
h, w = 9, 13
img = nrng.random((h, w)).astype(np.float32)
for comp in (X.NONE, X.RLE, X.ZIPS, X.ZIP):
    seeds['e%d.exr' % comp] = X._exr({"R": (X.HALF, img), "G": (X.FLOAT, img * 2), "B": (X.UINT, (img * 100).astype(np.uint32)), "A": (X.HALF, img)}, comp)
seeds['big.exr'] = X._exr({"Y": (X.HALF, nrng.random((40, 300)).astype(np.float32))}, X.ZIP)
seeds['a.pfm'] = b"PF\n%d %d\n-1.0\n" % (w, h) + nrng.random((h, w, 3)).astype('<f4').tobytes()
seeds['b.pfm'] = b"Pf\n%d %d\n1.0\n" % (w, h) + nrng.random((h, w)).astype('>f4').tobytes()
seeds['a.ppm'] = b"P6\n# c\n%d %d\n255\n" % (w, h) + nrng.integers(0, 255, (h, w, 3), dtype=np.uint8).tobytes()
seeds['a.pgm'] = b"P5\n%d %d\n255\n" % (w, h) + nrng.integers(0, 255, (h, w), dtype=np.uint8).tobytes()
stride = (w * 3 + 3) & ~3
seeds['a.bmp'] = b"BM" + struct.pack("<IHHI", 54 + stride * h, 0, 0, 54) + struct.pack("<IiiHHIIiiII", 40, w, h, 1, 24, 0, stride * h, 0, 0, 0, 0) + bytes(stride * h)
seeds['b.bmp'] = b"BM" + struct.pack("<IHHI", 54 + 4 * w * h, 0, 0, 54) + struct.pack("<IiiHHIIiiII", 40, w, -h, 1, 32, 3, 4 * w * h, 0, 0, 0, 0) + bytes(4 * w * h)
seeds['a.tga'] = bytes([0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0]) + struct.pack("<HH", w, h) + bytes([24, 0x20]) + bytes(3 * w * h)
seeds['b.tga'] = bytes([3, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0]) + struct.pack("<HH", w, h) + bytes([8, 0]) + b"abc" + bytes(w * h)
def _dds(fourcc, dxgi, dw, dh, payload, mips=1):
    hdr = bytearray(128)
    hdr[:4] = b"DDS "
    struct.pack_into("<II", hdr, 4, 124, 0x1007 | (0x20000 if mips > 1 else 0))
    struct.pack_into("<II", hdr, 12, dh, dw)
    struct.pack_into("<I", hdr, 28, mips)
    struct.pack_into("<II4s", hdr, 76, 32, 0x4, fourcc)
    return bytes(hdr) + (struct.pack("<IIIII", dxgi, 3, 0, 1, 0) if fourcc == b"DX10" else b"") + payload
seeds['a.dds'] = _dds(b"DX10", 99, w, h, nrng.integers(0, 256, 16 * 4 * 3, dtype=np.uint8).tobytes())                    # BC7 sRGB, partial blocks
seeds['b.dds'] = _dds(b"DXT1", 0, 8, 8, nrng.integers(0, 256, 8 * (4 + 1 + 1 + 1), dtype=np.uint8).tobytes(), mips=4)    # legacy FourCC with a mip chain
seeds['c.dds'] = _dds(b"DX10", 87, w, h, nrng.integers(0, 256, 4 * w * h, dtype=np.uint8).tobytes())                     # uncompressed BGRA8
seeds['d.dds'] = _dds(b"ATI2", 0, w, h, nrng.integers(0, 256, 16 * 4 * 3, dtype=np.uint8).tobytes())                     # BC5
for name in ("rgba16.png", "adam7_pal4_trns.png", "g2.png", "rgb8_stored.png", "base420.jpg", "prog420.jpg", "restart3.jpg", "cmyk_adobe.jpg", "own_h4v1.jpg"):
    seeds[name] = IMG.inputs()[name]                                                                                     # PNG / JPEG: palette, Adam7, 16 bit; restarts, progressive, CMYK
obj = b"""mtllib m.mtl
v 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0.5
vt 0 0\nvt 1 0\nvt 0 1\nvt 1 1
vn 0 0 1\nvn 0 1 0
usemtl a
f 1/1/1 2/2/1 3/3/1
f -1/-1/-1 2//2 3/3
usemtl c
f 1/1 2/2 3/3
usemtl b
f 1 2 3 4
g grp
s off
f 2/2 4/4 3/3
"""
mtl = b"""newmtl a\nKd 0.5 0.5 0.5\nKs 0.1 0.1 0.1\nNs 50\nKe 1 1 1\nmap_Kd a.ppm\nmap_Bump -bm 0.5 a.tga\nnewmtl b\nKd 1 0 0\nmap_Ke a.pfm\nmap_Ks b.bmp\nnewmtl c\nKd 1 1 1\nmap_Kd a.dds\nmap_Ks b.dds\nmap_Ke c.dds\nmap_bump d.dds\n"""
for n, d in seeds.items():
    open(os.path.join(tmp, n), 'wb').write(d)
open(os.path.join(tmp, 'm.mtl'), 'wb').write(mtl)
open(os.path.join(tmp, 's.obj'), 'wb').write(obj)

def mutate(d):
    d = bytearray(d)
    k = rng.random()
    if k < 0.25 and len(d) > 4:
        d = d[:rng.randrange(1, len(d))]
    elif k < 0.7:
        for _ in range(rng.randrange(1, 6)):
            d[rng.randrange(len(d))] = rng.randrange(256)
    elif k < 0.85:
        i = rng.randrange(len(d)); d[i:i + 4] = struct.pack("<I", rng.choice([0, 1, 0xFFFFFFFF, 0x7FFFFFFF, 0x80000000, 65536, 16385, len(d)]))[:max(0, min(4, len(d) - i))]
    else:
        i = rng.randrange(len(d)); j = rng.randrange(len(d)); d[i:i] = d[j:j + rng.randrange(1, 64)]
    return bytes(d)

ok = bad = 0
N = int(sys.argv[1]) if len(sys.argv) > 1 else 400
for n, d in seeds.items():
    s = api.HostScene()
    assert s.load_texture(os.path.join(tmp, n)) != 0, n          # the seed itself loads
    for it in range(N):
        p = os.path.join(tmp, 'mut_' + n)
        open(p, 'wb').write(mutate(d))
        s = api.HostScene()
        try:
            s.load_texture(p); ok += 1
        except api.GfxError:
            bad += 1
        if n.endswith(('.png', '.jpg')):                             # the memory entry points, on an exactly sized heap buffer
            try:
                api.image_decode_rgba8(open(p, 'rb').read())
            except api.GfxError:
                pass
        if n.endswith('.dds'):                                       # the parser on its own, on an exactly sized heap buffer
            try:
                api.dds_parse(open(p, 'rb').read())
            except api.GfxError:
                pass
print('images: loaded', ok, 'refused', bad)
ok = bad = 0
s = api.HostScene(); s.load_obj(os.path.join(tmp, 's.obj'))
for it in range(N * 3):
    which = rng.random()
    open(os.path.join(tmp, 'mut.obj'), 'wb').write(mutate(obj) if which < 0.6 else obj.replace(b"m.mtl", b"mm.mtl"))
    open(os.path.join(tmp, 'mm.mtl'), 'wb').write(mutate(mtl))
    s = api.HostScene()
    try:
        s.load_obj(os.path.join(tmp, 'mut.obj')); ok += 1
    except api.GfxError:
        bad += 1
print('obj: loaded', ok, 'refused', bad)
