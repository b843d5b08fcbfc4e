"""Mutation fuzzing of the host loaders (gfxexp_amd/csrc/host/image_formats.cpp: EXR / PFM / PNM / BMP / TGA decoders, the DDS parser;
obj_loader.cpp: the OBJ + MTL parser; image_codecs.cpp: the PNG and JPEG readers, seeded with fixtures of tests/golden/images) against
the ASan + UBSan build of the library's host code (tools/asan_cpu_suite.sh builds it and runs this).  Valid files are written here (the EXR
writer of tests/test_exr_reader.py), then truncated, byte-flipped, given extreme 32-bit fields or spliced (the CPU suite itself runs the image readers alone under
the sanitizers, on single-byte mutations: tests/test_image_codecs_cpu.py); a loader may refuse a file
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
seeds = dict(IMG.reader_seeds())                                                                                        # EXR, PFM, PPM, PGM, BMP, TGA, DDS: shared with tests/test_image_codecs_cpu.py
seeds['big.exr'] = X._exr({"Y": (X.HALF, nrng.random((40, 300)).astype(np.float32))}, X.ZIP)
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
