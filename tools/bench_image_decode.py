"""Host decode rate of the PNG / JPEG readers (gfxexp_amd/csrc/host/image_codecs.cpp): megapixels per second, one thread, best of
five, on a 2048 x 2048 colour PNG, a baseline 4:2:0 JPEG of the same picture and its progressive twin (written here with Pillow) --
next to the reference's decoder (its ext/ header, built -O2 in a temporary directory) where the reference tree is present, and the
load time of the textured test scene (the bunny with four PNG / JPEG maps of tests/golden/images).  Set-up-time work: nothing here
touches a GPU.  Prints one JSON line.

    python tools/bench_image_decode.py [--size 2048] [--reference-ext DIR]
"""
import argparse
import ctypes as C
import io
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gfxexp_amd import api  # noqa: E402


def reference_driver():
    """the timing driver is the golden generator's (tests/golden/images/make_image_golden.py): one text, built here with -O2"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_image_golden", os.path.join(ROOT, "tests", "golden", "images", "make_image_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.DRIVER


def picture(n):
    rng = np.random.default_rng(5)
    y, x = np.mgrid[0:n, 0:n].astype(np.float32) / n
    img = np.stack([x, 0.5 + 0.5 * np.sin(40 * y + 9 * x), np.sqrt(x * y)], -1)
    img += rng.normal(0, 0.03, img.shape).astype(np.float32)            # photographic-ish: ramps, texture, some noise
    return (np.clip(img, 0, 1) * 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--reference-ext", default=os.environ.get("GFX_REFERENCE_EXT", "/root/reference/ext"))
    a = ap.parse_args()
    from PIL import Image
    im = Image.fromarray(picture(a.size), "RGB")
    files = {}
    for name, kw in (("png", dict(format="PNG")), ("jpeg_baseline_420", dict(format="JPEG", quality=90, subsampling=2)),
                     ("jpeg_progressive_420", dict(format="JPEG", quality=90, subsampling=2, progressive=True))):
        b = io.BytesIO()
        im.save(b, **kw)
        files[name] = b.getvalue()
    L = api.lib()
    out = np.zeros((a.size, a.size, 4), np.uint8)
    mp = a.size * a.size / 1e6
    res = {"size": a.size, "threads": 1}
    for name, data in files.items():
        best = 1e30
        for _ in range(5):
            t0 = time.perf_counter()
            rc = L.gfxh_image_decode_rgba8(data, C.c_size_t(len(data)), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes))
            best = min(best, time.perf_counter() - t0)
            assert rc == 0, L.gfxh_last_error()
        res[name] = {"file_bytes": len(data), "mpix_per_s": round(mp / best, 1)}
    if os.path.exists(os.path.join(a.reference_ext, "stb_image.h")):
        with tempfile.TemporaryDirectory() as tmp:
            with open(os.path.join(tmp, "driver.cpp"), "w") as f:
                f.write(reference_driver())
            exe = os.path.join(tmp, "driver")
            subprocess.check_call(["g++", "-O2", "-w", "-I" + a.reference_ext, os.path.join(tmp, "driver.cpp"), "-o", exe])
            paths = []
            for name, data in files.items():
                paths.append(os.path.join(tmp, name))
                with open(paths[-1], "wb") as f:
                    f.write(data)
            lines = subprocess.run([exe, "--time"] + paths, capture_output=True, text=True, check=True).stdout.splitlines()
            times = [float(line.split("\t")[2]) for line in lines]
            assert len(times) == len(paths) and all(line.split("\t")[1] == "TIME" for line in lines), lines
        for name, t in zip(files, times):
            res[name]["reference_mpix_per_s"] = round(mp / t, 1)
            res[name]["reference_over_this"] = round(res[name]["reference_mpix_per_s"] / res[name]["mpix_per_s"], 2)
    # the textured test scene: OBJ + MTL with four maps, read and decoded on the host
    from tests import image_fixtures as F
    with tempfile.TemporaryDirectory() as tmp:
        bunny = os.path.join(ROOT, "tests", "golden", "assets", "stanford_bunny_309_faces")
        with open(bunny + ".obj") as f, open(os.path.join(tmp, "stanford_bunny_309_faces.obj"), "w") as g:
            g.write(f.read())
        with open(bunny + ".mtl") as f, open(os.path.join(tmp, "stanford_bunny_309_faces.mtl"), "w") as g:
            g.write(f.read() + "map_Kd rgba8.png\nmap_Ks base420.jpg\nmap_bump adam7_rgb8.png\nmap_Ke prog444.jpg\n")
        for name in ("rgba8.png", "base420.jpg", "adam7_rgb8.png", "prog444.jpg"):
            F.write_file(tmp, name)
        best = 1e30
        for _ in range(5):
            s = api.HostScene()
            t0 = time.perf_counter()
            s.load_obj(os.path.join(tmp, "stanford_bunny_309_faces.obj"))
            best = min(best, time.perf_counter() - t0)
            assert len(s.textures()) == 4
        res["textured_bunny_load_ms"] = round(best * 1e3, 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
