"""Builds tests/native/image_fuzz: image_fuzz.cpp + gfxexp_amd/csrc/host/image_codecs.cpp and image_formats.cpp alone, with g++ -fsanitize=address,undefined,
as an executable (a sanitized executable brings its own runtime; nothing is preloaded and nothing of it goes near the GPU library).
build() returns the path, or raises Unavailable with the reason when there is no g++ or no sanitizer runtime to link against."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
EXE = os.path.join(HERE, "image_fuzz")
HOST = os.path.join(ROOT, "gfxexp_amd", "csrc", "host")
SOURCES = [os.path.join(HERE, "image_fuzz.cpp"), os.path.join(HOST, "image_codecs.cpp"), os.path.join(HOST, "image_formats.cpp")]
HEADERS = [os.path.join(HOST, "image_codecs.h"), os.path.join(HOST, "image_formats.h"), os.path.join(HOST, "..", "bc", "bc_decode.hip.h"),
           os.path.join(ROOT, "include", "gfxexp_host.h"), os.path.join(ROOT, "include", "gfxexp.h")]


class Unavailable(RuntimeError):
    pass


def build():
    cxx = shutil.which("g++")
    if not cxx:
        raise Unavailable("no g++ on this machine")
    if os.path.exists(EXE) and os.path.getmtime(EXE) >= max(os.path.getmtime(p) for p in SOURCES + HEADERS):
        return EXE
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall"] + SOURCES + ["-o", EXE]
    # the runtimes linked statically where the toolchain has them: the executable then starts whatever else the loader brings along
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        if "asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr:
            raise Unavailable("no sanitizer runtime to link against: " + r.stderr.strip().splitlines()[-1])
        raise RuntimeError("g++ failed for image_fuzz:\n" + r.stderr[-4000:])
    return EXE


if __name__ == "__main__":
    print(build())
