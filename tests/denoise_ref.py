"""Loader of the CPU restatement of the SVGF denoiser (tests/denoise_ref.cpp): compiled with the oracle's flags into a directory the
caller provides (a pytest tmp_path_factory directory), nothing built into the tree."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "denoise_ref.cpp")
# oracle/Makefile's flags (-ffp-contract=off is part of the math contract)
FLAGS = ["-std=c++17", "-O2", "-march=x86-64-v3", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-Wall", "-Wno-unused-function"]


def compile_ref(out_dir):
    so = os.path.join(str(out_dir), "libdenoise_ref.so")
    subprocess.check_call(["g++"] + FLAGS + [SRC, "-o", so])
    L = C.CDLL(so)
    L.dn_ref_run.restype = C.c_int
    return L


def empty_history(w, h):
    n = w * h
    return {"lighting": np.zeros((n, 4), np.float32), "moments": np.zeros((n, 2), np.float32),
            "length": np.zeros(n, np.uint32), "guide": np.zeros((n, 4), np.float32)}


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def run(L, w, h, settings, beauty, albedo, normal, flow, depth, first, hist, emissive=None):
    """One gfx_denoise call: returns (denoised float4[n], the history it writes).  `settings` is an api.GfxDenoiserSettings (or any
    object with its fields); images are float32 arrays with W*H rows, `emissive` an optional uint32 mask."""
    f32 = lambda a, k: np.ascontiguousarray(np.asarray(a, np.float32).reshape(w * h, k))
    beauty, albedo, normal, flow = f32(beauty, 4), f32(albedo, 4), f32(normal, 4), f32(flow, 2)
    depth = None if depth is None else np.ascontiguousarray(np.asarray(depth, np.float32).reshape(w * h))
    emissive = None if emissive is None else np.ascontiguousarray(np.asarray(emissive, np.uint32).reshape(w * h))
    new = empty_history(w, h)
    out = np.zeros((w * h, 4), np.float32)
    s = settings
    L.dn_ref_run(C.c_int(w), C.c_int(h), C.c_int(s.numStages), C.c_int(s.kernel), C.c_int(s.feedbackStage), C.c_float(s.sigmaZ),
                 C.c_float(s.sigmaN), C.c_float(s.sigmaL), C.c_float(s.minAlpha),
                 _ptr(beauty), _ptr(albedo), _ptr(normal), _ptr(flow), _ptr(depth), _ptr(emissive), C.c_int(1 if first else 0),
                 _ptr(hist["lighting"]), _ptr(hist["moments"]), _ptr(hist["length"]), _ptr(hist["guide"]),
                 _ptr(new["lighting"]), _ptr(new["moments"]), _ptr(new["length"]), _ptr(new["guide"]), _ptr(out))
    return out, new
