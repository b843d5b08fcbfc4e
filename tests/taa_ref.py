"""Loader of the CPU restatement of the temporal anti-aliasing pass (tests/taa_ref.cpp): compiled with the oracle's flags into a
directory the caller provides (a pytest tmp_path_factory directory), nothing built into the tree."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.denoise_ref import FLAGS

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "taa_ref.cpp")


def compile_ref(out_dir):
    so = os.path.join(str(out_dir), "libtaa_ref.so")
    subprocess.check_call(["g++"] + FLAGS + [SRC, "-o", so])
    L = C.CDLL(so)
    L.taa_ref_run.restype = C.c_int
    return L


def empty_history(w, h):
    return np.zeros((w * h, 4), np.float32)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def run(L, w, h, n, color, flow, first, hist):
    """One gfx_taa_apply call with historyLength `n`: returns (output float4[W*H], the history it writes).  `color` and `hist` are
    float32 arrays with W*H*4 values, `flow` with W*H*2."""
    color = np.ascontiguousarray(np.asarray(color, np.float32).reshape(w * h, 4))
    flow = np.ascontiguousarray(np.asarray(flow, np.float32).reshape(w * h, 2))
    hist = np.ascontiguousarray(np.asarray(hist, np.float32).reshape(w * h, 4))
    out = np.zeros((w * h, 4), np.float32)
    new = np.zeros((w * h, 4), np.float32)
    rc = L.taa_ref_run(C.c_int(w), C.c_int(h), C.c_uint32(n), _ptr(color), _ptr(flow), C.c_int(1 if first else 0), _ptr(hist),
                       _ptr(out), _ptr(new))
    if rc:
        raise ValueError("taa_ref_run: bad arguments")
    return out, new
