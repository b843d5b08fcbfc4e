"""Shared by the displaced-rendering tests (CPU and GPU): the host compilation of gfxexp_amd/csrc/tfdm/displaced_surface.hip.h
(tests/displaced_host.cpp, compiled into a directory the caller provides)."""
import ctypes as C
import os
import subprocess

import numpy as np

from gfxexp_amd import api
from tests import tfdm_host as T

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "displaced_host.cpp")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class DisplacedHost:
    """displaced_surface.hip.h on the host, behind ctypes."""

    def __init__(self, out_dir):
        so = os.path.join(str(out_dir), "libdisplaced_host.so")
        subprocess.check_call(["g++"] + T.FLAGS + [SRC, "-o", so])
        self.L = L = C.CDLL(so)
        L.displaced_host_sizeof.restype = C.c_uint32
        assert L.displaced_host_sizeof(0) == api.TFDM_INSTANCE_DTYPE.itemsize and L.displaced_host_sizeof(1) == api.SCENE_HIT_DTYPE.itemsize
        assert L.displaced_host_sizeof(2) == C.sizeof(api.GfxCamera)

    def resolve(self, table, hits, org, dirs, base_verts, geom_slot, mat_slot, xy, prev_camera, width, height, reset_flow=False):
        """One displaced hit per entry -> dict(points (n, 11): position, normal, tangent, u, v; g0, g2, g3 (n, 4) uint32; g1 (n, 2))."""
        n = len(hits)
        table = np.ascontiguousarray(table, api.TFDM_INSTANCE_DTYPE)
        hits = np.ascontiguousarray(hits, api.SCENE_HIT_DTYPE)
        org, dirs = np.ascontiguousarray(org, np.float32).reshape(n, 4), np.ascontiguousarray(dirs, np.float32).reshape(n, 4)
        bv = np.ascontiguousarray(base_verts, np.float32).reshape(n, 15)
        gs, ms = np.ascontiguousarray(geom_slot, np.uint32).reshape(n), np.ascontiguousarray(mat_slot, np.uint32).reshape(n)
        xy = np.ascontiguousarray(xy, np.int32).reshape(n, 2)
        out = dict(points=np.zeros((n, 11), np.float32), g0=np.zeros((n, 4), np.uint32), g1=np.zeros((n, 2), np.float32),
                   g2=np.zeros((n, 4), np.uint32), g3=np.zeros((n, 4), np.uint32))
        self.L.displaced_host_resolve(_p(table), _p(hits), _p(org), _p(dirs), _p(bv), _p(gs), _p(ms), _p(xy), C.c_uint32(n), C.byref(prev_camera),
                                      C.c_float(width), C.c_float(height), C.c_int(int(reset_flow)), _p(out["points"]), _p(out["g0"]), _p(out["g1"]),
                                      _p(out["g2"]), _p(out["g3"]))
        return out

    def decode_dir(self, q):
        q = np.ascontiguousarray(q, np.uint32).reshape(-1)
        out = np.zeros((len(q), 3), np.float32)
        self.L.displaced_host_decode_dir(_p(q), C.c_uint32(len(q)), _p(out))
        return out


def base_verts_of(vertices, triangles, prim):
    """(n, 15): texCoord0Dir, u, v of the vertices A, B, C of base triangles `prim` (VERTEX_DTYPE vertices, (m, 3) triangles)."""
    tri = np.asarray(triangles).reshape(-1, 3)[np.asarray(prim)]
    out = np.zeros((len(tri), 3, 5), np.float32)
    for k in range(3):
        out[:, k, :3] = vertices["texCoord0Dir"][tri[:, k]]
        out[:, k, 3:] = vertices["texCoord"][tri[:, k]]
    return out.reshape(len(tri), 15)
