"""Shared by the shell-mapping tests (CPU and GPU): the host compilation of gfxexp_amd/csrc/nrtdsm/shell_core.hip.h + shell_build.h
(tests/shell_host.cpp, compiled into a directory the caller provides) behind ctypes, and the inputs of the test cases.  The tree over
the per-triangle boxes is TFDM's and comes from tests/tfdm_host.py.  The float64 model is tests/shell_ref.py."""
import ctypes as C
import os
import subprocess

import numpy as np

from gfxexp_amd import api
from tests import nrtdsm_host as NH
from tests import tfdm_host as T

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "shell_host.cpp")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Refused(Exception):
    pass


class Host:
    def __init__(self, out_dir):
        self.T = T.Host(out_dir)
        so = os.path.join(str(out_dir), "libshell_host.so")
        subprocess.check_call(["g++"] + T.FLAGS + [SRC, "-o", so])
        self.L = L = C.CDLL(so)
        for n in ("shell_host_sizeof", "shell_host_max_descent", "shell_host_walk"):
            getattr(L, n).restype = C.c_uint32
        assert L.shell_host_sizeof(0) == api.NRTDSM_RECORD_DTYPE.itemsize and L.shell_host_sizeof(1) == api.TFDM_NODE_DTYPE.itemsize
        assert L.shell_host_sizeof(2) == C.sizeof(T.CoreParams) and L.shell_host_sizeof(3) == api.SHELL_HIT_DTYPE.itemsize
        assert L.shell_host_sizeof(4) == api.SHELL_TRI_DTYPE.itemsize
        self.max_descent = L.shell_host_max_descent()

    def refuse(self, gp):
        msg = C.create_string_buffer(256)
        return msg.value.decode() if self.L.shell_host_refuse(C.byref(gp), msg, C.c_uint32(256)) else None

    def build(self, geoms):
        """(nodes, triangles) of the shell BVH; raises Refused with the builder's message."""
        arr, keep = api._shell_geoms(geoms)
        nn, nt = C.c_uint32(), C.c_uint32()
        msg = C.create_string_buffer(256)
        if self.L.shell_host_build(arr, C.c_uint32(len(keep)), None, None, C.byref(nn), C.byref(nt), msg, C.c_uint32(256)):
            raise Refused(msg.value.decode())
        nodes, tris = np.zeros(nn.value, api.TFDM_NODE_DTYPE), np.zeros(nt.value, api.SHELL_TRI_DTYPE)
        assert self.L.shell_host_build(arr, C.c_uint32(len(keep)), _p(nodes), _p(tris), C.byref(nn), C.byref(nt), msg, C.c_uint32(256)) == 0
        return nodes, tris

    def state(self, vertices, triangles, geoms, gp):
        """Everything gfx_shell_create derives, on the host: dict params / records / aabbs / nodes / shell_nodes / shell_tris."""
        sn, stri = self.build(geoms)
        p = T.CoreParams()
        self.L.shell_host_params(C.byref(gp), C.byref(p))
        v = np.ascontiguousarray(vertices, api.VERTEX_DTYPE)
        t = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
        rec = np.zeros(len(t), api.NRTDSM_RECORD_DTYPE)
        boxes = np.zeros((len(t), 6), np.float32)
        if self.L.shell_host_records(_p(v), _p(t), C.c_uint32(len(t)), C.byref(gp), _p(sn), _p(stri), _p(rec), _p(boxes)):
            raise Refused("a texture coordinate reaches 2^22 tiles")
        return {"params": p, "records": rec, "aabbs": boxes, "nodes": self.T.tree(boxes), "shell_nodes": sn, "shell_tris": stri}

    def trace(self, st, mode, org, dirs, counters=False, iterations=False):
        org, dirs = np.ascontiguousarray(org, np.float32), np.ascontiguousarray(dirs, np.float32)
        n = len(org)
        out = np.zeros(n, np.uint32 if mode == api.TRACE_ANY else api.SHELL_HIT_DTYPE)
        cnt = np.zeros(4, np.uint64)
        it = np.zeros(n, np.uint32)
        self.L.shell_host_trace(_p(st["nodes"]), _p(st["records"]), _p(st["shell_nodes"]), _p(st["shell_tris"]), C.byref(st["params"]), C.c_int(mode), _p(org), _p(dirs),
                                C.c_uint32(n), _p(out), _p(cnt) if counters else None, _p(it) if iterations else None)
        res = (out,)
        if counters:
            res += (cnt,)
        if iterations:
            res += (it,)
        return res if len(res) > 1 else out

    def walk(self, st, prim, capacity=1 << 14):
        """Every box the traversal can enter on base triangle `prim`: ids (tileX, tileY, lod, node or -1) and (lo, hi) in (u, v, h)."""
        rec = np.ascontiguousarray(st["records"][prim:prim + 1])
        while True:
            ids = np.zeros((capacity, 4), np.int32)
            box = np.zeros((capacity, 6), np.float32)
            k = self.L.shell_host_walk(_p(rec), _p(st["shell_nodes"]), _p(ids), _p(box), C.c_uint32(capacity))
            if k <= capacity:
                return ids[:k], box[:k]
            capacity = k


# ---------------------------------------------------------------- inputs
N_RAYS = 3000
N_BAD = 6


def box_geom():
    return api.shell_box()


def bunny_geom():
    v, t = T.obj_mesh("stanford_bunny_309_faces.obj")
    return api.shell_fit(v["position"], y_up=True), t


def pyramid_geom():
    """The second geometry of the two-geometry case: a small four-sided pyramid beside the box, apex up, base open."""
    pos = np.array([[0.84, 0.84, 0.0], [0.98, 0.84, 0.0], [0.98, 0.98, 0.0], [0.84, 0.98, 0.0], [0.91, 0.91, 0.12]], np.float32)
    tri = np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]], np.uint32)
    return pos, tri


def height_field_geom(heights):
    """The two-triangles-per-texel height field of a square map in the unit tile, split along the TL-BR diagonal, heights at the
    texel corners as the displacement query samples them (the mean of the four texels around a corner, repeat wrap)."""
    n = heights.shape[0]
    corner = T.corner_heights64(heights).astype(np.float32)
    g = (np.arange(n + 1, dtype=np.float64) / n).astype(np.float32)
    pos = np.stack([np.tile(g, n + 1), np.repeat(g, n + 1), corner.reshape(-1)], 1).astype(np.float32)
    tri = []
    for y in range(n):
        for x in range(n):
            tl, tr, bl, br = y * (n + 1) + x, y * (n + 1) + x + 1, (y + 1) * (n + 1) + x, (y + 1) * (n + 1) + x + 1
            tri += [(tl, bl, br), (tl, br, tr)]
    return pos, np.array(tri, np.uint32)


CASES = {
    "quad_box": dict(mesh="quad", geoms=("box",), gp=dict(h_scale=2.0, tex_scale=(4.0, 4.0))),
    "quad_box_wrapped_rotated": dict(mesh="quad", geoms=("box",), gp=dict(h_scale=2.0, h_offset=0.01, h_bias=0.02, tex_scale=(4.0, 3.0), tex_rotation=30.0, tex_offset=(-2.3, -1.6))),
    "cap_box_small_tiles": dict(mesh="cap", geoms=("box",), gp=dict(h_scale=10.0, tex_scale=(27.0, 27.0))),
    "cap_box_one_tile": dict(mesh="cap", geoms=("box",), gp=dict(h_scale=1.0, tex_scale=(0.8, 0.8), tex_offset=(0.1, 0.1))),
    "quad_bunny": dict(mesh="quad", geoms=("bunny",), gp=dict(h_scale=0.6, tex_scale=(3.0, 3.0))),
    "cap_two_geoms": dict(mesh="cap", geoms=("box", "pyramid"), gp=dict(h_scale=4.0, tex_scale=(9.0, 9.0))),
}
GEOMS = {"box": box_geom, "bunny": bunny_geom, "pyramid": pyramid_geom}


def case_inputs(name):
    """(vertices, triangles, geoms, params, rays): shared by the CPU and the GPU tests."""
    c = CASES[name]
    v, t = T.quad_mesh() if c["mesh"] == "quad" else NH.cap_mesh(n=4, mirror=(1, 2))
    geoms = [GEOMS[g]() for g in c["geoms"]]
    o, d = T.cap_rays(N_RAYS) if c["mesh"] == "quad" else T.mesh_rays(v, N_RAYS, 5)
    bo, bd = T.pack_rays(np.full((N_BAD, 3), 0.5), np.tile([0.1, 0.2, -1.0], (N_BAD, 1)))
    bo[0, 0], bo[1, 1], bd[2, 2], bd[3, 0], bd[4, :3], bo[5, 3] = np.nan, np.inf, np.nan, -np.inf, 0.0, np.nan
    return v, t, geoms, api.shell_params(**c["gp"]), (np.concatenate([o, bo]), np.concatenate([d, bd]))
