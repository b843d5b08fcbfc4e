"""Shared by the height-map update tests (CPU and GPU): the host model of gfx_tfdm_update_heights (tests/tfdm_update_host.cpp,
compiled into a directory the caller provides) behind ctypes, and the checks of a refitted tree that need no compiled code."""
import ctypes as C
import os
import subprocess

import numpy as np

from gfxexp_amd import api
from tests import tfdm_host as T

SRC = os.path.join(T.HERE, "tfdm_update_host.cpp")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class UpdateHost:
    def __init__(self, out_dir):
        so = os.path.join(str(out_dir), "libtfdm_update_host.so")
        subprocess.check_call(["g++"] + T.FLAGS + [SRC, "-o", so])
        self.L = L = C.CDLL(so)
        for n in ("tfdm_update_host_check_rect", "tfdm_update_host_check_all"):
            getattr(L, n).restype = C.c_uint32
        for n in ("tfdm_update_host_refit", "tfdm_update_host_update"):
            getattr(L, n).restype = C.c_int

    def dirty(self, size, rect):
        """[levels, 8]: hx.start, hx.len, hy.start, hy.len, px.start, px.len, py.start, py.len"""
        out = np.zeros((int(np.log2(size)) + 1, 8), np.uint32)
        self.L.tfdm_update_host_dirty(C.c_uint32(size), *[C.c_uint32(v) for v in rect], _p(out))
        return out

    def region(self, levels, pyramid, size, new_map, rect):
        """The region update in place on `levels` / `pyramid` (all levels, as Host.levels / Host.pyramid make them); returns the number
        of height and pyramid texels written per level, [levels, 2]."""
        x0, y0, w, h = rect
        src = np.ascontiguousarray(new_map[y0:y0 + h, x0:x0 + w], np.float32)
        counts = np.zeros((int(np.log2(size)) + 1, 2), np.uint32)
        self.L.tfdm_update_host_region(_p(levels), _p(pyramid), C.c_uint32(size), _p(src), C.c_uint32(w), *[C.c_uint32(v) for v in rect], _p(counts))
        return counts

    def check_rect(self, old, new, rect):
        size = old.shape[0]
        return self.L.tfdm_update_host_check_rect(C.c_uint32(size), _p(np.ascontiguousarray(old, np.float32)), _p(np.ascontiguousarray(new, np.float32)),
                                                  *[C.c_uint32(v) for v in rect])

    def check_all(self, old, new):
        """(rectangles that differ, rectangles tried, the first that differs as x0, y0, w, h, code)"""
        size = old.shape[0]
        n, first = C.c_uint32(), np.zeros(5, np.uint32)
        bad = self.L.tfdm_update_host_check_all(C.c_uint32(size), _p(np.ascontiguousarray(old, np.float32)), _p(np.ascontiguousarray(new, np.float32)), C.byref(n), _p(first))
        return bad, n.value, first

    def refit(self, nodes, aabbs):
        """(refitted copy of `nodes`, leaves whose primitive's box is empty, number of depths)"""
        out = np.ascontiguousarray(nodes, api.TFDM_NODE_DTYPE).copy()
        depths = C.c_uint32()
        r = self.L.tfdm_update_host_refit(_p(out), C.c_uint32(len(out)), _p(np.ascontiguousarray(aabbs, np.float32)), C.byref(depths))
        assert r >= 0, "the nodes are not a tree"
        return out, r, depths.value

    def update_state(self, st, new_map, rect):
        """The whole update on a copy of a Host.state dict."""
        x0, y0, w, h = rect
        out = dict(st)
        for k in ("levels", "pyramid", "aabbs", "nodes"):
            out[k] = np.ascontiguousarray(st[k]).copy()
        src = np.ascontiguousarray(new_map[y0:y0 + h, x0:x0 + w], np.float32)
        r = self.L.tfdm_update_host_update(_p(out["levels"]), _p(out["pyramid"]), C.c_uint32(st["size"]), _p(src), C.c_uint32(w), *[C.c_uint32(v) for v in rect],
                                           _p(st["records"]), C.c_uint32(len(st["records"])), C.byref(st["params"]), _p(out["aabbs"]), _p(out["nodes"]),
                                           C.c_uint32(len(out["nodes"])))
        assert r >= 0
        return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def box_empty(aabbs):
    b = np.asarray(aabbs, np.float32).reshape(-1, 6)
    return ~np.all(b[:, :3] <= b[:, 3:], axis=1)


def assert_refitted(what, nodes, before, aabbs):
    """`nodes` has the shape of `before`; every leaf's box is its primitive's (an empty one keeps the box it had); every inner box is
    the min / max of its two children's, bit for bit."""
    assert len(nodes) == len(before), what
    assert np.array_equal(nodes["first"], before["first"]) and np.array_equal(nodes["count"], before["count"]), what + ": the tree's shape changed"
    aabbs = np.asarray(aabbs, np.float32).reshape(-1, 6)
    leaf = nodes["count"] != 0
    prim = nodes["first"][leaf]
    want_lo, want_hi = aabbs[prim, :3].copy(), aabbs[prim, 3:].copy()
    keep = box_empty(aabbs)[prim]
    want_lo[keep], want_hi[keep] = before["lo"][leaf][keep], before["hi"][leaf][keep]
    assert np.array_equal(_bits(nodes["lo"][leaf]), _bits(want_lo)) and np.array_equal(_bits(nodes["hi"][leaf]), _bits(want_hi)), what + ": a leaf is not its primitive's box"
    inner = ~leaf
    a, b = nodes["first"][inner], nodes["first"][inner] + 1
    lo = np.where(nodes["lo"][b] < nodes["lo"][a], nodes["lo"][b], nodes["lo"][a])
    hi = np.where(nodes["hi"][a] < nodes["hi"][b], nodes["hi"][b], nodes["hi"][a])
    assert np.array_equal(_bits(nodes["lo"][inner]), _bits(lo)) and np.array_equal(_bits(nodes["hi"][inner]), _bits(hi)), what + ": an inner box is not the union of its children"


def bumped_map(heights, rect, seed):
    """`heights` with a seeded bump added inside the rectangle, clipped to [0, 1]; every texel of the rectangle changes."""
    x0, y0, w, h = rect
    rng = np.random.default_rng(seed)
    out = np.array(heights, np.float32, copy=True)
    cur = out[y0:y0 + h, x0:x0 + w]
    step = rng.uniform(0.15, 0.45, cur.shape).astype(np.float32)
    out[y0:y0 + h, x0:x0 + w] = np.where(cur < np.float32(0.5), cur + step, cur - step).astype(np.float32)
    return np.clip(out, 0, 1).astype(np.float32)
