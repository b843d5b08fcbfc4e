"""Shared by the motion tests of displaced instances (CPU and GPU): the host compilation of make_cur_to_prev
(gfxexp_amd/csrc/tfdm/tfdm_instance.hip.h) and of displaced_surface.hip.h with a motion table (tests/displaced_motion_host.cpp,
compiled into a directory the caller provides), and the float64 references both sides use."""
import ctypes as C
import os
import subprocess

import numpy as np

from gfxexp_amd import api
from tests import tfdm_host as T

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "displaced_motion_host.cpp")
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _m12(m):
    return np.ascontiguousarray(np.asarray(m, np.float32).reshape(-1)[:12])


class MotionHost:
    def __init__(self, out_dir):
        so = os.path.join(str(out_dir), "libdisplaced_motion_host.so")
        subprocess.check_call(["g++"] + T.FLAGS + [SRC, "-o", so])
        self.L = C.CDLL(so)

    def cur_to_prev(self, prev, cur):
        """curToPrev[12] float32 as gfx_tfdm_set_commit derives it; raises ValueError with the header's message."""
        out = np.zeros(12, np.float32)
        err = C.create_string_buffer(256)
        if self.L.motion_host_cur_to_prev(_p(_m12(prev)), _p(_m12(cur)), _p(out), err, C.c_uint32(256)):
            raise ValueError(err.value.decode())
        return out

    def prev_position(self, cur_to_prev, points):
        """One matrix (12 floats) for all points, or one per point ((n, 12))."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        m = np.ascontiguousarray(cur_to_prev, np.float32)
        per_point = m.size != 12
        assert m.size == (12 * len(pts) if per_point else 12)
        out = np.zeros_like(pts)
        self.L.motion_host_prev_position(_p(m), C.c_int(int(per_point)), _p(pts), C.c_uint32(len(pts)), _p(out))
        return out

    def resolve(self, table, motion, hits, org, dirs, base_verts, geom_slot, mat_slot, xy, prev_camera, width, height, reset_flow=False):
        """tests/displaced_host.py DisplacedHost.resolve with the motion table ((instances, 12) float32 or TFDM_MOTION_DTYPE; None: the
        form without a matrix)."""
        n = len(hits)
        table = np.ascontiguousarray(table, api.TFDM_INSTANCE_DTYPE)
        mo = None if motion is None else np.ascontiguousarray(np.asarray(motion).view(np.float32).reshape(-1, 12))
        assert mo is None or len(mo) == len(table)
        hits = np.ascontiguousarray(hits, api.SCENE_HIT_DTYPE)
        org, dirs = np.ascontiguousarray(org, np.float32).reshape(n, 4), np.ascontiguousarray(dirs, np.float32).reshape(n, 4)
        bv = np.ascontiguousarray(base_verts, np.float32).reshape(n, 15)
        gs, ms = np.ascontiguousarray(geom_slot, np.uint32).reshape(n), np.ascontiguousarray(mat_slot, np.uint32).reshape(n)
        xy = np.ascontiguousarray(xy, np.int32).reshape(n, 2)
        out = dict(points=np.zeros((n, 11), np.float32), g0=np.zeros((n, 4), np.uint32), g1=np.zeros((n, 2), np.float32),
                   g2=np.zeros((n, 4), np.uint32), g3=np.zeros((n, 4), np.uint32))
        self.L.motion_host_resolve(_p(table), _p(mo) if mo is not None else None, _p(hits), _p(org), _p(dirs), _p(bv), _p(gs), _p(ms), _p(xy), C.c_uint32(n),
                                   C.byref(prev_camera), C.c_float(width), C.c_float(height), C.c_int(int(reset_flow)), _p(out["points"]), _p(out["g0"]),
                                   _p(out["g1"]), _p(out["g2"]), _p(out["g3"]))
        return out


# ---------------------------------------------------------------- float64 references
def mat4(m):
    out = np.eye(4)
    out[:3] = np.asarray(m, np.float64).reshape(-1)[:12].reshape(3, 4)
    return out


def cur_to_prev64(prev, cur):
    """prev * inverse(cur) in float64 from the float32 entries: (3, 4)."""
    return (mat4(np.asarray(prev, np.float32)) @ np.linalg.inv(mat4(np.asarray(cur, np.float32))))[:3]


def project64(cam, pw, width, height):
    """PerspectiveCamera::calcScreenPosition times the image size, float64: the raster position of world points under a GfxCamera."""
    o = np.array(list(cam.orientation), np.float64).reshape(3, 3)
    pv = (np.asarray(pw, np.float64) - np.array(list(cam.position), np.float64)) @ np.linalg.inv(o).T
    hh = 2 * np.tan(np.float64(cam.fovY) / 2)
    ww = np.float64(cam.aspect) * hh
    sx = 1 - (pv[:, 0] / pv[:, 2] + 0.5 * ww) / ww
    sy = 1 - (pv[:, 1] / pv[:, 2] + 0.5 * hh) / hh
    return np.stack([sx * width, sy * height], 1)
