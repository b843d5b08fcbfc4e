"""Shared by the tests of NRTDSM members in a scene query (CPU and GPU): the host compilation of
gfxexp_amd/csrc/nrtdsm/nrtdsm_instance.hip.h (tests/scene_nrtdsm_host.cpp, compiled into a directory the caller provides) behind
ctypes, and the scene both sides use.  Records of both kinds are TFDM_INSTANCE_DTYPE; the objects behind them are the host states
of tests/tfdm_host.py (kind 0) and tests/nrtdsm_host.py (kind 1).  Ray transform, normal matrix, world-box test, ray sets and the
numpy merge of the chain are those of tests/scene_trace_host.py."""
import ctypes as C
import os
import subprocess

import numpy as np

from gfxexp_amd import api
from tests import nrtdsm_host as NH
from tests import scene_trace_host as S
from tests import tfdm_host as T

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "scene_nrtdsm_host.cpp")
TFDM, NRTDSM = api.INSTANCE_TFDM, api.INSTANCE_NRTDSM


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class MixedHost:
    """nrtdsm_instance.hip.h on the host, behind ctypes."""

    def __init__(self, out_dir):
        so = os.path.join(str(out_dir), "libscene_nrtdsm_host.so")
        subprocess.check_call(["g++"] + T.FLAGS + [SRC, "-o", so])
        self.L = L = C.CDLL(so)
        L.scene_nrtdsm_host_sizeof.restype = C.c_uint32
        L.scene_nrtdsm_host_kind.restype = C.c_uint32
        assert L.scene_nrtdsm_host_sizeof(0) == api.TFDM_INSTANCE_DTYPE.itemsize and L.scene_nrtdsm_host_sizeof(1) == api.SCENE_HIT_DTYPE.itemsize
        assert L.scene_nrtdsm_host_sizeof(2) == api.HIT_DTYPE.itemsize
        assert (L.scene_nrtdsm_host_kind(0), L.scene_nrtdsm_host_kind(1)) == (TFDM, NRTDSM)

    def make_instance(self, kind, obj_to_world, root, ptrs, params, user_id=0):
        """One InstanceRecord of `kind`; arguments as SceneHost.make_instance."""
        m = np.ascontiguousarray(obj_to_world, np.float32).reshape(-1)[:12].copy()
        rt = np.ascontiguousarray(np.asarray(root).reshape(1), api.TFDM_NODE_DTYPE)
        pp = np.array([int(x) for x in ptrs], np.uint64)
        out = np.zeros(1, api.TFDM_INSTANCE_DTYPE)
        err = C.create_string_buffer(256)
        if self.L.scene_nrtdsm_host_make_instance(C.c_uint32(kind), _p(m), _p(rt), _p(pp), C.byref(params), C.c_uint32(user_id), _p(out), err, C.c_uint32(256)):
            raise ValueError(err.value.decode())
        return out

    def instance_of_state(self, kind, st, obj_to_world, user_id=0):
        """A record whose pointers are the host arrays of a T.Host (kind 0) or NH.Host (kind 1) state (kept alive by `st`)."""
        ptrs = [st[k].ctypes.data for k in ("nodes", "records", "levels", "pyramid")]
        return self.make_instance(kind, obj_to_world, st["nodes"][0], ptrs, st["params"], user_id)

    def trace(self, table, plain, mode, org, dirs, cull=True, counters=False):
        """The mixed instance phase on the host over a table of records with host pointers; arguments as SceneHost.trace."""
        org, dirs = np.ascontiguousarray(org, np.float32), np.ascontiguousarray(dirs, np.float32)
        table = np.ascontiguousarray(table, api.TFDM_INSTANCE_DTYPE)
        n = len(org)
        out = np.zeros(n, np.uint32 if mode == api.TRACE_ANY else api.SCENE_HIT_DTYPE)
        cnt = np.zeros(8, np.uint64)
        pl = None if plain is None else np.ascontiguousarray(plain)
        self.L.scene_nrtdsm_host_trace(_p(table) if len(table) else None, C.c_uint32(len(table)), _p(pl) if pl is not None else None, C.c_int(mode), _p(org), _p(dirs),
                                       C.c_uint32(n), _p(out), _p(cnt) if counters else None, C.c_int(int(cull)))
        return (out, cnt) if counters else out


# ---------------------------------------------------------------- the mixed scene of the GPU chain test
def small_map(n=32):
    """A procedural 32 x 32 map in [0, 1], quantised to 8 bits as T.two_sine_map is."""
    y, x = np.mgrid[0:n, 0:n]
    h = 0.5 + 0.3 * np.sin(2 * np.pi * 2 * x / n) * np.sin(2 * np.pi * 3 * y / n) + 0.15 * np.cos(2 * np.pi * (3 * x - 2 * y) / n)
    return (np.round(np.clip(h, 0, 1) * 255).astype(np.float32) / np.float32(255)).astype(np.float32)


def mixed_objects():
    """[(kind, vertices, triangles, heights, params)]: the TFDM quad and bunny base of S.chain_objects, the NRTDSM cap, the NRTDSM quad."""
    (qv, qt, qh, qp), (bv, bt, bh, bp) = S.chain_objects()
    cv, ct = NH.cap_mesh()
    return [(TFDM, qv, qt, qh, qp), (NRTDSM, cv, ct, T.two_sine_map(64), api.tfdm_params(h_scale=0.05)), (TFDM, bv, bt, bh, bp),
            (NRTDSM, qv, qt, small_map(32), api.tfdm_params(h_scale=0.08))]


CAP_MIDDLE = (0.45, 0.75, 0.3)
NRTDSM_QUAD_AT = (2.2, 0.45, 0.0)


def mixed_instances():
    """[(object index, objToWorld 3 x 4)]: the TFDM quad as it is; the NRTDSM cap rotated and scaled (1.5, 0.75, 2), its middle (the
    object-space point (0, 0, 1)) moved to where it cuts through the quad; the TFDM bunny base mirrored in x (the case of
    S.chain_instances); the NRTDSM quad mirrored in x beside the first quad."""
    general = S.rotation((0.3, 1.0, 0.2), 35.0) @ np.diag([1.5, 0.75, 2.0])
    _, _, mirrored_bunny = S.chain_instances()
    return [(0, S.affine(np.eye(3), (0, 0, 0))), (1, S.affine(general, np.array(CAP_MIDDLE) - general @ np.array([0.0, 0.0, 1.0]))), (2, mirrored_bunny[1]),
            (3, S.affine(np.diag([-1.0, 1.0, 1.0]), NRTDSM_QUAD_AT))]
