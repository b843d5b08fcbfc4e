"""Shared by the tests of gfx_scene_bind_displaced_kinds (CPU and GPU): the host compilation of
gfxexp_amd/csrc/nrtdsm/displaced_kinds.hip.h (tests/displaced_kinds_host.cpp, compiled into a directory the caller provides) behind
ctypes, and the scene both sides use: its objects are those of tests/scene_shell_host.py and tests/scene_nrtdsm_host.py, taken by import.

The scene (z up): the plain bunny and an emissive rectangle in the BVH8, and a set of four members --
  0  the TFDM quad, three units wide: the ground;
  1  the NRTDSM cap;
  2  the shell box + pyramid on the cap (two shell geometries, two Lambert materials of different constant reflectance);
  3  the NRTDSM quad, mirrored in x, hovering.
CAMERAS: two positions of a moving camera from which the plain geometry and every member own at least 2 % of the 96 x 64 pixels and
both shell geometries are seen; tests/test_displaced_kinds_cpu.py holds that on the host, the GPU test on the device."""
import ctypes as C
import os
import subprocess

import numpy as np

from gfxexp_amd import api
from tests import displaced_host as D
from tests import scene_nrtdsm_host as M
from tests import scene_shell_host as Z
from tests import scene_trace_host as S
from tests import shell_host as SH
from tests import tfdm_host as T

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "displaced_kinds_host.cpp")
INVALID = api.GFX_INVALID_SLOT
W, H = 96, 64
RX90 = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], np.float64)      # the y-up bunny onto z-up


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class KindsHost:
    """displaced_kinds.hip.h on the host, behind ctypes."""

    def __init__(self, out_dir):
        so = os.path.join(str(out_dir), "libdisplaced_kinds_host.so")
        subprocess.check_call(["g++"] + T.FLAGS + [SRC, "-o", so])
        self.L = L = C.CDLL(so)
        L.displaced_kinds_host_sizeof.restype = C.c_uint32
        L.displaced_kinds_host_constant.restype = C.c_uint32
        assert [L.displaced_kinds_host_sizeof(k) for k in range(5)] == [api.TFDM_INSTANCE_DTYPE.itemsize, api.SCENE_HIT_DTYPE.itemsize, C.sizeof(api.GfxCamera), 16, 40]

    def constant(self, what):
        return int(self.L.displaced_kinds_host_constant(C.c_int(what)))

    def material(self, kind, member, shell_geom, geom_mat, shell_mats):
        a = [np.ascontiguousarray(x, np.uint32).reshape(-1) for x in (kind, member, shell_geom, geom_mat)]
        sm = np.ascontiguousarray(shell_mats, np.uint32).reshape(-1)
        out = np.zeros(len(a[0]), np.uint32)
        self.L.displaced_kinds_host_material(_p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), _p(sm), C.c_uint32(len(out)), _p(out))
        return out

    def word(self, slot, shell_geom):
        s, g = np.ascontiguousarray(slot, np.uint32).reshape(-1), np.ascontiguousarray(shell_geom, np.uint32).reshape(-1)
        w, sb, gb = (np.zeros(len(s), np.uint32) for _ in range(3))
        self.L.displaced_kinds_host_word(_p(s), _p(g), C.c_uint32(len(s)), _p(w), _p(sb), _p(gb))
        return w, sb, gb

    def resolve(self, table, hits, parts, org, dirs, base_verts, geom_slots, geom_mats, shell_mats, xy, prev_camera, width, height, reset_flow=False,
                cur_to_prev=None, plain_form=False):
        """One displaced hit per entry (with its shell part) -> dict(points (n, 11); g0, g2, g3 (n, 4) uint32; g1 (n, 2); mat (n,)).  geom_slots /
        geom_mats: per MEMBER; shell_mats: 8 per member; cur_to_prev: (members, 12) or None."""
        n = len(hits)
        table = np.ascontiguousarray(table, api.TFDM_INSTANCE_DTYPE)
        hits = np.ascontiguousarray(hits, api.SCENE_HIT_DTYPE)
        parts = np.ascontiguousarray(parts, api.SCENE_SHELL_PART_DTYPE)
        org, dirs = np.ascontiguousarray(org, np.float32).reshape(n, 4), np.ascontiguousarray(dirs, np.float32).reshape(n, 4)
        bv = np.ascontiguousarray(base_verts, np.float32).reshape(n, 15)
        gs, gm = np.ascontiguousarray(geom_slots, np.uint32).reshape(-1), np.ascontiguousarray(geom_mats, np.uint32).reshape(-1)
        sm = np.ascontiguousarray(shell_mats, np.uint32).reshape(-1)
        assert len(gs) == len(gm) == len(table) and len(sm) == 8 * len(table)
        ctp = None if cur_to_prev is None else np.ascontiguousarray(cur_to_prev, np.float32).reshape(len(table), 12)
        xy = np.ascontiguousarray(xy, np.int32).reshape(n, 2)
        out = dict(points=np.zeros((n, 11), np.float32), g0=np.zeros((n, 4), np.uint32), g1=np.zeros((n, 2), np.float32),
                   g2=np.zeros((n, 4), np.uint32), g3=np.zeros((n, 4), np.uint32), mat=np.zeros(n, np.uint32))
        self.L.displaced_kinds_host_resolve(_p(table), _p(hits), _p(parts), _p(org), _p(dirs), _p(bv), _p(gs), _p(gm), _p(sm), _p(ctp) if ctp is not None else None,
                                            _p(xy), C.c_uint32(n), C.byref(prev_camera), C.c_float(width), C.c_float(height), C.c_int(int(reset_flow)),
                                            _p(out["points"]), _p(out["g0"]), _p(out["g1"]), _p(out["g2"]), _p(out["g3"]), _p(out["mat"]), C.c_int(int(plain_form)))
        return out


# ---------------------------------------------------------------- the scene
LAMBERT = 0
GROUND_RGB, CAP_RGB, SHELL_BASE_RGB, NQUAD_RGB = (0.7, 0.7, 0.7), (0.8, 0.3, 0.2), (0.5, 0.5, 0.5), (0.3, 0.8, 0.3)
SHELL_RGB = [(0.2, 0.6, 0.8), (0.9, 0.8, 0.1)]          # shell geometry 0 (the box), 1 (the pyramid)


def lambert(rgb):
    m = api.GfxMaterial()
    m.bsdfType = LAMBERT
    m.a = (C.c_float * 3)(*rgb)
    return m


def flat_quad(x0, y0, x1, y1, z, up=True):
    v = np.zeros(4, api.VERTEX_DTYPE)
    v["position"] = [(x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)]
    v["normal"] = (0, 0, 1 if up else -1)
    v["texCoord0Dir"] = (1, 0, 0)
    v["texCoord"] = [(0, 0), (1, 0), (1, 1), (0, 1)]
    return v, np.array([[0, 1, 2], [0, 2, 3]] if up else [[0, 2, 1], [0, 3, 2]], np.uint32)


def objects():
    """[(kind, vertices, triangles, heights or shell geometries, params)]: the TFDM quad of S.chain_objects, the NRTDSM cap and the NRTDSM
    quad of M.mixed_objects, the shell box + pyramid on the cap of Z.shell_objects."""
    mixed = M.mixed_objects()
    shells = Z.shell_objects()
    assert mixed[0][0] == Z.TFDM and mixed[1][0] == mixed[3][0] == Z.NRTDSM and shells[2][0] == Z.SHELL and len(shells[2][3]) == 2
    return [mixed[0], mixed[1], shells[2], mixed[3]]


GROUND = S.affine(np.diag([3.0, 3.0, 1.0]), (-0.5, -0.5, 0.0))
CAP = S.affine(np.diag([0.9, 0.9, 0.9]), (0.55, 0.45, -0.55))
SHELL_CAP = S.affine(np.diag([1.1, 1.1, 1.1]), (1.75, 0.75, -0.75))
NQUAD = S.affine(S.rotation((1.0, 0.0, 0.0), 50.0) @ np.diag([-1.0, 1.0, 1.0]), (1.75, 1.75, 0.2))
TRANSFORMS = [GROUND, CAP, SHELL_CAP, NQUAD]
BUNNY = S.affine(RX90 * 0.01, (0.1, 1.4, 0.1))
CAMERAS = [((1.0, -2.1, 1.9), (1.0, 0.95, 0.25)), ((1.15, -2.05, 1.85), (1.0, 0.95, 0.25))]


def camera(k, w=W, h=H):
    return T.look_at_camera(w, h, CAMERAS[k][0], CAMERAS[k][1], fov_y_deg=40.0)


class SceneParts:
    """The host scene before upload: the BVH8 part (bunny, lamp), the ungrouped shading geometry of the four members, the materials."""

    def __init__(self, plain_extra=None):
        self.hs = hs = api.HostScene()
        self.light = hs.add_material_traditional((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0.0, emittance=(30.0, 30.0, 30.0))
        self.geom_mats = [hs.add_material(lambert(c)) for c in (GROUND_RGB, CAP_RGB, SHELL_BASE_RGB, NQUAD_RGB)]
        self.shell_mats = [hs.add_material(lambert(c)) for c in SHELL_RGB]
        g = hs.load_obj(os.path.join(T.ASSETS, "stanford_bunny_309_faces.obj"))
        hs.add_instance(g, BUNNY)
        self.lamp = hs.add_geom(*flat_quad(0.2, 0.0, 1.8, 1.6, 3.0, up=False), self.light)
        hs.add_instance(hs.add_group([self.lamp]), S.affine(np.eye(3), (0, 0, 0)))
        if plain_extra is not None:
            plain_extra(self, hs)
        self.inputs = objects()
        # the shading geometry of the members: in NO group, so not in the BVH8
        self.slots = [hs.add_geom(inp[1], inp[2], m) for inp, m in zip(self.inputs, self.geom_mats)]

    def members(self):
        """what api.Context.bind_displaced_kinds takes"""
        return [self.slots[0], self.slots[1], (self.slots[2], self.shell_mats), self.slots[3]]

    def shell_mat_table(self):
        t = np.zeros((4, 8), np.uint32)
        t[2, :2] = self.shell_mats
        return t


def host_table(hosts, zhost):
    """The four members on the host: (host states, the table with host pointers; userId 100 + k)."""
    inputs = objects()
    states = [hosts[k].state(v, t, x, gp) for k, v, t, x, gp in inputs]
    table = np.concatenate([zhost.instance_of_state(inputs[k][0], states[k], TRANSFORMS[k], 100 + k) for k in range(4)])
    return states, table


def shares_of(where, part):
    """[plain, member 0..3, miss, shell geometry 0, shell geometry 1] as shares of the rays"""
    disp = (where != INVALID) & (where != api.SCENE_PLAIN)
    on_shell = disp & (where >> 1 == 2)
    return ([np.mean(where == api.SCENE_PLAIN)] + [np.mean(disp & (where >> 1 == k)) for k in range(4)] + [np.mean(where == INVALID)] +
            [np.mean(on_shell & (part["shellGeom"] == g)) for g in range(2)])


def base_verts(inputs, hits):
    """(n, 15) for displaced hits of any member"""
    bv = np.zeros((len(hits), 15), np.float32)
    inst = hits["where"] >> 1
    for k in range(len(inputs)):
        m = inst == k
        bv[m] = D.base_verts_of(inputs[k][1], inputs[k][2], hits["index"][m])
    return bv
