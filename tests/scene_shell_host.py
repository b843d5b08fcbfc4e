"""Shared by the tests of shell members in a scene query (CPU and GPU): the host compilation of
gfxexp_amd/csrc/nrtdsm/shell_instance.hip.h (tests/scene_shell_host.cpp, compiled into a directory the caller provides) behind
ctypes, and the scene both sides use.  Records of all kinds are TFDM_INSTANCE_DTYPE; the objects behind them are the host states of
tests/tfdm_host.py (kind 0), tests/nrtdsm_host.py (kind 1) and tests/shell_host.py (kind 2: the two height-map pointers carry the
shell BVH's nodes and triangles).  Ray transform, normal matrix, world-box test, ray sets and the numpy merge of the chain are those
of tests/scene_trace_host.py."""
import ctypes as C
import os
import subprocess

import numpy as np

from gfxexp_amd import api
from tests import nrtdsm_host as NH
from tests import scene_nrtdsm_host as M
from tests import scene_trace_host as S
from tests import shell_host as SH
from tests import tfdm_host as T

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "scene_shell_host.cpp")
TFDM, NRTDSM, SHELL = 0, 1, 2       # api.INSTANCE_*; written out so that this module imports where the api does not have them yet
INVALID = api.GFX_INVALID_SLOT
PART_DTYPE = np.dtype([("shellTriangle", "<u4"), ("shellGeom", "<u4"), ("tile", "<i4", 2)])     # api.SCENE_SHELL_PART_DTYPE


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class ThreeKindsHost:
    """shell_instance.hip.h on the host, behind ctypes."""

    def __init__(self, out_dir):
        so = os.path.join(str(out_dir), "libscene_shell_host.so")
        subprocess.check_call(["g++"] + T.FLAGS + [SRC, "-o", so])
        self.L = L = C.CDLL(so)
        L.scene_shell_host_sizeof.restype = C.c_uint32
        L.scene_shell_host_kind.restype = C.c_uint32
        assert L.scene_shell_host_sizeof(0) == api.TFDM_INSTANCE_DTYPE.itemsize and L.scene_shell_host_sizeof(1) == api.SCENE_HIT_DTYPE.itemsize
        assert L.scene_shell_host_sizeof(2) == api.HIT_DTYPE.itemsize and L.scene_shell_host_sizeof(3) == PART_DTYPE.itemsize == 16
        assert [L.scene_shell_host_kind(k) for k in range(3)] == [TFDM, NRTDSM, SHELL]

    def make_instance(self, kind, obj_to_world, root, ptrs, params, user_id=0):
        """One InstanceRecord of `kind`; ptrs: nodes, records, then heights, pyramid or (kind 2) shell nodes, shell triangles."""
        m = np.ascontiguousarray(obj_to_world, np.float32).reshape(-1)[:12].copy()
        rt = np.ascontiguousarray(np.asarray(root).reshape(1), api.TFDM_NODE_DTYPE)
        pp = np.array([int(x) for x in ptrs], np.uint64)
        out = np.zeros(1, api.TFDM_INSTANCE_DTYPE)
        err = C.create_string_buffer(256)
        if self.L.scene_shell_host_make_instance(C.c_uint32(kind), _p(m), _p(rt), _p(pp), C.byref(params), C.c_uint32(user_id), _p(out), err, C.c_uint32(256)):
            raise ValueError(err.value.decode())
        return out

    def instance_of_state(self, kind, st, obj_to_world, user_id=0):
        """A record whose pointers are the host arrays of a T.Host (kind 0), NH.Host (kind 1) or SH.Host (kind 2) state (kept alive by `st`)."""
        names = ("nodes", "records", "shell_nodes", "shell_tris") if kind == SHELL else ("nodes", "records", "levels", "pyramid")
        return self.make_instance(kind, obj_to_world, st["nodes"][0], [st[k].ctypes.data for k in names], st["params"], user_id)

    def trace(self, table, plain, mode, org, dirs, cull=True, counters=False, part=False):
        """The instance phase over three kinds on the host over a table of records with host pointers; arguments as SceneHost.trace.
        part: also the shell part of every closest hit (PART_DTYPE)."""
        org, dirs = np.ascontiguousarray(org, np.float32), np.ascontiguousarray(dirs, np.float32)
        table = np.ascontiguousarray(table, api.TFDM_INSTANCE_DTYPE)
        n = len(org)
        out = np.zeros(n, np.uint32 if mode == api.TRACE_ANY else api.SCENE_HIT_DTYPE)
        sp = np.full(n, 0x5A5A5A5A, np.uint32).repeat(4).view(PART_DTYPE)
        cnt = np.zeros(8, np.uint64)
        pl = None if plain is None else np.ascontiguousarray(plain)
        self.L.scene_shell_host_trace(_p(table) if len(table) else None, C.c_uint32(len(table)), _p(pl) if pl is not None else None, C.c_int(mode), _p(org), _p(dirs),
                                      C.c_uint32(n), _p(out), _p(sp) if part else None, _p(cnt) if counters else None, C.c_int(int(cull)))
        res = (out,)
        if part:
            res += (sp,)
        if counters:
            res += (cnt,)
        return res if len(res) > 1 else out


def part_of_chain(best, shell_hits):
    """The shell part the chain implies: best = the merged SCENE_HIT_DTYPE, shell_hits = {member index: SHELL_HIT_DTYPE of that member's
    step}.  The fields of the winning member's own hit where it is a shell member, zeros elsewhere."""
    part = np.zeros(len(best), PART_DTYPE)
    where = best["where"]
    disp = (where != INVALID) & (where != api.SCENE_PLAIN)
    for k, h in shell_hits.items():
        win = disp & (where >> 1 == k)
        for f in PART_DTYPE.names:
            part[f][win] = h[f][win]
    return part


# ---------------------------------------------------------------- the scene of the GPU chain test
def shell_objects():
    """[(kind, vertices, triangles, heights or geoms, params)]: the shell box on the quad (SH.CASES quad_box), the TFDM quad of
    S.chain_objects, the shell box + pyramid on the cap (cap_two_geoms), the NRTDSM quad of M.mixed_objects."""
    qv, qt, qg, qp, _ = SH.case_inputs("quad_box")
    cv, ct, cg, cp, _ = SH.case_inputs("cap_two_geoms")
    (tv, tt, th, tp), _ = S.chain_objects()
    return [(SHELL, qv, qt, qg, qp), (TFDM, tv, tt, th, tp), (SHELL, cv, ct, cg, cp), (NRTDSM, tv, tt, M.small_map(32), api.tfdm_params(h_scale=0.08))]


SHELL_QUAD_AT = (0.1, 0.3, 0.35)
CAP_AT = (1.05, 0.35, 0.6)


def shell_instances():
    """[(object index, objToWorld 3 x 4)]: the shell quad under a general rotation and the scale (1.5, 0.75, 2), cutting through the
    TFDM quad as the second instance of S.chain_instances does; the TFDM quad as it is; the shell cap mirrored in x, beside them; the
    NRTDSM quad mirrored in x where M.mixed_instances has it."""
    general = S.rotation((0.3, 1.0, 0.2), 35.0) @ np.diag([1.5, 0.75, 2.0])
    mirrored = np.diag([-0.6, 0.6, 0.6])
    return [(0, S.affine(general, SHELL_QUAD_AT)), (1, S.affine(np.eye(3), (0, 0, 0))), (2, S.affine(mirrored, np.array(CAP_AT) - mirrored @ np.array([0.0, 0.0, 1.0]))),
            (3, S.affine(np.diag([-1.0, 1.0, 1.0]), M.NRTDSM_QUAD_AT))]


def host_scene(hosts, zhost):
    """The scene above on the host.  hosts: {TFDM: T.Host, NRTDSM: NH.Host, SHELL: SH.Host}.  Returns (the objects' inputs, their host
    states, the table with host pointers: userId 100 + member index, as the GPU tests add them)."""
    inputs = shell_objects()
    states = [hosts[k].state(v, t, x, gp) for k, v, t, x, gp in inputs]
    table = np.concatenate([zhost.instance_of_state(inputs[o][0], states[o], m, 100 + k) for k, (o, m) in enumerate(shell_instances())])
    return inputs, states, table


def rays_of_table(table):
    """S.chain_rays over the members' padded world boxes"""
    return S.chain_rays([(table[k]["boxLo"].astype(np.float64), table[k]["boxHi"].astype(np.float64)) for k in range(len(table))])


def shares_of(where, members):
    """[plain, member 0, ..., miss]"""
    return [np.mean(where == api.SCENE_PLAIN)] + [np.mean((where >> 1 == k) & (where < api.SCENE_PLAIN)) for k in range(members)] + [np.mean(where == INVALID)]
