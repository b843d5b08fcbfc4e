"""-m gpu: displaced instances that move (gfx_tfdm_set_move): the motion table, the motion vector of the G-buffer pass and the
consumers that reproject through it.

Scenes, frame size and helpers are those of tests/test_gpu_displaced_render.py, plus the wall scene defined here (a plain floor and
lamp, a fixed displaced ground quad, a displaced wall with a smooth height map that translates).  What each case is held against:
  * every G-buffer word of a displaced pixel: the host compilation of csrc/tfdm/displaced_surface.hip.h with the motion table
    (tests/displaced_motion_host.cpp), fed the gfx_trace_scene hit of the pixel's primary ray and read_motion(); every other pixel
    and the RNG: the same frame under a set that was teleported (set_transform) to the same transforms;
  * a move to where the instance already is: a set that was never moved, every buffer;
  * the motion vector: the tessellated quad as a plain animated instance (gfx_instance_set_transform), by the bound computed at the
    test from E_mesh;
  * reprojection: frame 1's pixel under the motion vector shows the same point of the instance's surface, to the pixel's own footprint;
  * gfx_restir_copy_taa_flow_to_linear and the temporal pass's neighbour index follow.
Measured on an MI355X: DESIGN.md section 19."""
import ctypes as C

import numpy as np
import pytest

from gfxexp_amd import api
from tests import displaced_host as D
from tests import displaced_motion_host as M
from tests import scene_trace_host as S
from tests import test_gpu_displaced_render as DR
from tests import test_gpu_displaced_restir as RS
from tests import tfdm_host as T
from tests import util
from tests.test_gpu_tfdm import EDGE_CAP, _clip, _upload_mesh

pytestmark = pytest.mark.gpu
INVALID = api.GFX_INVALID_SLOT
W, H = DR.W, DR.H
_stream = DR._stream
_words = DR._words


@pytest.fixture(scope="module")
def mhost(built_lib, tmp_path_factory):
    return M.MotionHost(tmp_path_factory.mktemp("displaced_motion_host"))


@pytest.fixture(scope="module")
def e_mesh(built_lib):
    """E_mesh as tests/test_gpu_tfdm.py measures it, in this run: the largest |t - t64| / max(1, t64) of gfx_trace on the tessellated
    64 x 64 quad against the float64 brute force, over the rays the edge rule keeps -- here over 2500 rays of that file's ray
    generator instead of its 20 000 (the brute force is the cost): a maximum over fewer rays is no larger, so the bound made from it
    is no wider."""
    v, t = T.quad_mesh()
    mm = T.MicroMesh(v, t, T.mips32(T.two_sine_map(64)), api.tfdm_params(h_scale=0.1))
    ctx, accel = _upload_mesh(*mm.float32_mesh())
    org, dirs = T.cap_rays(2500)
    hits = util.gpu_trace(ctx, accel, api.TRACE_CLOSEST, org, dirs)
    t64, _, edge, near = T.brute64(mm.A, mm.B, mm.C, org[:, :3], dirs[:, :3], org[:, 3].astype(np.float64), dirs[:, 3].astype(np.float64), clip=_clip(mm))
    keep = ~(edge | near)
    assert (~keep).mean() <= EDGE_CAP
    got_hit = hits["triIndex"] != api.GFX_INVALID_SLOT
    assert np.array_equal(got_hit[keep], np.isfinite(t64)[keep])
    both = keep & got_hit
    e = float((np.abs(hits["dist"][both].astype(np.float64) - t64[both]) / np.maximum(1.0, t64[both])).max())
    print("E_mesh = %.3e (gfx_trace on the tessellated 64 x 64 quad against float64, %d rays)" % (e, both.sum()))
    assert 0 < e < 1e-4
    return e


# ---------------------------------------------------------------- transforms
def translated(m, d):
    out = np.array(m, np.float32).copy()
    out[:, 3] = (out[:, 3].astype(np.float64) + np.asarray(d, np.float64)).astype(np.float32)
    return out


def rotated_about(m, centre_obj, axis, degrees):
    """`m` followed by a rotation about the world image of the object point `centre_obj`."""
    m64 = np.asarray(m, np.float64)
    c = m64[:, :3] @ np.asarray(centre_obj, np.float64) + m64[:, 3]
    R = S.rotation(axis, degrees)
    return S.affine(R @ m64[:, :3], R @ (m64[:, 3] - c) + c)


MOVED0 = translated(DR.HOVER, (0.2, 0.1, 0.05))
MOVED1 = rotated_about(DR.GENERAL, (0.5, 0.5, 0.0), (0.0, 0.0, 1.0), 10.0)


def to_object64(m, pw):
    m64 = np.asarray(m, np.float32).astype(np.float64)
    return (np.asarray(pw, np.float64) - m64[:, 3]) @ np.linalg.inv(m64[:, :3]).T


def twin_set(sc):
    """A second set over the objects of a DR.Scene, under the same transforms."""
    s = api.TfdmSet(sc.ctx)
    for k, (o, m, _) in enumerate(sc.members):
        assert s.add(sc.tfdm[o], m, 50 + k) == k
    s.commit()
    return s


def primary_hits(sc, tset, w, h):
    """The primary rays of the current parameters and their gfx_trace_scene hits: (org, dirs, hits)."""
    import torch
    n = w * h
    d_org, d_dir = torch.zeros(n * 4, dtype=torch.float32, device="cuda"), torch.zeros(n * 4, dtype=torch.float32, device="cuda")
    d_hit = torch.zeros(n * 8, dtype=torch.int32, device="cuda")
    sc.ctx.restir_primary_rays(w, h, d_org.data_ptr(), d_dir.data_ptr(), _stream())
    api.trace_scene(sc.ctx, sc.accel, tset, api.TRACE_CLOSEST, d_org.data_ptr(), d_dir.data_ptr(), n, d_hit.data_ptr(), stream=_stream())
    torch.cuda.synchronize()
    return d_org.cpu().numpy().reshape(n, 4), d_dir.cpu().numpy().reshape(n, 4), d_hit.cpu().numpy().view(api.SCENE_HIT_DTYPE).reshape(n)


# ---------------------------------------------------------------- 4. every G-buffer word, bit for bit
@pytest.mark.parametrize("second_camera", [0, 1])
def test_gbuffer_of_a_moved_set_bit_for_bit(built_lib, mhost, second_camera):
    sc = DR.Scene()
    ctx = sc.ctx
    tele = twin_set(sc)
    cams = [DR.camera(0), DR.camera(second_camera)]
    finals = [DR.HOVER, DR.GENERAL, DR.MIRRORED]
    bound, ref = DR.Frames(sc), DR.Frames(sc)
    n = W * H
    xy = np.stack([np.arange(n) % W, np.arange(n) // W], 1)
    for frame in range(2):
        if frame:
            sc.set.move(0, MOVED0)
            sc.set.move(1, MOVED1)
            sc.set.commit()
            tele.set_transform(0, MOVED0)
            tele.set_transform(1, MOVED1)
            tele.commit()
            finals = [MOVED0, MOVED1, DR.MIRRORED]
        table, motion = sc.set.read(), sc.set.read_motion()
        # the tables against the host derivation; the teleported set has the same records and no motion
        firsts = [DR.HOVER, DR.GENERAL, DR.MIRRORED]
        for k in range(3):
            util.assert_same_bits("frame %d: curToPrev of instance %d" % (frame, k), motion["curToPrev"][k], mhost.cur_to_prev(firsts[k], finals[k]))
            assert np.array_equal(table["objToWorld"][k].reshape(3, 4), finals[k])
        util.assert_same_bits("frame %d: records of the teleported set" % frame, tele.read(), table)
        assert all(m.tobytes() == M.IDENTITY.tobytes() for m in tele.read_motion()["curToPrev"])
        assert motion["curToPrev"][2].tobytes() == M.IDENTITY.tobytes()
        assert (motion["curToPrev"][0].tobytes() != M.IDENTITY.tobytes()) == bool(frame)
        # plain pixels, misses, the RNG: the same frame from the same state under the teleported set
        ref.copy_state_from(bound)
        ctx.bind_displaced(tele, sc.slots)
        ref.set_params(frame, cams[frame], cams[frame - 1] if frame else None, jitter=1)
        ref.gbuffer()
        want = ref.dev.download()
        ctx.bind_displaced(sc.set, sc.slots)
        f = bound.set_params(frame, cams[frame], cams[frame - 1] if frame else None, jitter=1)
        org, dirs, hits = primary_hits(sc, sc.set, W, H)
        bound.gbuffer()
        got = bound.dev.download()
        b = frame % 2
        util.assert_same_bits("frame %d: RNG after the pass" % frame, got["rng"], want["rng"])
        where = hits["where"]
        disp = (where != INVALID) & (where != api.SCENE_PLAIN)
        for k in ("gb0", "gb1", "gb2", "gb3"):
            util.assert_same_bits("frame %d: %s of plain and empty pixels" % (frame, k), _words(got["%s_%d" % (k, b)])[~disp], _words(want["%s_%d" % (k, b)])[~disp])
        for k in ("gb0", "gb2", "gb3", "albedo", "normal"):       # a move changes the motion vector of a displaced pixel and nothing else
            key = "%s_%d" % (k, b) if k.startswith("gb") else k
            util.assert_same_bits("frame %d: %s of displaced pixels against the teleported set" % (frame, k), _words(got[key])[disp], _words(want[key])[disp])
        idx = np.nonzero(disp)[0]
        inst = where[idx] >> 1
        bv = np.zeros((len(idx), 15), np.float32)
        for k in range(3):
            m = inst == k
            bv[m] = D.base_verts_of(sc.meshes[k][0], sc.meshes[k][1], hits["index"][idx][m])
        geom = np.array(sc.slots, np.uint32)[inst]
        mat = np.array([m for _, _, m in sc.members], np.uint32)[inst]
        host = mhost.resolve(table, motion, hits[idx], org[idx], dirs[idx], bv, geom, mat, xy[idx], f.prevCamera, W, H, reset_flow=frame == 0)
        for k in ("g0", "g1", "g2", "g3"):
            util.assert_same_bits("frame %d: gbuffer%s of displaced pixels" % (frame, k[1]), _words(got["gb%s_%d" % (k[1], b)])[idx], _words(host[k]))
        shares = [np.mean(disp & (where >> 1 == k)) for k in range(3)]
        print("frame %d: instances %s %% of the pixels" % (frame, ["%.1f" % (100 * s) for s in shares]))
        assert all(s >= 0.02 for s in shares), shares
        if frame:
            own = np.abs(got["gb1_%d" % b][idx] - want["gb1_%d" % b][idx]).max(1)
            print("frame 1: motion of the instances themselves, worst per instance %s pixels" % ["%.2f" % own[inst == k].max() for k in range(3)])
            assert own[inst == 0].min() > 0.5 and own[inst == 1].max() > 0.5, "the moved instances carry a flow of their own"
            assert own[inst == 2].max() == 0.0, "the one that stayed carries the camera's alone"
    ctx.bind_displaced(None)


# ---------------------------------------------------------------- 5. still means still
def test_a_move_to_the_same_place_is_no_move(built_lib):
    cams = [DR.camera(0), DR.camera(1)]
    fresh = DR.Scene()
    fresh.bind()
    want = DR.Frames(fresh).render(2, 5, 1, cams)
    fresh.unbind()
    sc = DR.Scene()
    never = sc.set.read_motion()
    for k, (_, m, _) in enumerate(sc.members):
        sc.set.move(k, m)
    sc.set.commit()
    util.assert_same_bits("motion table after moves to the same place", sc.set.read_motion(), never)
    assert all(m.tobytes() == M.IDENTITY.tobytes() for m in never["curToPrev"])
    sc.bind()
    got = DR.Frames(sc).render(2, 5, 1, cams)
    DR.assert_same_buffers("moved to where it was", got, want)
    # set_transform after a move: identity motion for that member, and the moved one keeps its own
    sc.set.move(0, MOVED0)
    sc.set.move(1, MOVED1)
    sc.set.set_transform(0, translated(MOVED0, (0.0, 0.1, 0.0)))
    sc.set.commit()
    motion = sc.set.read_motion()["curToPrev"]
    assert motion[0].tobytes() == M.IDENTITY.tobytes() and motion[2].tobytes() == M.IDENTITY.tobytes()
    assert motion[1].tobytes() != M.IDENTITY.tobytes()
    fr = DR.Frames(sc)
    fr.set_params(1, cams[0], cams[0])
    fr.gbuffer()
    out = fr.dev.download()
    g0, mv = out["gb0_1"]["instSlot"], out["gb1_1"]
    assert np.abs(mv[g0 == (api.GBUFFER_DISPLACED | 0)]).max() <= 5e-4, "a teleported instance under a still camera: no flow"
    assert np.abs(mv[g0 == (api.GBUFFER_DISPLACED | 1)]).max() > 0.5
    sc.unbind()


# ---------------------------------------------------------------- 6. against the trusted plain path
def projection_gain(cam, pw, width, height):
    """Per raster axis, the 2-norm of d(raster position) / d(world position) at the world points `pw` under `cam`: (n, 2)."""
    o = np.array(list(cam.orientation), np.float64).reshape(3, 3)
    oi = np.linalg.inv(o)
    pv = (np.asarray(pw, np.float64) - np.array(list(cam.position), np.float64)) @ oi.T
    hh = 2 * np.tan(np.float64(cam.fovY) / 2)
    ww = np.float64(cam.aspect) * hh
    gx = (width / (ww * pv[:, 2]))[:, None] * np.stack([np.ones(len(pv)), np.zeros(len(pv)), -pv[:, 0] / pv[:, 2]], 1)
    gy = (height / (hh * pv[:, 2]))[:, None] * np.stack([np.zeros(len(pv)), np.ones(len(pv)), -pv[:, 1] / pv[:, 2]], 1)
    return np.stack([np.linalg.norm(gx @ oi, axis=1), np.linalg.norm(gy @ oi, axis=1)], 1)


QUAD_MOVES = [translated(DR.HOVER, (0.15, -0.1, 0.1)),
              rotated_about(translated(DR.HOVER, (0.15, -0.1, 0.1)), (0.5, 0.5, 0.0), (0.2, 0.1, 1.0), 12.0)]


def quad_edge_flags(mm, m, org, dirs):
    """The edge rule of tests/test_gpu_tfdm.py for world rays against the quad under `m`: the float64 brute force in object space,
    over the rays that come within 0.01 of the mesh's bounding box (the others miss every triangle by far more than the rule's
    margin, 1e-3 of a micro-triangle).  Returns (hit, flagged)."""
    m64 = np.asarray(m, np.float32).astype(np.float64)
    li = np.linalg.inv(m64[:, :3])
    oo = (org[:, :3].astype(np.float64) - m64[:, 3]) @ li.T
    od = dirs[:, :3].astype(np.float64) @ li.T
    pts = np.concatenate([mm.A, mm.B, mm.C])
    lo, hi = pts.min(0) - 0.01, pts.max(0) + 0.01
    with np.errstate(all="ignore"):
        a, b = (lo - oo) / od, (hi - oo) / od
    t0, t1 = np.fmin(a, b).max(1), np.fmax(a, b).min(1)
    close = np.nonzero((t1 >= t0) & (t1 > 0))[0]
    hit, flagged = np.zeros(len(org), bool), np.zeros(len(org), bool)
    t64, _, edge, near = T.brute64(mm.A, mm.B, mm.C, oo[close], od[close], org[close, 3].astype(np.float64), dirs[close, 3].astype(np.float64),
                                   clip=(mm.tA, mm.tB, mm.tC, mm.baseTc, mm.prim))
    hit[close], flagged[close] = np.isfinite(t64), edge | near
    return hit, flagged


def test_motion_vector_against_the_tessellated_animated_instance(built_lib, e_mesh):
    """D: the 64 x 64 displaced quad (TwoTriangle, level 0) as instance 0 of a bound set, moved twice with gfx_tfdm_set_move.  T: the
    same quad tessellated as a plain animated instance, moved with gfx_instance_set_transform by the same two transforms.  On the
    pixels where both name the quad and the primary ray is no edge ray (at most 2 % are left out): |mv_D - mv_T| <= bound, with
        delta = 8 E_mesh max(1, t)                  the position allowance of tests/test_gpu_tfdm.py, E_mesh measured in this run
        bound = gain * |curToPrev| * delta + 5e-4   gain: the 2-norm of d(raster) / d(position) of the previous camera at the pixel's
                                                    previous position, |curToPrev| the 2-norm of its linear part; 5e-4 pixel for the
                                                    projection's own rounding (tests/test_displaced_surface_cpu.py)."""
    cams = [DR.camera(0), DR.camera(0), DR.camera(1)]
    sd = DR.Scene(which=(0,), bunny=False)
    st = DR.Scene(tessellated=True, bunny=False)
    quad_inst = 2                                        # floor, lamp, the tessellated quad
    qv, qt = T.quad_mesh()
    mm = T.MicroMesh(qv, qt, T.mips32(sd.heights), sd.quad_params)
    fd, ft = DR.Frames(sd), DR.Frames(st)
    sd.bind()
    worst = 0.0
    placements = [DR.HOVER] + QUAD_MOVES
    for frame in range(3):
        if frame:
            sd.set.move(0, placements[frame])
            sd.set.commit()
            st.ctx.instance_set_transform(quad_inst, placements[frame])
            assert st.ctx.accel_build(handle=st.accel) == st.accel
        f = fd.set_params(frame, cams[frame], cams[frame - 1] if frame else None)
        org, dirs, _ = primary_hits(sd, sd.set, W, H)
        fd.gbuffer()
        ft.set_params(frame, cams[frame], cams[frame - 1] if frame else None)
        ft.gbuffer()
        if not frame:
            continue
        b = frame % 2
        gd, gt = fd.dev.download(), ft.dev.download()
        on_d = gd["gb0_%d" % b]["instSlot"] == (api.GBUFFER_DISPLACED | 0)
        on_t = gt["gb0_%d" % b]["instSlot"] == quad_inst
        hit64, flagged = quad_edge_flags(mm, placements[frame], org, dirs)
        left_out = flagged | (on_d != on_t)
        print("frame %d: the quad owns %.1f %% of the pixels; edge rays %.2f %%, left out in all %.2f %%" %
              (frame, 100 * on_d.mean(), 100 * flagged.mean(), 100 * left_out.mean()))
        assert on_d.mean() > 0.05 and left_out.mean() <= EDGE_CAP
        assert not ((on_d != on_t) & ~flagged).any(), "the two runs disagree on who owns a pixel whose ray is no edge ray"
        keep = on_d & on_t & ~flagged
        pos = gd["gb2_%d" % b]["positionInWorld"][keep].astype(np.float64)
        t = np.linalg.norm(pos - np.array(list(f.camera.position), np.float64), axis=1)
        c2p = sd.set.read_motion()["curToPrev"][0].astype(np.float64).reshape(3, 4)
        prev = pos @ c2p[:, :3].T + c2p[:, 3]
        delta = 8 * e_mesh * np.maximum(1.0, t) * np.linalg.norm(c2p[:, :3], 2)
        bound = projection_gain(f.prevCamera, prev, W, H) * delta[:, None] + 5e-4
        diff = np.abs(gd["gb1_%d" % b][keep].astype(np.float64) - gt["gb1_%d" % b][keep].astype(np.float64))
        ratio = float((diff / bound).max())
        worst = max(worst, ratio)
        print("frame %d: %d pixels, motion vectors up to %.1f pixels, worst |mv_D - mv_T| %.3e pixel = %.3f of its bound (bounds %.2e .. %.2e)" %
              (frame, keep.sum(), np.abs(gt["gb1_%d" % b][keep]).max(), diff.max(), ratio, bound.min(), bound.max()))
        assert np.abs(gt["gb1_%d" % b][keep]).max() > 2.0, "the quad moves on screen"
        assert np.all(diff <= bound)
    print("worst ratio |mv_D - mv_T| / bound = %.3f" % worst)
    sd.unbind()


# ---------------------------------------------------------------- 7, 8. the wall scene
WW, WH = 192, 128
GROUND = S.affine(np.diag([3.0, 3.0, 1.0]), (-0.6, -0.9, 0.02))
WALL = S.affine(S.rotation((1.0, 0.0, 0.0), 75.0) @ np.diag([3.0, 2.0, 2.0]), (-0.6, 2.2, 0.1))
WALL_MOVED = translated(WALL, (0.25, 0.0, 0.0))
WALL_CAMERA = ((0.9, -2.2, 1.6), (0.9, 2.3, 1.0))
WALL_INST = 1


def smooth_map(n=64):
    """One period of a sine product plus a slanted sine, quantised to 8 bits: slopes that hide no part of the wall from the camera."""
    y, x = np.mgrid[0:n, 0:n]
    h = 0.5 + 0.3 * np.sin(2 * np.pi * x / n) * np.cos(2 * np.pi * y / n) + 0.15 * np.sin(2 * np.pi * (2 * x + y) / n)
    return (np.round(np.clip(h, 0, 1) * 255).astype(np.float32) / np.float32(255)).astype(np.float32)


def wall_objects():
    """[(vertices, triangles, heights, params)]: the ground's quad, the wall's quad."""
    qv, qt = T.quad_mesh()
    return [(qv, qt, T.two_sine_map(64), api.tfdm_params(h_scale=0.05)), (qv, qt, smooth_map(64), api.tfdm_params(h_scale=0.04))]


def wall_camera():
    return T.look_at_camera(WW, WH, WALL_CAMERA[0], WALL_CAMERA[1], fov_y_deg=40.0)


class WallScene:
    """A plain floor and lamp; displaced instance 0 the ground (fixed), 1 the wall (moves)."""

    def __init__(self):
        self.ctx = ctx = api.Context(0)
        hs = api.HostScene()
        grey = hs.add_material(DR.lambert((0.7, 0.7, 0.7)))
        light = hs.add_material_traditional((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0.0, emittance=(30.0, 30.0, 30.0))
        mats = [hs.add_material(DR.lambert(c)) for c in ((0.8, 0.3, 0.2), (0.2, 0.6, 0.8))]
        hs.add_instance(hs.add_group([hs.add_geom(*DR.flat_quad(-3.0, -3.0, 5.0, 5.0, 0.0), grey)]), DR.IDENT)
        hs.add_instance(hs.add_group([hs.add_geom(*DR.flat_quad(0.0, -1.0, 1.8, 0.5, 3.5, up=False), light)]), DR.IDENT)
        objects = wall_objects()
        self.slots = [hs.add_geom(v, t, m) for (v, t, _, _), m in zip(objects, mats)]
        hs.upload(ctx)
        self.hs = hs
        self.accel = ctx.accel_build()
        ctx.lights_build_static()
        self.tfdm = [api.Tfdm(ctx, v, t, h, gp) for v, t, h, gp in objects]
        self.set = self.new_set()

    def new_set(self):
        s = api.TfdmSet(self.ctx)
        assert s.add(self.tfdm[0], GROUND, 1) == 0 and s.add(self.tfdm[1], WALL, 2) == WALL_INST
        s.commit()
        return s

    def bind(self, tset=None, restir=False):
        self.ctx.bind_displaced(tset or self.set, self.slots, restir=restir)

    def unbind(self):
        self.ctx.bind_displaced(None)


@pytest.fixture(scope="module")
def wall(built_lib):
    ws = WallScene()
    yield ws
    ws.unbind()


def reprojection(first, second, prev_xfm, cur_xfm, inst=WALL_INST, w=WW, h=WH):
    """first / second: (gbuffer0, gbuffer1, gbuffer2) of frames 1 and 2.  For every frame-2 pixel p of instance `inst`:
    q = floor((p + 0.5) - mv); kept: all eight neighbours of p on the instance, q inside the image and on the instance in frame 1.
    Returns dict(on, kept, q (flat index), resid = |W2O_prev P1(q) - W2O_cur P2(p)|, rho = the largest object-space distance from p to
    its eight neighbours), all over the whole frame, float64."""
    name = api.GBUFFER_DISPLACED | inst
    on2 = (second[0]["instSlot"] == name).reshape(h, w)
    on1 = (first[0]["instSlot"] == name).reshape(h * w)
    obj2 = to_object64(cur_xfm, second[2]["positionInWorld"]).reshape(h, w, 3)
    obj1 = to_object64(prev_xfm, first[2]["positionInWorld"])
    interior = np.zeros((h, w), bool)
    interior[1:-1, 1:-1] = True
    rho = np.zeros((h, w))
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                sh_on = np.roll(on2, (dy, dx), (0, 1))
                sh_obj = np.roll(obj2, (dy, dx), (0, 1))
                interior &= sh_on
                rho = np.maximum(rho, np.linalg.norm(sh_obj - obj2, axis=2))
    ys, xs = np.mgrid[0:h, 0:w]
    mv = second[1].astype(np.float64).reshape(h, w, 2)
    qx, qy = np.floor((xs + 0.5) - mv[..., 0]).astype(np.int64), np.floor((ys + 0.5) - mv[..., 1]).astype(np.int64)
    inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
    q = np.where(inside, qy * w + qx, 0)
    kept = on2 & interior & inside & on1[q]
    resid = np.linalg.norm(obj1[q] - obj2, axis=2)
    return dict(on=on2, kept=kept, q=q, resid=resid, rho=rho, shift=np.hypot(mv[..., 0], mv[..., 1]))


def wall_frames(ws, fr, tset, change, jitter=0):
    """Frame 1 under WALL, then `change`(tset, WALL_INST, WALL_MOVED) + commit and frame 2; the camera stands still.
    Returns ((gb0, gb1, gb2) of frame 1, of frame 2)."""
    cam = wall_camera()
    ws.bind(tset)
    out = []
    for frame in range(2):
        if frame:
            change(tset, WALL_INST, WALL_MOVED)
            tset.commit()
        fr.set_params(frame, cam, cam if frame else None, jitter=jitter)
        fr.gbuffer()
        d = fr.dev.download()
        out.append(tuple(d["gb%d_%d" % (k, frame % 2)].copy() for k in range(3)))
    return out


def test_reprojection_lands_on_the_same_surface_point(wall):
    """192 x 128, camera still, the wall translates by 0.25 (about 9 pixels).  For each kept frame-2 pixel p of the wall, frame 1's pixel
    q = floor((p + 0.5) - mv) shows the wall, and the two pixels' points agree in the wall's object space to rho(p), the largest
    object-space distance from p to its eight neighbours in frame 2 (float64 numpy on the G-buffer positions).  At most 25 % of the
    wall's pixels are left out (a neighbour off the wall, q outside the image or off the wall).  The same statistic over the same two
    frames under set_transform in place of move fails for more than half of its kept pixels."""
    first, second = wall_frames(wall, DR.Frames(wall, WW, WH), wall.new_set(), api.TfdmSet.move)
    r = reprojection(first, second, WALL, WALL_MOVED)
    on, kept = r["on"].sum(), r["kept"].sum()
    ratio = r["resid"][r["kept"]] / r["rho"][r["kept"]]
    print("moved: the wall owns %d pixels (%.1f %%), %.1f %% of them left out; shift %.2f .. %.2f pixels; worst residual / rho = %.3f, median %.3f" %
          (on, 100.0 * on / (WW * WH), 100.0 * (1 - kept / on), r["shift"][r["kept"]].min(), r["shift"][r["kept"]].max(), ratio.max(), np.median(ratio)))
    assert on > 0.15 * WW * WH
    assert r["shift"][r["kept"]].min() >= 6.0, "the wall translates by at least 6 pixels"
    assert 1 - kept / on <= 0.25
    assert np.all(r["resid"][r["kept"]] <= r["rho"][r["kept"]])
    first, second = wall_frames(wall, DR.Frames(wall, WW, WH), wall.new_set(), api.TfdmSet.set_transform)
    t = reprojection(first, second, WALL, WALL_MOVED)
    fails = (t["resid"][t["kept"]] > t["rho"][t["kept"]]).mean()
    print("teleported: %d kept pixels, %.1f %% of them fail" % (t["kept"].sum(), 100 * fails))
    assert t["kept"].sum() > 0.5 * kept and fails > 0.5, "without the motion the statistic fails: the test has teeth"
    wall.unbind()


def test_the_consumers_follow(wall):
    """The frames of the reprojection test with jitter on, under a binding that carries GFX_DISPLACED_RESTIR.
    gfx_restir_copy_taa_flow_to_linear on displaced pixels: current minus previous raster position of the pixel's point (float64: the
    G-buffer position under the camera, its curToPrev image under the previous camera), to 5e-4 pixel.  The temporal pass's neighbour
    of a kept wall pixel -- int(px + 0.5 - mv) in float, C truncation, as INITIAL_AND_TEMPORAL_BIASED computes it -- is q of the
    reprojection test and names the wall in frame 1's gbuffer0."""
    import torch
    ctx, cam = wall.ctx, wall_camera()
    tset = wall.new_set()
    fr = RS.Restir(wall, WW, WH)
    wall.bind(tset, restir=True)
    n = WW * WH
    frames = []
    for frame in range(2):
        if frame:
            tset.move(WALL_INST, WALL_MOVED)
            tset.commit()
        fr.params(frame, cam, cam if frame else None, enableJittering=1)
        fr.launch(api.PASS_SETUP_GBUFFERS, frame % 2, 0)
        d = fr.dev.download()
        frames.append(tuple(d["gb%d_%d" % (k, frame % 2)].copy() for k in range(3)))
        if frame == 0:
            fr.launch(api.PASS_INITIAL_RIS, 0, 0)
            fr.launch(api.PASS_SHADING, 0, 0)
    first, second = frames
    # the flow TAA and the denoiser reproject through
    d_flow = torch.zeros(n * 2, dtype=torch.float32, device="cuda")
    ctx.restir_copy_taa_flow_to_linear(d_flow.data_ptr(), _stream())
    torch.cuda.synchronize()
    flow = d_flow.cpu().numpy().reshape(n, 2).astype(np.float64)
    motion = tset.read_motion()["curToPrev"].astype(np.float64).reshape(-1, 3, 4)
    slot = second[0]["instSlot"]
    disp = (slot != INVALID) & (slot >= api.GBUFFER_DISPLACED)
    m = motion[slot[disp] & 0x7FFFFFFF]
    pos = second[2]["positionInWorld"][disp].astype(np.float64)
    prev = np.einsum("nrc,nc->nr", m[:, :, :3], pos) + m[:, :, 3]
    want = M.project64(cam, pos, WW, WH) - M.project64(cam, prev, WW, WH)
    err = np.abs(flow[disp] - want)
    is_wall = (slot[disp] & 0x7FFFFFFF) == WALL_INST
    print("TAA flow on %d displaced pixels: worst error %.2e pixel; the wall's flow %.2f .. %.2f pixels, the ground's at most %.2e" %
          (disp.sum(), err.max(), np.hypot(*flow[disp][is_wall].T).min(), np.hypot(*flow[disp][is_wall].T).max(), np.abs(flow[disp][~is_wall]).max()))
    assert err.max() <= 5e-4
    assert np.hypot(*flow[disp][is_wall].T).min() >= 6.0 and np.abs(flow[disp][~is_wall]).max() <= 5e-4
    # the temporal pass
    r = reprojection(first, second, WALL, WALL_MOVED)
    kept = r["kept"].reshape(n)
    assert 1 - kept.sum() / r["on"].sum() <= 0.25
    xs, ys = (np.arange(n) % WW).astype(np.float32), (np.arange(n) // WW).astype(np.float32)
    mv = second[1]
    nbx = ((xs + np.float32(0.5)) - mv[:, 0]).astype(np.int32)           # float arithmetic, truncation toward zero
    nby = ((ys + np.float32(0.5)) - mv[:, 1]).astype(np.int32)
    assert np.all((nbx[kept] >= 0) & (nbx[kept] < WW) & (nby[kept] >= 0) & (nby[kept] < WH))
    nb = nby.astype(np.int64) * WW + nbx
    assert np.array_equal(nb[kept], r["q"].reshape(n)[kept]), "the kernel's neighbour is q"
    assert np.all(first[0]["instSlot"][nb[kept]] == (api.GBUFFER_DISPLACED | WALL_INST))
    assert np.all(r["resid"].reshape(n)[kept] <= r["rho"].reshape(n)[kept])
    fr.launch(api.PASS_INITIAL_TEMPORAL_BIASED, 1, 0)
    out = fr.dev.download()
    assert np.isfinite(out["res_1"]).all() and np.isfinite(out["info_1"]).all()
    assert np.mean(out["info_1"][kept, 0] > 0) > 0.5, "the wall's pixels hold a sample after the temporal pass"
    wall.unbind()


# ---------------------------------------------------------------- 9. refusals
def test_refusals_each_with_its_message(built_lib):
    sc = DR.Scene(which=(0, 1), bunny=False)
    ctx, tset = sc.ctx, sc.set
    with pytest.raises(api.GfxError, match="gfx_tfdm_set_move: no such instance"):
        tset.move(2, DR.HOVER)
    assert tset.L.gfx_tfdm_set_move(tset.h, C.c_uint32(0), None) != 0
    assert "gfx_tfdm_set_move: null transform" in ctx.L.gfx_last_error(ctx.h).decode()
    with pytest.raises(api.GfxError, match="12 floats"):
        tset.move(0, np.zeros(7, np.float32))
    # the refused calls changed nothing: the set is still committed
    tset.read_motion()
    # an uncommitted move: the query, the tables and a launch
    tset.move(0, MOVED0)
    fr = DR.Frames(sc)
    fr.set_params(0, DR.camera(0))
    sc.bind()
    with pytest.raises(api.GfxError, match="not committed"):
        primary_hits(sc, tset, W, H)
    with pytest.raises(api.GfxError, match="not committed"):
        fr.gbuffer()
    with pytest.raises(api.GfxError, match="gfx_tfdm_set_read_motion.*not committed"):
        tset.read_motion()
    tset.move(1, MOVED1)
    tset.commit()
    table, motion = tset.read(), tset.read_motion()
    fr.gbuffer()
    before = fr.dev.download()
    # a wrong size
    buf = np.zeros(3, api.TFDM_MOTION_DTYPE)
    for nbytes in (0, 48, 2 * 48 + 4, 3 * 48, 2 * 192):
        assert tset.L.gfx_tfdm_set_read_motion(ctx.h, tset.h, buf.ctypes.data_as(C.c_void_p), C.c_size_t(nbytes)) != 0
        assert "exactly 48 bytes per instance" in ctx.L.gfx_last_error(ctx.h).decode()
    assert tset.L.gfx_tfdm_set_read_motion(ctx.h, tset.h, None, C.c_size_t(2 * 48)) != 0
    # a move that is not finite: the commit fails, nothing is swapped in, and the set stays uncommitted until it is repaired
    bad = MOVED1.copy()
    bad[2, 3] = np.inf
    tset.move(1, bad)
    with pytest.raises(api.GfxError, match="gfx_tfdm_set_commit: instance 1: .*not finite"):
        tset.commit()
    for refused in (tset.read, tset.read_motion, fr.gbuffer):
        with pytest.raises(api.GfxError, match="not committed"):
            refused()
    tset.move(1, MOVED1)                                  # previous <- the transform that is not finite
    with pytest.raises(api.GfxError, match="gfx_tfdm_set_commit: instance 1: .*previous transform is not finite"):
        tset.commit()
    # repaired to the pair it had (teleport to where it was, move to where it is): both tables and the picture are the ones from before
    tset.set_transform(1, DR.GENERAL)
    tset.move(1, MOVED1)
    tset.commit()
    util.assert_same_bits("record table after the repair", tset.read(), table)
    util.assert_same_bits("motion table after the repair", tset.read_motion(), motion)
    fr.set_params(0, DR.camera(0))
    fr.gbuffer()
    after = fr.dev.download()
    for k in ("gb0_0", "gb1_0", "gb2_0", "gb3_0"):
        util.assert_same_bits("%s after the repair" % k, after[k], before[k])
    sc.unbind()
