"""-m gpu: displaced instances in the G-buffer pass and the baseline path tracer (gfx_scene_bind_displaced).

The scene (z up): a plain floor, a plain bunny and an emissive rectangle above them; three displaced instances -- the unit quad in
TwoTriangle mode hovering over the floor, the same quad rotated and scaled (1.5, 0.75, 2), the bunny base mesh in Box mode at level 1,
mirrored.  What each case is held against:
  * an empty bound set: the unbound passes, bit for bit;
  * the G-buffer of a displaced pixel: the host compilation of csrc/tfdm/displaced_surface.hip.h (tests/displaced_host.cpp) fed the
    gfx_trace_scene hit of the ray gfx_restir_primary_rays reports for the pixel; every other pixel: the unbound pass;
  * bands, a second run, pt_overlap off: the same bytes;
  * the integral: the same quad tessellated into the BVH8 and rendered by the existing tracer (whose parity with the oracle the
    existing tests establish), by the statistic written at the test."""
import ctypes as C
import os

import numpy as np
import pytest

from gfxexp_amd import api
from tests import displaced_host as D
from tests import scene_trace_host as S
from tests import tfdm_host as T
from tests import util

pytestmark = pytest.mark.gpu
INVALID = api.GFX_INVALID_SLOT
W, H = 96, 64
LAMBERT = 0
RX90 = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], np.float64)      # the y-up bunny onto z-up


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def lambert(rgb, tex=0):
    m = api.GfxMaterial()
    m.bsdfType = LAMBERT
    m.a = (C.c_float * 3)(*rgb)
    m.texA = tex
    return m


def flat_quad(x0, y0, x1, y1, z, up=True):
    v = np.zeros(4, api.VERTEX_DTYPE)
    v["position"] = [(x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)]
    v["normal"] = (0, 0, 1 if up else -1)
    v["texCoord0Dir"] = (1, 0, 0)
    v["texCoord"] = [(0, 0), (1, 0), (1, 1), (0, 1)]
    t = np.array([[0, 1, 2], [0, 2, 3]] if up else [[0, 2, 1], [0, 3, 2]], np.uint32)
    return v, t


IDENT = S.affine(np.eye(3), (0, 0, 0))
HOVER = S.affine(np.eye(3), (0.0, 0.0, 0.4))
GENERAL = S.affine(S.rotation((0.3, 1.0, 0.2), 35.0) @ np.diag([1.5, 0.75, 2.0]), (1.7, 0.9, 0.45))
MIRRORED = S.affine(RX90 @ np.diag([-0.012, 0.012, 0.012]), (0.0, 1.9, 0.0))
CAMERAS = [((0.9, -1.9, 2.1), (0.9, 0.9, 0.3)), ((1.1, -1.8, 2.0), (0.9, 0.9, 0.3))]


def camera(k, w=W, h=H):
    return T.look_at_camera(w, h, CAMERAS[k][0], CAMERAS[k][1], fov_y_deg=40.0)


class Scene:
    """One context: the plain scene in the BVH8, the displaced objects, their ungrouped shading geometry.  which: the displaced
    instances taken along (indices into the list above); tessellated: the hovering quad as micro-triangles in the BVH8 instead;
    texture: the bunny's displaced instance gets a textured material (and a plain twin of it stands in the BVH8 with `plain_twin`)."""

    def __init__(self, which=(0, 1, 2), tessellated=False, bunny=True, texture=None, plain_twin=False):
        self.ctx = ctx = api.Context(0)
        hs = api.HostScene()
        grey = hs.add_material(lambert((0.7, 0.7, 0.7)))
        light = hs.add_material_traditional((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0.0, emittance=(30.0, 30.0, 30.0))
        mats = [hs.add_material(lambert(c)) for c in ((0.8, 0.3, 0.2), (0.2, 0.6, 0.8), (0.3, 0.8, 0.3))]
        self.tex = hs.load_texture(texture) if texture is not None else 0
        if texture is not None:
            mats[2] = hs.add_material(lambert((1.0, 1.0, 1.0), self.tex))
        self.mats = mats
        floor = hs.add_geom(*flat_quad(-2.0, -1.5, 4.0, 3.5, 0.0), grey)
        lamp = hs.add_geom(*flat_quad(0.0, 0.0, 1.5, 1.5, 3.0, up=False), light)
        hs.add_instance(hs.add_group([floor]), IDENT)
        hs.add_instance(hs.add_group([lamp]), IDENT)
        self.floor_inst = 0
        if bunny:
            g = hs.load_obj(os.path.join(T.ASSETS, "stanford_bunny_309_faces.obj"))
            hs.add_instance(g, S.affine(RX90 * 0.006, (-0.9, 0.7, 0.0)))
        qv, qt = T.quad_mesh()
        bv, bt = T.obj_mesh("stanford_bunny_309_faces.obj")
        ext = float((bv["position"].max(0) - bv["position"].min(0)).max())
        self.heights = T.two_sine_map(64)
        self.quad_params = api.tfdm_params(h_scale=0.1)
        objects = [(qv, qt, self.quad_params), (bv, bt, api.tfdm_params(h_scale=0.02 * ext, local_intersection=api.TFDM_BOX, target_mip_level=1))]
        layout = [(0, HOVER), (0, GENERAL), (1, MIRRORED)]
        self.members = [(layout[k][0], layout[k][1], mats[k]) for k in which]
        if tessellated:
            mv, mt = tessellated_quad_mesh(qv, qt, self.heights, self.quad_params)
            hs.add_instance(hs.add_group([hs.add_geom(mv, mt, mats[0])]), HOVER)
            self.members = []
        if plain_twin:
            hs.add_instance(hs.add_group([hs.add_geom(bv, bt, mats[2])]), MIRRORED)
            self.members = []
        # the shading geometry of the displaced instances: in NO group, so not in the BVH8
        self.meshes = [(objects[o][0], objects[o][1]) for o, _, _ in self.members]
        self.slots = [hs.add_geom(objects[o][0], objects[o][1], m) for o, _, m in self.members]
        hs.upload(ctx)
        self.hs = hs
        self.accel = ctx.accel_build()
        ctx.lights_build_static()
        self.tfdm = {}
        self.set = None
        if self.members or not (tessellated or plain_twin):
            for o in sorted(set(m[0] for m in self.members)):
                self.tfdm[o] = api.Tfdm(ctx, objects[o][0], objects[o][1], self.heights, objects[o][2])
            self.set = api.TfdmSet(ctx)
            for k, (o, m, _) in enumerate(self.members):
                assert self.set.add(self.tfdm[o], m, 50 + k) == k
            self.set.commit()

    def bind(self):
        self.ctx.bind_displaced(self.set, self.slots)

    def unbind(self):
        self.ctx.bind_displaced(None)


def tessellated_quad_mesh(qv, qt, heights, gp):
    """The displaced quad as its micro-triangles (tests/tfdm_host.py MicroMesh), each with its face normal as its vertex normals and
    its own texture coordinates (the quad's are its x, y): the same radiometric scene as the displaced instance."""
    v, t = T.MicroMesh(qv, qt, T.mips32(heights), gp).float32_mesh()
    p = v["position"].astype(np.float64).reshape(-1, 3, 3)
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    assert np.all(n[:, 2] > 0)
    v["normal"] = np.repeat(n, 3, axis=0)
    v["texCoord"] = v["position"][:, :2]
    return v, t


class Frames:
    """Per-pixel buffers on the device and the two passes of a path-traced frame."""

    def __init__(self, scene, w=W, h=H, env=None, seed=util.PIXEL_RNG_SEED):
        self.scene, self.w, self.h, self.env = scene, w, h, env
        pb = util.PixelBuffers(w, h, seed)
        if env is not None:
            pb.set_env(*env)
        self.dev = util.DeviceBuffers(pb)
        self.s = self.dev.static_params()

    def set_params(self, frame, cam, prev_cam=None, jitter=0):
        kw = dict(frameIndex=frame, bufferIndex=frame % 2, resetFlowBuffer=int(frame == 0), numAccumFrames=frame, enableJittering=jitter,
                  enableEnvLight=int(self.env is not None))
        f = util.frame_params(api.GfxRestirFrameParams, api.GfxCamera, self.w, self.h, cam, prev_cam, travHandle=self.scene.accel, **kw)
        ctx = self.scene.ctx
        ctx.lights_build_instances(_stream())
        ctx.restir_set_params(self.s, f, 0, 0, _stream())
        return f

    def gbuffer(self, bands=((0, 0),)):
        for rb, re in bands:
            self.scene.ctx.pt_launch(api.PT_SETUP_GBUFFERS, self.w, self.h, 0, rb, re, _stream())

    def trace(self, max_len, bands=((0, 0),)):
        for rb, re in bands:
            self.scene.ctx.pt_launch(api.PT_PATH_TRACE_BASELINE, self.w, self.h, max_len, rb, re, _stream())

    def render(self, frames, max_len, jitter=0, cams=None, bands=((0, 0),)):
        for f in range(frames):
            cam = cams[f] if cams else camera(0, self.w, self.h)
            self.set_params(f, cam, cams[f - 1] if cams and f else None, jitter)
            self.gbuffer(bands)
            self.trace(max_len, bands)
        return self.dev.download()

    def copy_state_from(self, other, keys=("rng", "albedo", "normal", "beauty")):
        for k in keys:
            self.dev.t[k].copy_(other.dev.t[k])


KEYS = ("rng", "beauty", "gb0_0", "gb0_1", "gb1_0", "gb1_1", "gb2_0", "gb2_1", "gb3_0", "gb3_1", "albedo", "normal")


def assert_same_buffers(what, a, b, keys=KEYS):
    for k in keys:
        util.assert_same_bits("%s: %s" % (what, k), a[k], b[k])


@pytest.fixture(scope="module")
def full(built_lib):
    return Scene()


@pytest.fixture(scope="module")
def dhost(built_lib, tmp_path_factory):
    return D.DisplacedHost(tmp_path_factory.mktemp("displaced_host"))


# ---------------------------------------------------------------- 1. an empty set is no set
@pytest.mark.parametrize("jitter", [1, 0])
def test_an_empty_bound_set_renders_what_no_binding_renders(built_lib, jitter):
    sc = Scene(which=())
    env = (api.env_make_sky(64, 32), 64, 32)
    cams = [camera(0), camera(1)]
    want = Frames(sc, env=env).render(2, 5, jitter, cams)
    assert len(sc.set) == 0
    sc.bind()
    got = Frames(sc, env=env).render(2, 5, jitter, cams)
    assert_same_buffers("empty set bound", got, want)
    sc.ctx.tunable_set("fuse_passes", 2)             # asked for, and overruled by the binding: the same bytes again
    got = Frames(sc, env=env).render(2, 5, jitter, cams)
    sc.ctx.tunable_set("fuse_passes", 0)
    assert_same_buffers("empty set bound, fuse_passes 2 requested", got, want)
    sc.unbind()
    assert np.isfinite(want["beauty"]).all() and want["beauty"][:, :3].mean() > 1e-3
    assert np.mean(want["gb0_1"]["instSlot"] == INVALID) > 0.02, "some pixels see the environment"


# ---------------------------------------------------------------- 2. the G-buffer, every field
def _words(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(len(a), -1)


def test_gbuffer_of_every_pixel_bit_for_bit(full, dhost):
    import torch
    sc, ctx = full, full.ctx
    table = sc.set.read()
    cams = [camera(0), camera(1)]
    bound, plain = Frames(sc), Frames(sc)
    n = W * H
    d_org, d_dir = torch.zeros(n * 4, dtype=torch.float32, device="cuda"), torch.zeros(n * 4, dtype=torch.float32, device="cuda")
    d_hit = torch.zeros(n * 8, dtype=torch.int32, device="cuda")
    xy = np.stack([np.arange(n) % W, np.arange(n) // W], 1)
    for frame in range(2):
        prev = {k: bound.dev.download()[k].copy() for k in ("albedo", "normal")}
        # the reference for plain pixels, misses and the RNG: the same frame from the same state without a binding
        plain.copy_state_from(bound)
        sc.unbind()
        plain.set_params(frame, cams[frame], cams[frame - 1] if frame else None, jitter=1)
        plain.gbuffer()
        want = plain.dev.download()
        sc.bind()
        f = bound.set_params(frame, cams[frame], cams[frame - 1] if frame else None, jitter=1)
        rng_before = bound.dev.download()["rng"].copy()
        ctx.restir_primary_rays(W, H, d_org.data_ptr(), d_dir.data_ptr(), _stream())
        api.trace_scene(ctx, sc.accel, sc.set, api.TRACE_CLOSEST, d_org.data_ptr(), d_dir.data_ptr(), n, d_hit.data_ptr(), stream=_stream())
        torch.cuda.synchronize()
        util.assert_same_bits("gfx_restir_primary_rays leaves the RNG alone", bound.dev.download()["rng"], rng_before)
        org, dirs = d_org.cpu().numpy().reshape(n, 4), d_dir.cpu().numpy().reshape(n, 4)
        hits = d_hit.cpu().numpy().view(api.SCENE_HIT_DTYPE).reshape(n)
        bound.gbuffer()
        got = bound.dev.download()
        b = frame % 2
        util.assert_same_bits("frame %d: RNG after the pass" % frame, got["rng"], want["rng"])
        where = hits["where"]
        disp = (where != INVALID) & (where != api.SCENE_PLAIN)
        rest = ~disp
        for k in ("gb0", "gb1", "gb2", "gb3"):
            util.assert_same_bits("frame %d: %s of plain and empty pixels" % (frame, k), _words(got["%s_%d" % (k, b)])[rest], _words(want["%s_%d" % (k, b)])[rest])
        for k in ("albedo", "normal"):
            util.assert_same_bits("frame %d: %s accumulation of plain and empty pixels" % (frame, k), got[k][rest], want[k][rest])
        # displaced pixels: the host compilation of the header, fed the hit
        idx = np.nonzero(disp)[0]
        inst = where[idx] >> 1
        bv = np.zeros((len(idx), 15), np.float32)
        for k in range(len(sc.members)):
            m = inst == k
            bv[m] = D.base_verts_of(sc.meshes[k][0], sc.meshes[k][1], hits["index"][idx][m])
        geom = np.array(sc.slots, np.uint32)[inst]
        mat = np.array([m for _, _, m in sc.members], np.uint32)[inst]
        ref = dhost.resolve(table, hits[idx], org[idx], dirs[idx], bv, geom, mat, xy[idx], f.prevCamera, W, H, reset_flow=frame == 0)
        for k in ("g0", "g1", "g2", "g3"):
            util.assert_same_bits("frame %d: gbuffer%s of displaced pixels" % (frame, k[1]), _words(got["gb%s_%d" % (k[1], b)])[idx], _words(ref[k]))
        assert np.all(_words(got["gb0_%d" % b])[idx, 0] == (api.GBUFFER_DISPLACED | inst))
        cw = np.float32(1.0) / np.float32(1 + frame)
        colour = np.array([(0.8, 0.3, 0.2), (0.2, 0.6, 0.8), (0.3, 0.8, 0.3)], np.float32)[inst]      # Lambert: the reflectance itself
        for key, cur in (("albedo", colour), ("normal", ref["points"][:, 3:6])):
            p = prev[key][idx, :3] if frame else np.zeros((len(idx), 3), np.float32)
            acc = (np.float32(1) - cw) * p + cw * cur
            util.assert_same_bits("frame %d: %s accumulation of displaced pixels" % (frame, key), got[key][idx, :3], acc.astype(np.float32))
            assert np.all(got[key][idx, 3] == 1.0)
        if frame:
            assert np.abs(ref["g1"]).max() > 0.5, "the camera moved: displaced pixels carry a flow"
        shares = [np.mean(where == api.SCENE_PLAIN)] + [np.mean(disp & (where >> 1 == k)) for k in range(3)]
        print("frame %d: plain %.1f %%, instances %s %%, empty %.1f %%" % (frame, 100 * shares[0], ["%.1f" % (100 * s) for s in shares[1:]], 100 * np.mean(where == INVALID)))
        assert all(s >= 0.02 for s in shares), "every instance and the plain geometry own 2 %% of the pixels: %s" % shares
    # the output-chain copies on a frame with displaced pixels: emissive is zero there, depth is the camera distance of gbuffer2
    d_em, d_depth = torch.full((n,), 7, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.float32, device="cuda")
    d_flow = torch.zeros(n * 2, dtype=torch.float32, device="cuda")
    ctx.restir_copy_emissive_to_linear(d_em.data_ptr(), _stream())
    ctx.restir_copy_depth_to_linear(d_depth.data_ptr(), _stream())
    ctx.restir_copy_taa_flow_to_linear(d_flow.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert np.all(d_em.cpu().numpy()[idx] == 0)
    dist = np.linalg.norm(ref["points"][:, :3].astype(np.float64) - np.array(CAMERAS[1][0]), axis=1)
    assert np.abs(d_depth.cpu().numpy()[idx] - dist).max() < 1e-5 * dist.max()
    assert np.isfinite(d_flow.cpu().numpy()).all()
    sc.unbind()


# ---------------------------------------------------------------- 3. bands, repeatability, overlap
def test_bands_a_second_run_and_no_overlap_give_the_same_bytes(full):
    sc = full
    sc.bind()
    cams = [camera(0), camera(1)]
    want = Frames(sc).render(2, 5, 1, cams)
    assert_same_buffers("two row bands", Frames(sc).render(2, 5, 1, cams, bands=((0, 24), (24, 64))), want)
    assert_same_buffers("a second run", Frames(sc).render(2, 5, 1, cams), want)
    sc.ctx.tunable_set("pt_overlap", 0)
    got = Frames(sc).render(2, 5, 1, cams)
    sc.ctx.tunable_set("pt_overlap", 1)
    assert_same_buffers("pt_overlap off", got, want)
    sc.unbind()
    disp = (want["gb0_1"]["instSlot"] != INVALID) & (want["gb0_1"]["instSlot"] >= api.GBUFFER_DISPLACED)
    rgb = want["beauty"][:, :3]
    assert np.isfinite(rgb).all() and rgb[disp].mean() > 1e-3, "displaced pixels receive light"


# ---------------------------------------------------------------- 4. the integral, against the tessellation
def _tile_means(beauty, w, h):
    return beauty.reshape(h // 8, 8, w // 8, 8, 4)[..., :3].mean(axis=(1, 3)).reshape(-1, 3).astype(np.float64)


def test_the_integral_against_the_tessellated_quad(built_lib):
    """64 x 48, max_len 4, 64 accumulated frames.  T1, T2: the quad tessellated into the BVH8 under two RNG seedings, by the existing
    tracer; D: the bound set.  Over the 8 x 8 tile means N = rms((T2 - T1) / (T1 + 0.01)) and the test asserts
    rms((D - T1) / (T1 + 0.01)) <= 2 N: D - T1 and T2 - T1 have the same variance when D estimates the same integrand."""
    w, h, frames = 64, 48, 64
    cam = [camera(0, w, h)] * frames
    tess = Scene(tessellated=True, bunny=False)
    t1 = Frames(tess, w, h, seed=1001).render(frames, 4, 1, cam)
    t2 = Frames(tess, w, h, seed=2002).render(frames, 4, 1, cam)
    sc = Scene(which=(0,), bunny=False)
    u = Frames(sc, w, h, seed=3003).render(frames, 4, 1, cam)
    sc.bind()
    d = Frames(sc, w, h, seed=3003).render(frames, 4, 1, cam)
    sc.unbind()
    T1, T2, Dm, U = (_tile_means(x["beauty"], w, h) for x in (t1, t2, d, u))
    rms = lambda x: float(np.sqrt(np.mean(x * x)))
    N = rms((T2 - T1) / (T1 + 0.01))
    R = rms((Dm - T1) / (T1 + 0.01))
    print("integral: N = %.4f, rms((D - T1) / (T1 + 0.01)) = %.4f, ratio %.2f; unbound against T1: %.4f" % (N, R, R / N, rms((U - T1) / (T1 + 0.01))))
    quad_share = np.mean(d["gb0_1"]["instSlot"] == api.GBUFFER_DISPLACED)
    assert quad_share > 0.05, "the quad is in the picture"
    assert R <= 2 * N
    # the shadow: floor tiles under the hovering quad (all floor in both pictures, a quarter darker in T1 than without the quad)
    floor_t = (t1["gb0_1"]["instSlot"] == tess.floor_inst).reshape(h // 8, 8, w // 8, 8).all(axis=(1, 3)).reshape(-1)
    floor_d = (d["gb0_1"]["instSlot"] == sc.floor_inst).reshape(h // 8, 8, w // 8, 8).all(axis=(1, 3)).reshape(-1)
    lum = lambda x: x.mean(axis=1)
    shadow = floor_t & floor_d & (lum(T1) < 0.75 * lum(U))
    print("shadow tiles: %d; mean luminance unbound %.4f, tessellated %.4f, displaced %.4f" %
          (shadow.sum(), lum(U)[shadow].mean() if shadow.any() else 0, lum(T1)[shadow].mean() if shadow.any() else 0, lum(Dm)[shadow].mean() if shadow.any() else 0))
    assert shadow.sum() >= 1, "the camera sees floor in the quad's shadow"
    assert np.all(lum(U)[shadow] - lum(Dm)[shadow] >= 0.5 * (lum(U)[shadow] - lum(T1)[shadow]))


# ---------------------------------------------------------------- 5. a textured displaced material
def test_a_textured_displaced_material(built_lib, dhost, tmp_path):
    """The bunny's displaced instance under a Lambert material whose reflectance is a PNG map.  The albedo of a Lambert surface is the
    reflectance itself, tex2DLod(map, texCoord, 0), so the expected accumulation of frame 0 is gfx_texture_sample at the texture
    coordinate the host compilation of the header gives for the pixel's hit: the library's own sampler at bit-equal coordinates, so
    the comparison is exact (the plain pass reads the same sampler for a plain instance of the geometry at that (primIndex, bc))."""
    import torch
    from tests import image_fixtures as F
    sc = Scene(which=(2,), texture=F.write_file(tmp_path, "rgba8.png"))
    ctx = sc.ctx
    tex = sc.tex
    n = W * H
    fr = Frames(sc)
    sc.bind()
    f = fr.set_params(0, camera(0))
    d_org, d_dir = torch.zeros(n * 4, dtype=torch.float32, device="cuda"), torch.zeros(n * 4, dtype=torch.float32, device="cuda")
    d_hit = torch.zeros(n * 8, dtype=torch.int32, device="cuda")
    ctx.restir_primary_rays(W, H, d_org.data_ptr(), d_dir.data_ptr(), _stream())
    api.trace_scene(ctx, sc.accel, sc.set, api.TRACE_CLOSEST, d_org.data_ptr(), d_dir.data_ptr(), n, d_hit.data_ptr(), stream=_stream())
    fr.gbuffer()
    got = fr.dev.download()
    sc.unbind()
    hits = d_hit.cpu().numpy().view(api.SCENE_HIT_DTYPE).reshape(n)
    idx = np.nonzero((hits["where"] != INVALID) & (hits["where"] != api.SCENE_PLAIN))[0]
    assert len(idx) > 0.03 * n
    xy = np.stack([np.arange(n) % W, np.arange(n) // W], 1)
    bv = D.base_verts_of(sc.meshes[0][0], sc.meshes[0][1], hits["index"][idx])
    ref = dhost.resolve(sc.set.read(), hits[idx], d_org.cpu().numpy().reshape(n, 4)[idx], d_dir.cpu().numpy().reshape(n, 4)[idx], bv,
                        np.full(len(idx), sc.slots[0], np.uint32), np.full(len(idx), sc.mats[2], np.uint32), xy[idx], f.prevCamera, W, H, reset_flow=True)
    util.assert_same_bits("gbuffer3 of the textured pixels", _words(got["gb3_0"])[idx], _words(ref["g3"]))
    d_uv = torch.from_numpy(np.ascontiguousarray(ref["points"][:, 9:11])).cuda()
    d_out = torch.zeros((len(idx), 4), dtype=torch.float32, device="cuda")
    ctx.texture_sample(tex, d_uv.data_ptr(), len(idx), d_out.data_ptr(), False, _stream())
    torch.cuda.synchronize()
    want = d_out.cpu().numpy()[:, :3]
    util.assert_same_bits("albedo of the textured displaced pixels", got["albedo"][idx, :3], want)
    assert len(np.unique(want.view(np.uint32), axis=0)) > 20, "the map varies over the instance"


# ---------------------------------------------------------------- 6. refusals
def test_refusals_name_their_cause(full):
    sc, ctx = full, full.ctx
    sc.unbind()
    with pytest.raises(api.GfxError, match="3 instances"):
        ctx.bind_displaced(sc.set, sc.slots[:2])
    with pytest.raises(api.GfxError, match="unknown geometry slot"):
        ctx.bind_displaced(sc.set, [sc.slots[0], sc.slots[1], 9999])
    with pytest.raises(api.GfxError, match="triangle count"):
        ctx.bind_displaced(sc.set, [sc.slots[0], sc.slots[2], sc.slots[2]])
    with pytest.raises(api.GfxError, match="emittance"):
        ctx.bind_displaced(sc.set, [sc.slots[0], 1, sc.slots[2]])            # geometry 1: the lamp, two triangles like the quad
    fr = Frames(sc)
    fr.set_params(0, camera(0))
    sc.bind()
    sc.set.set_transform(0, HOVER)
    for launch in (fr.gbuffer, lambda: fr.trace(3)):
        with pytest.raises(api.GfxError, match="not committed"):
            launch()
    sc.set.commit()
    fr.gbuffer()
    regir = util.RegirBuffers(sc.hs.bounds())
    ctx.regir_set_params(regir.device_params())
    for what, launch in (("ReSTIR", lambda: ctx.restir_launch(api.PASS_INITIAL_RIS, W, H, _stream())),
                         ("ReSTIR", lambda: ctx.restir_launch(api.PASS_SHADING, W, H, _stream())),
                         ("ReGIR", lambda: ctx.pt_launch(api.PT_REGIR_BUILD_CELLS, W, H, 3, 0, 0, _stream())),
                         ("NRC", lambda: ctx.pt_launch(api.PT_NRC_PREPROCESS, W, H, 3, 0, 0, _stream()))):
        with pytest.raises(api.GfxError, match="displaced instance set is bound"):
            launch()
    sc.unbind()
    fr.gbuffer()                                     # no displaced ids are left in the G-buffers the passes below read
    ctx.restir_launch(api.PASS_INITIAL_RIS, W, H, _stream())
    ctx.restir_launch(api.PASS_SHADING, W, H, _stream())
    ctx.pt_launch(api.PT_REGIR_BUILD_CELLS, W, H, 3, 0, 0, _stream())
    import torch
    torch.cuda.synchronize()
    with pytest.raises(api.GfxError, match="gfx_nrc_set_render_params"):     # past the binding's refusal: NRC wants its own parameters
        ctx.pt_launch(api.PT_NRC_PREPROCESS, W, H, 3, 0, 0, _stream())
    assert np.isfinite(fr.dev.download()["beauty"]).all()
