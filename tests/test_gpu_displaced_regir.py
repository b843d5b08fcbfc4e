"""-m gpu: the ReGIR passes of gfx_pt_launch over a bound set of displaced instances (GFX_DISPLACED_REGIR), the
inspection entry gfx_pt_last_nee_rays and gfx_tfdm_set_bounds.

Scenes, frame size, Frames, far_twin, KScene and the tile statistics are those of tests/test_gpu_displaced_render.py,
test_gpu_displaced_restir.py and test_gpu_displaced_kinds.py, taken by import; the ReGIR state is util.RegirBuffers.  S is the scene's
set, S' the same objects 1400 units away (it occludes nothing and a G-buffer written under S is valid under it).  The grid of every
case covers the scene's bounds joined with S's.  What each case is held against is written at the case."""
import re

import numpy as np
import pytest

from gfxexp_amd import api
from tests import displaced_kinds_host as K
from tests import displaced_regir_host as G
from tests import test_gpu_displaced_kinds as DK
from tests import test_gpu_displaced_render as DR
from tests import test_gpu_displaced_restir as RR
from tests import util

pytestmark = pytest.mark.gpu
W, H = DR.W, DR.H
CAP = 2 * W * H
DIMS = (8, 4, 8)
REGIR_KEYS = ("regir_res_0", "regir_res_1", "regir_info_0", "regir_info_1", "regir_accesses", "regir_last_access", "regir_active_0", "regir_active_1", "regir_rngs")
KEYS = DR.KEYS + REGIR_KEYS
TODAYS_REFUSAL = "only the G-buffer pass and the baseline path tracer render displaced instances; ReGIR / NRC pass %d is refused"


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def grid_bounds(hs, tset):
    """lo + hi (six floats): the scene's bounds joined with the set's (the displaced members are not in the BVH8)."""
    b = hs.bounds()
    lo, hi = tset.bounds()
    return np.concatenate([np.minimum(b[:3], lo), np.maximum(b[3:], hi)]).astype(np.float32)


class Regir(DR.Frames):
    """The ReGIR frame loop (regir_main.cpp:2021-2066) over the buffers of DR.Frames and a grid of its own."""

    def __init__(self, scene, bounds, w=W, h=H, env=None, seed=util.PIXEL_RNG_SEED, dims=DIMS, randomize=1):
        super().__init__(scene, w, h, env, seed)
        self.rb = util.RegirBuffers(bounds, dims, randomize=randomize)
        self.g = self.rb.device_params()

    def params(self, frame, cam, prev_cam=None, **kw):
        base = dict(frameIndex=frame, bufferIndex=frame % 2, resetFlowBuffer=int(frame == 0), numAccumFrames=0, enableEnvLight=int(self.env is not None))
        base.update(kw)
        f = util.frame_params(api.GfxRestirFrameParams, api.GfxCamera, self.w, self.h, cam, prev_cam, travHandle=self.scene.accel, **base)
        ctx = self.scene.ctx
        ctx.lights_build_instances(_stream())
        ctx.restir_set_params(self.s, f, 0, 0, _stream())
        ctx.regir_set_params(self.g)
        return f

    def launch(self, pass_id, max_len=0, bands=((0, 0),)):
        for rb, re_ in bands:
            self.scene.ctx.pt_launch(pass_id, self.w, self.h, max_len, rb, re_, _stream())

    def first_vertex_state(self, cam, frame=0):
        """Frame parameters, the G-buffer pass and the cell build of one frame: what a tracer launch at path length 1 starts from."""
        self.params(frame, cam)
        self.launch(api.PT_SETUP_GBUFFERS)
        self.launch(api.PT_REGIR_BUILD_CELLS)

    def frames(self, n, max_len, cams, bands=((0, 0),), accumulate=False, jitter=0):
        for f in range(n):
            self.params(f, cams[f], cams[f - 1] if f else None, numAccumFrames=f if accumulate else 0, enableJittering=jitter)
            self.launch(api.PT_SETUP_GBUFFERS, 0, bands)
            self.launch(api.PT_REGIR_BUILD_CELLS_TEMPORAL if f else api.PT_REGIR_BUILD_CELLS)
            self.launch(api.PT_PATH_TRACE_REGIR, max_len, bands)
            self.launch(api.PT_REGIR_UPDATE_LAST_ACCESS)
        return self.download()

    def download(self):
        out = self.dev.download()
        out.update(self.rb.download())
        return out

    def snapshot(self):
        import torch
        torch.cuda.synchronize()
        return [{k: t.clone() for k, t in d.items()} for d in (self.dev.t, self.rb.t)]

    def restore(self, snap):
        for d, s in zip((self.dev.t, self.rb.t), snap):
            for k, t in s.items():
                d[k].copy_(t)


class NeeQueue:
    """gfx_pt_last_nee_rays into device buffers of `capacity` entries (the attributes RR.any_hit reads, and the owners)."""

    def __init__(self, ctx, capacity=CAP):
        import torch
        self.d_org = torch.zeros(capacity * 4, dtype=torch.float32, device="cuda")
        self.d_dir = torch.zeros(capacity * 4, dtype=torch.float32, device="cuda")
        self.d_occ = torch.full((capacity,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        self.d_own = torch.full((capacity,), -1, dtype=torch.int32, device="cuda")
        self.n = ctx.pt_last_nee_rays(self.d_org.data_ptr(), self.d_dir.data_ptr(), self.d_occ.data_ptr(), self.d_own.data_ptr(), capacity, _stream())
        torch.cuda.synchronize()
        self.org = self.d_org.cpu().numpy().reshape(-1, 4)[:self.n]
        self.dir = self.d_dir.cpu().numpy().reshape(-1, 4)[:self.n]
        self.occ = self.d_occ.cpu().numpy().view(np.uint32)[:self.n]
        self.owner = self.d_own.cpu().numpy().view(np.uint32)[:self.n]
        self.by_owner = np.argsort(self.owner, kind="stable")       # blocks append to the queue in the order they get there: compare by owner
        assert np.all(self.d_own.cpu().numpy()[self.n:] == -1) and np.all(self.d_occ.cpu().numpy()[self.n:] == 0x5A5A5A5A), "nothing is written past the count"


class World(RR.World):
    def __init__(self):
        super().__init__()
        self.bounds = grid_bounds(self.sc.hs, self.sc.set)

    def bind(self, tset, regir=True, restir=False):
        self.ctx.bind_displaced(tset, self.sc.slots if len(tset) else [], restir=restir, regir=regir)


class KWorld:
    """DK.KScene with its far twin: a kinds binding, so the shell kernels run."""

    def __init__(self):
        self.sc = DK.KScene()
        self.ctx = self.sc.ctx
        self.far = api.TfdmSet(self.ctx)
        for i, k in enumerate(self.sc.which):
            m = np.array(K.TRANSFORMS[k], np.float32).copy()
            m[:, 3] += RR.FAR
            assert self.far.add(self.sc.objects[k], m, 100 + k) == i
        self.far.commit()
        self.bounds = grid_bounds(self.sc.hs, self.sc.set)

    def bind(self, tset, regir=True):
        self.ctx.bind_displaced_kinds(tset, self.sc.members(), regir=regir)

    def unbind(self):
        self.ctx.bind_displaced_kinds(None)


@pytest.fixture(scope="module")
def world(built_lib):
    w = World()
    yield w
    w.unbind()
    w.ctx.tunable_set("fuse_passes", 0)
    w.ctx.tunable_set("pt_overlap", 1)


@pytest.fixture(scope="module")
def kworld(built_lib):
    w = KWorld()
    yield w
    w.unbind()
    w.ctx.tunable_set("fuse_passes", 0)
    w.ctx.tunable_set("pt_overlap", 1)


def same(what, a, b, keys=KEYS):
    DR.assert_same_buffers(what, a, b, keys)


def _displaced(inst):
    return (inst != DR.INVALID) & (inst >= api.GBUFFER_DISPLACED)


# ---------------------------------------------------------------- 1. nothing displaced in play gives the unbound bytes
@pytest.mark.parametrize("sky", [False, True])
def test_nothing_displaced_in_play_gives_the_unbound_bytes(world, sky):
    """An empty set and S' (the camera sees none of it), each bound with the bit, against the unbound ReGIR frame sequence in its
    wavefront form ("fuse_passes" 1): three frames, path length 4, temporal build after frame 0, cell randomisation on.  Beauty, RNG,
    G-buffers, both cell-reservoir buffers and infos, slot RNGs, per-cell access counts, last-access frames, active-cell counts."""
    ctx = world.ctx
    env = (api.env_make_sky(64, 32), 64, 32) if sky else None
    cams = [DR.camera(0), DR.camera(1), DR.camera(0)]
    run = lambda: Regir(world.sc, world.bounds, env=env).frames(3, 4, cams)
    world.unbind()
    ctx.tunable_set("fuse_passes", 1)
    want = run()
    ctx.tunable_set("fuse_passes", 0)
    for name, tset in (("an empty set", world.empty), ("S'", world.far)):
        world.bind(tset)
        got = run()
        world.unbind()
        same("%s bound with the bit, sky %d" % (name, sky), got, want)
    world.bind(world.empty)
    ctx.tunable_set("fuse_passes", 2)                # asked for, and overruled by the binding
    got = run()
    ctx.tunable_set("fuse_passes", 0)
    world.unbind()
    same("an empty set bound, fuse_passes 2 requested, sky %d" % sky, got, want)
    assert np.isfinite(want["beauty"]).all() and want["beauty"][:, :3].mean() > 1e-3
    assert want["regir_accesses"].sum() + (want["regir_last_access"] != 0xFFFFFFFF).sum() > 0, "the grid was used"


def test_nothing_displaced_in_play_under_a_kinds_binding(kworld):
    """The same against a kinds binding over the far twin of the KScene set: the plain lanes of the shell kernels."""
    ctx = kworld.ctx
    cams = [K.camera(0), K.camera(1), K.camera(0)]
    run = lambda: Regir(kworld.sc, kworld.bounds).frames(3, 4, cams)
    kworld.unbind()
    ctx.tunable_set("fuse_passes", 1)
    want = run()
    ctx.tunable_set("fuse_passes", 0)
    kworld.bind(kworld.far)
    got = run()
    kworld.unbind()
    same("the far twin under a kinds binding", got, want)
    assert np.isfinite(want["beauty"]).all() and want["beauty"][:, :3].mean() > 1e-3


# ---------------------------------------------------------------- 2. the grid passes do not see the binding
def test_the_grid_passes_do_not_see_the_binding(world):
    """From identical state (one unbound ReGIR frame behind it, the parameters of frame 1 set) each of the three grid passes under S with
    the bit gives the bytes of the unbound pass."""
    world.unbind()
    fr = Regir(world.sc, world.bounds)
    fr.frames(1, 3, [DR.camera(0)])
    fr.params(1, DR.camera(1), DR.camera(0))
    snap = fr.snapshot()
    for pass_id in (api.PT_REGIR_BUILD_CELLS, api.PT_REGIR_BUILD_CELLS_TEMPORAL, api.PT_REGIR_UPDATE_LAST_ACCESS):
        out = []
        for bound in (False, True):
            fr.restore(snap)
            if bound:
                world.bind(world.sc.set)
            fr.launch(pass_id)
            out.append(fr.download())
            world.unbind()
        same("grid pass %d under S" % pass_id, out[1], out[0])
        before = {k: snap[1][k].cpu().numpy() for k in snap[1]}
        assert any(not np.array_equal(before[k].view(np.uint8).reshape(-1), np.ascontiguousarray(out[0][k]).view(np.uint8).reshape(-1)) for k in REGIR_KEYS), \
            "pass %d changes the grid state" % pass_id


# ---------------------------------------------------------------- 3. the shadow rays are the scene query's
def _check_nee_queue(ctx, accel, tset, far, what):
    q = NeeQueue(ctx)
    assert q.n > 0
    util.assert_same_bits("%s: occlusion words against gfx_trace_scene" % what, q.occ, RR.any_hit(ctx, accel, tset, q))
    plain = RR.any_hit(ctx, accel, None, q, scene=False)
    if tset is far:
        util.assert_same_bits("%s: occlusion words against gfx_trace under S'" % what, q.occ, plain)
    assert set(np.unique(q.occ)) <= {0, 1}
    assert np.all(q.dir[:, 3] > q.org[:, 3]), "a compacted queue holds rays only"
    assert len(np.unique(q.owner)) == q.n and q.owner.max() < W * H, "one entry per pixel at path length 1"
    print("%s: %d entries, %d occluded (%d by gfx_trace)" % (what, q.n, q.occ.sum(), plain.sum()))
    return q, plain


def _shadow_rays_case(w, tracer, regir_bit, which, cam):
    """Path length 1 (first vertex, its NEE trace, break), numAccumFrames 0, the G-buffer written under S."""
    tset = w.sc.set if which == "S" else w.far
    fr = Regir(w.sc, w.bounds)
    w.bind(w.sc.set, regir=True)
    fr.first_vertex_state(cam)
    w.bind(tset, regir=regir_bit)
    fr.launch(tracer, 1)
    q, plain = _check_nee_queue(w.ctx, w.sc.accel, tset, w.far, "%s, pass %d" % (which, tracer))
    w.unbind()
    assert np.isfinite(fr.dev.download()["beauty"]).all()
    return q, plain, fr


@pytest.mark.parametrize("which", ["S", "S'"])
@pytest.mark.parametrize("tracer", ["regir", "baseline"])
def test_the_shadow_rays_are_the_scene_querys(world, tracer, which):
    """The words of gfx_pt_last_nee_rays equal gfx_trace_scene (any hit) over the queue's own rays, under S and under S'; under S' they
    also equal gfx_trace.  The baseline tracer under a plain binding pins the new entry against code that did not change."""
    regir = tracer == "regir"
    q, plain, _ = _shadow_rays_case(world, api.PT_PATH_TRACE_REGIR if regir else api.PT_PATH_TRACE_BASELINE, regir, which, DR.camera(0))
    assert q.n > 0.3 * W * H
    if which == "S":
        assert (q.occ != plain).sum() > 0, "the displaced instances occlude some shadow ray the BVH8 lets through"


# ---------------------------------------------------------------- 4. the answer is consumed as before
def test_the_answer_is_consumed_as_before(world):
    """From identical state the ReGIR tracer at path length 1 runs under S' and under S.  Same rays, owners, RNG and cell accesses; beauty
    (entry by entry once both queues are put in the order of their owners: the blocks append in the order they get there); beauty
    differs exactly at the owners of entries whose word is 1 under S and 0 under S', and is there the first vertex's emission alone
    (zero: the camera sees no emitter at those pixels); those pixels are at least 1 % of the frame."""
    fr = Regir(world.sc, world.bounds)
    world.bind(world.sc.set)
    fr.first_vertex_state(DR.camera(0))
    snap = fr.snapshot()
    out, queue = {}, {}
    for name, tset in (("S'", world.far), ("S", world.sc.set)):
        fr.restore(snap)
        world.bind(tset)
        fr.launch(api.PT_PATH_TRACE_REGIR, 1)
        queue[name] = NeeQueue(world.ctx)
        out[name] = fr.download()
    world.unbind()
    a, b = queue["S"], queue["S'"]
    assert a.n == b.n and len(np.unique(a.owner)) == a.n, "one entry per pixel at path length 1"
    ia, ib = a.by_owner, b.by_owner
    util.assert_same_bits("owners", a.owner[ia], b.owner[ib])
    util.assert_same_bits("ray origins", a.org[ia], b.org[ib])
    util.assert_same_bits("ray directions", a.dir[ia], b.dir[ib])
    util.assert_same_bits("RNG", out["S"]["rng"], out["S'"]["rng"])
    util.assert_same_bits("per-cell access counts", out["S"]["regir_accesses"], out["S'"]["regir_accesses"])
    n = W * H
    words = lambda o: np.ascontiguousarray(o["beauty"]).view(np.uint32)
    changed = np.any(words(out["S"]) != words(out["S'"]), axis=1)
    occ_s, occ_f, owner = a.occ[ia], b.occ[ib], a.owner[ia]
    newly = (occ_s == 1) & (occ_f == 0)
    print("%d pixels changed; %d entries occluded under S only (%.2f %% of the frame)" % (changed.sum(), newly.sum(), 100.0 * newly.sum() / n))
    assert not ((occ_f == 1) & (occ_s == 0)).any(), "S' occludes nothing S does not"
    want_changed = np.zeros(n, bool)
    want_changed[owner[newly]] = True
    assert np.array_equal(changed, want_changed)
    inst = out["S"]["gb0_0"]["instSlot"]
    lamp = 1                                         # DR.Scene: instance 1 is the emissive rectangle
    assert not np.any(inst[want_changed] == lamp) and np.all(out["S"]["beauty"][want_changed, :3] == 0)
    assert np.all(out["S'"]["beauty"][want_changed, :3].max(axis=1) > 0)
    assert newly.sum() >= 0.01 * n


# ---------------------------------------------------------------- 5. displaced first vertices shade where the baseline's do
def test_displaced_first_vertices_shade_where_the_baselines_do(world):
    """From the same state under S, the baseline tracer and the ReGIR tracer at path length 1: for every pixel that owns an entry in both
    NEE queues the ray origins are equal bit for bit, and displaced pixels of every member are among them."""
    fr = Regir(world.sc, world.bounds)
    world.bind(world.sc.set)
    fr.first_vertex_state(DR.camera(0))
    snap = fr.snapshot()
    fr.launch(api.PT_PATH_TRACE_BASELINE, 1)
    qb = NeeQueue(world.ctx)
    fr.restore(snap)
    fr.launch(api.PT_PATH_TRACE_REGIR, 1)
    qg = NeeQueue(world.ctx)
    inst = fr.dev.download()["gb0_0"]["instSlot"]
    world.unbind()
    common, ib, ig = np.intersect1d(qb.owner, qg.owner, return_indices=True)
    util.assert_same_bits("NEE ray origins of the pixels both tracers sample a light for", qb.org[ib], qg.org[ig])
    counts = [int((inst[common] == (api.GBUFFER_DISPLACED | k)).sum()) for k in range(3)]
    plain = int((~_displaced(inst[common])).sum())
    print("%d common owners (baseline %d, ReGIR %d): plain %d, members %s" % (len(common), qb.n, qg.n, plain, counts))
    assert all(c > 0 for c in counts) and plain > 0


# ---------------------------------------------------------------- 6. cell accesses
def test_cell_accesses_count_every_surface_pixel_in_its_cell(world):
    """Randomisation off, path length 1, under S: every surface pixel, plain or displaced, counts one access, in the cell of its offset
    shading position.  Per cell lo <= got <= hi with lo the pixels whose G-buffer-2 position lies in the cell farther than eps from
    every inner face and hi those plus the ones within eps of a face of it (tests/displaced_regir_host.py); eps is twice the largest
    step offsetRayOrigin can take at the grid's largest coordinate."""
    fr = Regir(world.sc, world.bounds, randomize=0)
    world.bind(world.sc.set)
    fr.first_vertex_state(DR.camera(0))
    fr.launch(api.PT_PATH_TRACE_REGIR, 1)
    out = fr.download()
    world.unbind()
    inst = out["gb0_0"]["instSlot"]
    surface = inst != DR.INVALID
    pos = out["gb2_0"]["positionInWorld"][surface]
    got = out["regir_accesses"].astype(np.int64)
    eps = 2.0 * G.max_offset_step(float(np.abs(world.bounds).max()))
    cell = fr.rb.cell_size
    assert eps < 0.01 * float(cell.min())
    lo, hi, near = G.cell_count_bounds(pos, fr.rb.origin, cell, DIMS, eps)
    disp = _displaced(inst[surface])
    print("surface pixels %d (displaced %d), accesses %d, eps %.3g, smallest cell edge %.3g, within eps of an inner face %d, cells used %d" %
          (surface.sum(), disp.sum(), got.sum(), eps, cell.min(), near.sum(), (got > 0).sum()))
    assert disp.sum() > 0.05 * W * H
    assert near.sum() <= 0.02 * surface.sum(), "the grid puts a surface on an inner cell face: change the grid dimensions"
    assert got.sum() == surface.sum()
    assert np.all(lo <= got) and np.all(got <= hi), "cells off: %s" % np.nonzero((lo > got) | (got > hi))[0][:8]
    assert (got > 0).sum() >= 8


# ---------------------------------------------------------------- 7. determinism
def test_a_second_run_two_bands_and_no_overlap_give_the_same_bytes(world):
    cams = [DR.camera(0), DR.camera(1), DR.camera(0)]
    world.bind(world.sc.set)
    run = lambda **kw: Regir(world.sc, world.bounds).frames(3, 4, cams, **kw)
    want = run()
    same("a second run", run(), want)
    same("two row bands", run(bands=((0, 24), (24, 64))), want)
    world.ctx.tunable_set("pt_overlap", 0)
    got = run()
    world.ctx.tunable_set("pt_overlap", 1)
    same("pt_overlap off", got, want)
    world.unbind()
    disp = _displaced(want["gb0_0"]["instSlot"])
    rgb = want["beauty"][:, :3]
    assert disp.mean() > 0.05 and np.isfinite(rgb).all() and rgb[disp].mean() > 1e-3, "displaced pixels receive light"


# ---------------------------------------------------------------- 8. the integral
def test_the_integral_against_the_bound_path_tracer(built_lib):
    """64 x 48, 64 accumulated frames, path length 3, no environment.  G: the ReGIR tracer, P: the baseline tracer; stat(A, B) =
    rms((A - B) / (B + 0.01)) over 8 x 8 tile means.  Asserted: stat(G under S, P under S) <= 2 stat(G, P on the tessellated twin,
    unbound), where both renderers are existing code and the twin calibrates their systematic disagreement (the form and the margin of
    section 17's integral case); and the floor tiles in the hovering quad's shadow (selected as in section 16) are darkened by ReGIR
    under S by at least half of what ReGIR on the twin darkens them, against ReGIR with no quad.
    Measured on an MI355X: see DESIGN.md section 26."""
    w, h, frames, L = 64, 48, 64, 3
    cams = [DR.camera(0, w, h)] * frames
    rms = lambda x: float(np.sqrt(np.mean(x * x)))
    tiles = lambda x: DR._tile_means(x["beauty"], w, h)
    stat = lambda a, b: rms((a - b) / (b + 0.01))
    regir = lambda scene, bounds, seed: Regir(scene, bounds, w, h, seed=seed).frames(frames, L, cams, accumulate=True, jitter=1)
    tess = DR.Scene(tessellated=True, bunny=False)
    gt = regir(tess, tess.hs.bounds(), 1001)
    pt = DR.Frames(tess, w, h, seed=2002).render(frames, L, 1, cams)
    twin = stat(tiles(gt), tiles(pt))
    sc = DR.Scene(which=(0,), bunny=False)
    bounds = grid_bounds(sc.hs, sc.set)
    gu = regir(sc, bounds, 1001)                     # no quad: nothing bound
    sc.ctx.bind_displaced(sc.set, sc.slots, regir=True)
    gs = regir(sc, bounds, 1001)
    ps = DR.Frames(sc, w, h, seed=2002).render(frames, L, 1, cams)
    sc.unbind()
    got = stat(tiles(gs), tiles(ps))
    print("tessellated twin: stat(ReGIR, tracer) = %.4f; under S: %.4f (ratio %.2f); ReGIR under S against ReGIR on the twin: %.4f" %
          (twin, got, got / twin, stat(tiles(gs), tiles(gt))))
    assert np.mean(gs["gb0_1"]["instSlot"] == api.GBUFFER_DISPLACED) > 0.05, "the quad is in the picture"
    assert got <= 2 * twin
    whole = lambda x, inst: (x["gb0_1"]["instSlot"] == inst).reshape(h // 8, 8, w // 8, 8).all(axis=(1, 3)).reshape(-1)
    lum = lambda x: x.mean(axis=1)
    U, T, S = lum(tiles(gu)), lum(tiles(gt)), lum(tiles(gs))
    shadow = whole(gt, tess.floor_inst) & whole(gs, sc.floor_inst) & (T < 0.75 * U)
    print("shadow tiles: %d; mean luminance no quad %.4f, twin %.4f, under S %.4f" %
          (shadow.sum(), U[shadow].mean() if shadow.any() else 0, T[shadow].mean() if shadow.any() else 0, S[shadow].mean() if shadow.any() else 0))
    assert shadow.sum() >= 1, "the camera sees floor in the quad's shadow"
    assert np.all(U[shadow] - S[shadow] >= 0.5 * (U[shadow] - T[shadow]))


# ---------------------------------------------------------------- 9. kinds
@pytest.mark.parametrize("which", ["S", "S'"])
def test_kinds_the_shadow_rays_are_the_scene_querys(kworld, which):
    """Case 3 over the kinds binding; under S every member (TFDM, NRTDSM, shell, mirrored NRTDSM) owns NEE entries and both shell
    geometries own some."""
    q, plain, fr = _shadow_rays_case(kworld, api.PT_PATH_TRACE_REGIR, True, which, K.camera(0))
    g0 = fr.dev.download()["gb0_0"]
    inst, geom = g0["instSlot"][q.owner], g0["geomInstSlot"][q.owner]
    owners = [int((inst == (api.GBUFFER_DISPLACED | k)).sum()) for k in range(4)]
    shell = [int(((inst == (api.GBUFFER_DISPLACED | 2)) & (geom >> api.GEOM_SLOT_BITS == g)).sum()) for g in range(2)]
    print("NEE entries by member %s, by shell geometry %s" % (owners, shell))
    assert all(c > 0 for c in owners) and all(c > 0 for c in shell)
    if which == "S":
        assert (q.occ != plain).sum() > 0


def test_kinds_determinism_and_every_member_lit(kworld):
    """Case 7 over the kinds binding, and after 8 accumulated frames at path length 3 the mean beauty over each member's pixels is
    finite and above 1e-3."""
    cams = [K.camera(0), K.camera(1), K.camera(0)]
    kworld.bind(kworld.sc.set)
    run = lambda **kw: Regir(kworld.sc, kworld.bounds).frames(3, 4, cams, **kw)
    want = run()
    same("a second run", run(), want)
    same("two row bands", run(bands=((0, 24), (24, 64))), want)
    kworld.ctx.tunable_set("pt_overlap", 0)
    got = run()
    kworld.ctx.tunable_set("pt_overlap", 1)
    same("pt_overlap off", got, want)
    lit = Regir(kworld.sc, kworld.bounds).frames(8, 3, [K.camera(0)] * 8, accumulate=True, jitter=1)
    kworld.unbind()
    inst = lit["gb0_1"]["instSlot"]
    rgb = lit["beauty"][:, :3]
    assert np.isfinite(rgb).all()
    for k in range(4):
        on = inst == (api.GBUFFER_DISPLACED | k)
        print("member %d: %.1f %% of the pixels, mean beauty %.4f" % (k, 100 * on.mean(), rgb[on].mean()))
        assert on.mean() >= 0.02 and rgb[on].mean() > 1e-3, "member %d receives light" % k


# ---------------------------------------------------------------- 10. refusals
def test_refusals(world):
    import torch
    sc, ctx = world.sc, world.ctx
    fr = Regir(sc, world.bounds)
    fr.params(0, DR.camera(0))
    launch = lambda p: ctx.pt_launch(p, W, H, 3, 0, 0, _stream())
    regir_passes = (api.PT_REGIR_BUILD_CELLS, api.PT_REGIR_BUILD_CELLS_TEMPORAL, api.PT_PATH_TRACE_REGIR, api.PT_REGIR_UPDATE_LAST_ACCESS)
    nrc_passes = tuple(range(api.PT_NRC_PREPROCESS, api.PT_PATH_TRACE_NRC_RESTIR + 1))
    assert regir_passes == (2, 3, 4, 5) and api.PT_PATH_TRACE_NRC_REGIR in nrc_passes
    for restir in (False, True):                     # without the bit: today's message, byte for byte
        world.bind(sc.set, regir=False, restir=restir)
        fr.launch(api.PT_SETUP_GBUFFERS)
        for p in regir_passes + (api.PT_NRC_PREPROCESS, api.PT_PATH_TRACE_NRC_REGIR):
            with pytest.raises(api.GfxError, match="displaced instance set is bound.*" + re.escape(TODAYS_REFUSAL % p)):
                launch(p)
    world.bind(sc.set, regir=True, restir=True)      # the two bits together; NRC stays refused
    for p in nrc_passes:
        with pytest.raises(api.GfxError, match="displaced instance set is bound.*NRC pass %d is refused" % p):
            launch(p)
    for p in regir_passes:
        launch(p)
    ctx.restir_launch(api.PASS_INITIAL_RIS, W, H, _stream())
    torch.cuda.synchronize()
    for bind in (lambda m: ctx.bind_displaced(sc.set, sc.slots, pass_mask=m), lambda m: ctx.bind_displaced_kinds(sc.set, sc.slots, pass_mask=m)):
        for mask in (api.DISPLACED_GBUFFER_PT | 16, api.DISPLACED_GBUFFER_PT | api.DISPLACED_REGIR | 4):
            with pytest.raises(api.GfxError, match="unknown bit"):
                bind(mask)
    # displaced_check runs at every ReGIR launch
    world.bind(sc.set)
    sc.set.set_transform(0, DR.HOVER)
    for p in regir_passes:
        with pytest.raises(api.GfxError, match="not committed"):
            launch(p)
    with pytest.raises(api.GfxError, match="gfx_tfdm_set_bounds.*not committed"):
        sc.set.bounds()
    sc.set.commit()
    launch(api.PT_PATH_TRACE_REGIR)
    world.unbind()
    # gfx_tfdm_set_bounds
    table = sc.set.read()
    lo, hi = sc.set.bounds()
    util.assert_same_bits("set bounds, lo", lo, table["boxLo"].min(axis=0))
    util.assert_same_bits("set bounds, hi", hi, table["boxHi"].max(axis=0))
    lo, hi = world.empty.bounds()
    assert np.all(lo > hi) and np.all(np.isinf(lo)) and np.all(np.isinf(hi))
    fresh_set = api.TfdmSet(ctx)
    fresh_set.add(sc.tfdm[0], DR.HOVER, 1)
    with pytest.raises(api.GfxError, match="not committed"):
        fresh_set.bounds()
    fresh_set.close()
    # gfx_pt_last_nee_rays
    fresh = DR.Scene(which=(), bunny=False)
    bufs = [torch.zeros(4 * CAP, dtype=torch.float32, device="cuda") for _ in range(4)]
    args = tuple(b.data_ptr() for b in bufs)
    with pytest.raises(api.GfxError, match="no NEE pass"):
        fresh.ctx.pt_last_nee_rays(*args, CAP, _stream())
    ff = Regir(fresh, fresh.hs.bounds())
    ff.first_vertex_state(DR.camera(0))
    fresh.ctx.tunable_set("fuse_passes", 2)
    ff.launch(api.PT_PATH_TRACE_REGIR, 1)
    with pytest.raises(api.GfxError, match="fused"):
        fresh.ctx.pt_last_nee_rays(*args, CAP, _stream())
    fresh.ctx.tunable_set("fuse_passes", 1)
    ff.launch(api.PT_PATH_TRACE_REGIR, 1)
    with pytest.raises(api.GfxError, match="capacity"):
        fresh.ctx.pt_last_nee_rays(*args, 16, _stream())
    with pytest.raises(api.GfxError, match="aligned"):
        fresh.ctx.pt_last_nee_rays(args[0] + 4, args[1], args[2], args[3], CAP, _stream())
    with pytest.raises(api.GfxError, match="aligned"):
        fresh.ctx.pt_last_nee_rays(args[0], args[1], args[2], args[3] + 2, CAP, _stream())
    n = fresh.ctx.pt_last_nee_rays(args[0], args[1], args[2], 0, CAP, _stream())      # no owners asked for; and without a binding it works
    assert 0.3 * W * H < n <= W * H
    torch.cuda.synchronize()
