"""Shared by tools/tfdm_view.py, tools/bench_tfdm.py and the TFDM tests: procedural height maps, the base meshes, a look-at camera."""
import ctypes as C
import os

import numpy as np

from gfxexp_amd import api

ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "assets")


def procedural_map(n):
    """Two sines and a ripple, quantised to 8 bits like a height texture: float32 c / 255, [n, n]."""
    y, x = np.mgrid[0:n, 0:n]
    h = 0.5 + 0.25 * np.sin(2 * np.pi * 3 * x / n) * np.cos(2 * np.pi * 2 * y / n) + 0.2 * np.sin(2 * np.pi * (5 * x + 7 * y) / n) \
        + 0.04 * np.sin(2 * np.pi * 37 * x / n) * np.sin(2 * np.pi * 41 * y / n)
    return (np.round(np.clip(h, 0, 1) * 255).astype(np.float32) / np.float32(255)).astype(np.float32)


def quad_mesh():
    """Unit quad in z = 0, normal +z, uv = xy, split along the TL-BR diagonal: TL TR BR, TL BR BL."""
    v = np.zeros(4, api.VERTEX_DTYPE)
    v["position"] = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)]
    v["normal"] = (0, 0, 1)
    v["texCoord0Dir"] = (1, 0, 0)
    v["texCoord"] = [(0, 0), (1, 0), (1, 1), (0, 1)]
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.uint32)


def obj_mesh(name):
    s = api.HostScene()
    s.load_obj(os.path.join(ASSETS, name))
    vs, ts, base = [], [], 0
    for v, t, _ in s.geoms():
        vs.append(v)
        ts.append(t + base)
        base += len(v)
    return np.concatenate(vs), np.concatenate(ts).astype(np.uint32)


def base_mesh(name):
    """(vertices, triangles, camera position, look-at point, up)"""
    if name == "quad":
        v, t = quad_mesh()
        return v, t, (0.5, -0.75, 0.8), (0.5, 0.45, 0.0), (0, 0, 1)
    v, t = obj_mesh({"bunny": "stanford_bunny_309_faces.obj", "teapot": "teapot.obj"}[name])
    lo, hi = v["position"].min(0).astype(np.float64), v["position"].max(0).astype(np.float64)
    c, r = 0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo))
    return v, t, tuple(c + np.array([0.6, 0.9, 2.0]) * r), tuple(c), (0, 1, 0)


def extent(v):
    return float((v["position"].max(0) - v["position"].min(0)).max())


def look_at_camera(width, height, pos, target, fov_y_deg=42.0, up=(0, 0, 1)):
    """A gfx_camera at `pos` looking at `target` (orientation columns: left, up, forward)."""
    f = np.asarray(target, np.float64) - np.asarray(pos, np.float64)
    f /= np.linalg.norm(f)
    left = np.cross(np.asarray(up, np.float64), f)
    left /= np.linalg.norm(left)
    cam = api.GfxCamera()
    cam.aspect = float(width) / float(height)
    cam.fovY = float(np.radians(fov_y_deg))
    cam.position = (C.c_float * 3)(*[float(x) for x in pos])
    cam.orientation = (C.c_float * 9)(*np.stack([left, np.cross(f, left), f], axis=1).astype(np.float32).reshape(9).tolist())
    return cam


def tessellated_quad(heights, h_scale):
    """The displaced unit quad of quad_mesh() as ordinary triangles, two per texel (TL TR BR, TL BR BL): corner heights are the mean of
    the four texels around the corner with repeat wrap, as the query samples them."""
    n = heights.shape[0]
    h = heights.astype(np.float64)
    i = np.arange(n + 1)
    a, b = (i - 1) % n, i % n
    corner = 0.25 * (h[np.ix_(a, a)] + h[np.ix_(a, b)] + h[np.ix_(b, a)] + h[np.ix_(b, b)])
    gy, gx = np.mgrid[0:n + 1, 0:n + 1]
    v = np.zeros((n + 1) * (n + 1), api.VERTEX_DTYPE)
    v["position"] = np.stack([gx.ravel() / n, gy.ravel() / n, (h_scale * corner).ravel()], 1)
    v["normal"] = (0, 0, 1)
    v["texCoord0Dir"] = (1, 0, 0)
    v["texCoord"] = np.stack([gx.ravel() / n, gy.ravel() / n], 1)
    y, x = np.mgrid[0:n, 0:n]
    tl = (y * (n + 1) + x).ravel()
    tr, bl, br = tl + 1, tl + n + 1, tl + n + 2
    t = np.concatenate([np.stack([tl, tr, br], 1), np.stack([tl, br, bl], 1)]).astype(np.uint32)
    return v, t


def shell_geom(name):
    """A shell mesh for api.Shell: (positions [n, 3] as (u, v, h), triangles [m, 3]); "box" (gfxh_shell_box) or "bunny" (the
    309-face bunny through gfxh_shell_fit, Y up)."""
    if name == "box":
        return api.shell_box()
    v, t = obj_mesh("stanford_bunny_309_faces.obj")
    return api.shell_fit(v["position"], y_up=True), t


def instantiated_shell_on_quad(geom, tiles, h_scale):
    """The shell mesh `geom` repeated tiles x tiles times over quad_mesh() as ordinary triangles (indexed: one copy of the shell's
    vertices per tile), in float64: what gfx_shell_trace intersects there with tex_scale = (tiles, tiles), since the map is affine on
    the quad.  A shell height h lies at z = h_scale / tiles * h."""
    pos, tri = np.asarray(geom[0], np.float64), np.asarray(geom[1], np.int64)
    j, i = np.mgrid[0:tiles, 0:tiles]
    shift = np.stack([i.ravel(), j.ravel(), np.zeros(tiles * tiles)], 1)                      # [tiles^2, 3]
    p = (pos[None] + shift[:, None]) * np.array([1.0 / tiles, 1.0 / tiles, h_scale / tiles])
    v = np.zeros(len(shift) * len(pos), api.VERTEX_DTYPE)
    v["position"] = p.reshape(-1, 3)
    v["normal"] = (0, 0, 1)
    v["texCoord0Dir"] = (1, 0, 0)
    t = (tri[None] + (np.arange(len(shift)) * len(pos))[:, None, None]).reshape(-1, 3).astype(np.uint32)
    return v, t


def affine(linear, translation):
    """Row-major 3 x 4 float32 from a 3 x 3 linear part and a translation."""
    m = np.zeros((3, 4), np.float64)
    m[:, :3], m[:, 3] = linear, translation
    return m.astype(np.float32)


def rotation_x(degrees):
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float64)


def mixed_scene(map_size):
    """The scene of tools/tfdm_view.py --scene and tools/bench_scene_trace.py, z up: a plain teapot (15 704 triangles in the BVH8)
    standing on a displaced 4 x 4 ground quad, and a second displaced quad as a tilted wall behind it; both quads share one
    height map of map_size x map_size.  Returns (HostScene of the plain part, (vertices, triangles, heights, params) of the
    displaced object, [(objToWorld, userId)] of its instances, camera position, look-at point)."""
    s = api.HostScene()
    g = s.load_obj(os.path.join(ASSETS, "teapot.obj"))
    tv, _ = obj_mesh("teapot.obj")
    lo, hi = tv["position"].min(0).astype(np.float64), tv["position"].max(0).astype(np.float64)
    k = 1.6 / float((hi - lo).max())
    up = rotation_x(90.0)                                   # the teapot's y axis becomes z
    centre = 0.5 * (lo + hi)
    # its footprint centred on the ground quad, its lowest point just above the crests of the ground (0.08)
    s.add_instance(g, affine(k * up, (-k * centre[0], k * centre[2], 0.08 - k * lo[1])))
    v, t = quad_mesh()
    gp = api.tfdm_params(h_scale=0.02, tex_scale=(1.0, 1.0))            # in object space: 0.08 under the ground's scale of 4
    ground = affine(np.diag([4.0, 4.0, 4.0]), (-2.0, -2.0, 0.0))
    wall = affine(rotation_x(70.0) @ np.diag([4.0, 2.5, 4.0]), (-2.0, 2.0, 0.0))
    return s, (v, t, procedural_map(map_size), gp), [(ground, 1), (wall, 2)], (0.6, -4.2, 2.2), (0.0, 0.3, 0.6)


# ---------------------------------------------------------------- the mixed scene, lit and path traced (tools/tfdm_view.py --render, tools/bench_displaced_render.py)
def lit_mixed_scene(map_size, tessellate=False):
    """mixed_scene() with an emissive rectangle above it and a constant grey Lambert material for the two displaced quads.
    tessellate=False: the quads' shading geometry is added in NO group (gfx_scene_bind_displaced wants it so) and its slot returned.
    tessellate=True: the quads stand in the BVH8 as tessellated_quad() meshes, two triangles per texel, under the same transforms.
    Returns (HostScene, (vertices, triangles, heights, params), instances, shading geometry slot or None, camera position, target)."""
    s, (v, t, heights, gp), instances, pos, target = mixed_scene(map_size)
    grey = api.GfxMaterial()
    grey.bsdfType = 0                                       # GFX_BSDF_LAMBERT
    grey.a = (C.c_float * 3)(0.7, 0.7, 0.7)
    grey_slot = s.add_material(grey)
    lamp = s.add_material_traditional((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0.0, emittance=(40.0, 38.0, 34.0))
    lv = np.zeros(4, api.VERTEX_DTYPE)
    lv["position"] = [(-1.5, -1.5, 4.5), (1.5, -1.5, 4.5), (1.5, 1.5, 4.5), (-1.5, 1.5, 4.5)]
    lv["normal"] = (0, 0, -1)
    lv["texCoord0Dir"] = (1, 0, 0)
    s.add_instance(s.add_group([s.add_geom(lv, np.array([[0, 2, 1], [0, 3, 2]], np.uint32), lamp)]), affine(np.eye(3), (0, 0, 0)))
    slot = None
    if tessellate:
        mv, mt = tessellated_quad(heights, gp.hScale)
        group = s.add_group([s.add_geom(mv, mt, grey_slot)])
        for m, _ in instances:
            s.add_instance(group, m)
    else:
        slot = s.add_geom(v, t, grey_slot)
    return s, (v, t, heights, gp), instances, slot, pos, target


class PathTraceFrames:
    """The per-pixel buffers of the G-buffer pass + baseline path tracer on the device (torch), and one frame of the two passes."""

    def __init__(self, ctx, accel, width, height, seed=591842031321323413):
        import torch
        self.ctx, self.accel, self.w, self.h = ctx, accel, width, height
        n = width * height
        z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        self.t = {"rng": torch.from_numpy(api.seed_rng_states(n, seed).view(np.uint8)).cuda(), "beauty": z(16 * n), "albedo": z(16 * n), "normal": z(16 * n)}
        for i in range(2):
            self.t.update({"gb0_%d" % i: z(16 * n), "gb1_%d" % i: z(8 * n), "gb2_%d" % i: z(16 * n), "gb3_%d" % i: z(16 * n)})
        s = api.GfxRestirStaticParams()
        s.imageSizeX, s.imageSizeY = width, height
        s.rngBuffer = self.t["rng"].data_ptr()
        for i in range(2):
            s.gbuffer0[i], s.gbuffer1[i] = self.t["gb0_%d" % i].data_ptr(), self.t["gb1_%d" % i].data_ptr()
            s.gbuffer2[i], s.gbuffer3[i] = self.t["gb2_%d" % i].data_ptr(), self.t["gb3_%d" % i].data_ptr()
        s.beautyAccumBuffer, s.albedoAccumBuffer, s.normalAccumBuffer = self.t["beauty"].data_ptr(), self.t["albedo"].data_ptr(), self.t["normal"].data_ptr()
        s.numTilesX, s.numTilesY = (width + 7) // 8, (height + 7) // 8
        self.s = s

    def frame(self, index, cam, max_len=5, stream=0):
        f = api.GfxRestirFrameParams()
        C.memmove(C.byref(f.camera), C.byref(cam), C.sizeof(cam))
        C.memmove(C.byref(f.prevCamera), C.byref(cam), C.sizeof(cam))
        f.travHandle, f.numAccumFrames, f.frameIndex, f.bufferIndex = self.accel, index, index, index % 2
        f.resetFlowBuffer, f.enableJittering, f.envLightPowerCoeff = int(index == 0), 1, 1.0
        self.ctx.lights_build_instances(stream)
        self.ctx.restir_set_params(self.s, f, 0, 0, stream)
        self.ctx.pt_launch(api.PT_SETUP_GBUFFERS, self.w, self.h, max_len, 0, 0, stream)
        self.ctx.pt_launch(api.PT_PATH_TRACE_BASELINE, self.w, self.h, max_len, 0, 0, stream)

    def beauty(self):
        import torch
        torch.cuda.synchronize()
        return self.t["beauty"].cpu().numpy().view(np.float32).reshape(-1, 4)


class RegirFrames(PathTraceFrames):
    """... and a ReGIR grid over `bounds` (lo + hi, six floats: the scene's bounds joined with the bound set's, whose members are not in
    the BVH8), with one frame of the ReGIR loop: G-buffer, build cells (temporal after frame 0), PATH_TRACE_REGIR, update last access
    (regir_main.cpp:2021-2066)."""
    SLOTS_PER_CELL = 512

    def __init__(self, ctx, accel, width, height, bounds, dims=(16, 8, 16), seed=591842031321323413):
        import torch
        super().__init__(ctx, accel, width, height, seed)
        cells = int(dims[0]) * int(dims[1]) * int(dims[2])
        slots = cells * self.SLOTS_PER_CELL
        z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        self.t["regir_rngs"] = torch.from_numpy(api.seed_rng_states(slots, seed).view(np.uint8)).cuda()
        self.t["regir_accesses"] = z(4 * cells)
        self.t["regir_last_access"] = torch.full((4 * cells,), 0xFF, dtype=torch.uint8, device="cuda")
        g = api.GfxRegirParams()
        for i in range(2):
            self.t.update({"regir_res_%d" % i: z(48 * slots), "regir_info_%d" % i: z(8 * slots), "regir_active_%d" % i: z(4)})
            g.reservoirs[i], g.reservoirInfos[i] = self.t["regir_res_%d" % i].data_ptr(), self.t["regir_info_%d" % i].data_ptr()
            g.numActiveCells[i] = self.t["regir_active_%d" % i].data_ptr()
        g.lightSlotRngs, g.perCellNumAccesses = self.t["regir_rngs"].data_ptr(), self.t["regir_accesses"].data_ptr()
        g.lastAccessFrameIndices = self.t["regir_last_access"].data_ptr()
        lo, hi = np.asarray(bounds[:3], np.float32), np.asarray(bounds[3:], np.float32)
        size = ((hi - lo) / np.asarray(dims, np.float32)).astype(np.float32)
        for k in range(3):
            g.gridOrigin[k], g.gridCellSize[k], g.gridDimension[k] = float(lo[k]), float(size[k]), int(dims[k])
        g.log2NumCandidatesPerLightSlot, g.log2NumCandidatesPerCell, g.enableCellRandomization = 3, 2, 1
        self.g = g

    def frame(self, index, cam, max_len=5, stream=0):
        f = api.GfxRestirFrameParams()
        C.memmove(C.byref(f.camera), C.byref(cam), C.sizeof(cam))
        C.memmove(C.byref(f.prevCamera), C.byref(cam), C.sizeof(cam))
        f.travHandle, f.numAccumFrames, f.frameIndex, f.bufferIndex = self.accel, index, index, index % 2
        f.resetFlowBuffer, f.enableJittering, f.envLightPowerCoeff = int(index == 0), 1, 1.0
        ctx = self.ctx
        ctx.lights_build_instances(stream)
        ctx.restir_set_params(self.s, f, 0, 0, stream)
        ctx.regir_set_params(self.g)
        build = api.PT_REGIR_BUILD_CELLS_TEMPORAL if index else api.PT_REGIR_BUILD_CELLS
        for pass_id in (api.PT_SETUP_GBUFFERS, build, api.PT_PATH_TRACE_REGIR, api.PT_REGIR_UPDATE_LAST_ACCESS):
            ctx.pt_launch(pass_id, self.w, self.h, max_len, 0, 0, stream)


def joined_bounds(scene_bounds, tset=None):
    """lo + hi (six floats) of the scene's bounds joined with a displaced-instance set's (TfdmSet.bounds), for a ReGIR grid."""
    b = np.asarray(scene_bounds, np.float32)
    if tset is None:
        return b
    lo, hi = tset.bounds()
    return np.concatenate([np.minimum(b[:3], lo), np.maximum(b[3:], hi)]).astype(np.float32)


class RestirFrames(PathTraceFrames):
    """... and the buffers of the ReSTIR DI passes (reservoirs, reservoir info, sample visibility, neighbour deltas) with one frame of
    G-buffer, initial + temporal (biased), `spatial` biased spatial passes and shading, sequenced as restir_di_main.cpp does."""
    NUM_NEIGHBORS = 5

    def __init__(self, ctx, accel, width, height, seed=591842031321323413):
        import torch
        super().__init__(ctx, accel, width, height, seed)
        n = width * height
        z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        self.t["deltas"] = torch.from_numpy(api.spatial_neighbor_deltas().view(np.uint8).reshape(-1)).cuda()
        for i in range(2):
            self.t.update({"res_%d" % i: z(48 * n), "info_%d" % i: z(8 * n), "vis_%d" % i: z(4 * n)})
            self.s.reservoirBuffer[i], self.s.reservoirInfoBuffer[i] = self.t["res_%d" % i].data_ptr(), self.t["info_%d" % i].data_ptr()
            self.s.sampleVisibilityBuffer[i] = self.t["vis_%d" % i].data_ptr()
        self.s.spatialNeighborDeltas = self.t["deltas"].data_ptr()
        self.last_res, self.last_base = 1, 0

    def frame(self, index, cam, spatial=2, stream=0, accumulate=True):
        f = api.GfxRestirFrameParams()
        C.memmove(C.byref(f.camera), C.byref(cam), C.sizeof(cam))
        C.memmove(C.byref(f.prevCamera), C.byref(cam), C.sizeof(cam))
        f.travHandle, f.numAccumFrames, f.frameIndex, f.bufferIndex = self.accel, index if accumulate else 0, index, index % 2
        f.resetFlowBuffer, f.enableJittering, f.envLightPowerCoeff = int(index == 0), 1, 1.0
        f.spatialNeighborRadius, f.radiusThresholdForSpatialVisReuse = 20.0, 10.0
        f.log2NumCandidateSamples, f.numSpatialNeighbors, f.useLowDiscrepancyNeighbors = 5, self.NUM_NEIGHBORS, 1
        f.reuseVisibility, f.reuseVisibilityForTemporal, f.enableTemporalReuse, f.enableSpatialReuse = 1, 1, 1, 1
        ctx, w, h = self.ctx, self.w, self.h
        ctx.lights_build_instances(stream)
        cur = (self.last_res + 1) % 2

        def launch(pass_id, cur_res, base):
            ctx.restir_set_params(self.s, f, cur_res, base, stream)
            ctx.restir_launch(pass_id, w, h, stream)

        launch(api.PASS_SETUP_GBUFFERS, cur, self.last_base)
        launch(api.PASS_INITIAL_RIS if index == 0 else api.PASS_INITIAL_TEMPORAL_BIASED, cur, self.last_base)
        for i in range(spatial):
            launch(api.PASS_SPATIAL_BIASED, cur, self.last_base + self.NUM_NEIGHBORS * i)
            cur = (cur + 1) % 2
        self.last_base += self.NUM_NEIGHBORS * spatial
        launch(api.PASS_SHADING, cur, self.last_base)
        self.last_res = cur
