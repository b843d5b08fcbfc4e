"""Look at a displaced surface: pinhole primary rays through gfx_tfdm_trace, the normals and the depth written as images.

    python tools/tfdm_view.py [--mesh quad|bunny|teapot] [--height FILE] [--size 256] [--scale 0.05] [--level 0] [--box | --bilinear]
                              [--tex-scale 1] [--rotation 0] [--width 960] [--height-px 540] [--out tfdm_view]

--height: a .png / .jpg / .tga / .dds height map (gfxh_tfdm_load_height); without it a procedural map of --size.  --scale is
relative to the mesh's extent.  --box / --bilinear: the local intersection, GFX_TFDM_BOX / GFX_TFDM_BILINEAR (the smooth surface by
Newton's iteration) instead of two triangles per texel; with --scene, --render and --restir they set the mode of the scene's
displaced object.  Writes <out>_normal.png (n * 0.5 + 0.5 in object space) and <out>_depth.png (near = bright), and
prints the hit share and the traversal counters per ray.

    python tools/tfdm_view.py --nrtdsm [--mesh teapot] [--height FILE] [--size 256] [--scale 0.05] [--out tfdm_view]

--nrtdsm: the same images through gfx_nrtdsm_trace, the crack-free query that displaces along the interpolated, not renormalised normals
(csrc/nrtdsm/); the teapot unless --mesh says otherwise.  Map values must lie in [0, 1].

    python tools/tfdm_view.py --shell [box|bunny] [--mesh quad|bunny|teapot] [--tiles 16] [--scale 0.5] [--out tfdm_view]

--shell: a shell mesh (the "One Box", or the 309-face bunny placed by gfxh_shell_fit) repeated --tiles times per unit of texture
coordinate over the base mesh, through gfx_shell_trace (csrc/nrtdsm/shell*).  --scale: the height of one unit of shell height in
tiles.  Writes <out>_normal.png, <out>_depth.png and <out>_geom.png (the shell geometry index as a colour, tiles alternating in
brightness like a checkerboard).

    python tools/tfdm_view.py --scene [--size 256] [--width 960] [--height-px 540] [--out tfdm_view]

--scene: a plain teapot on a displaced ground quad with a second displaced quad as a tilted wall (tfdm_common.mixed_scene), through
ONE gfx_trace_scene call.  Writes <out>_normal.png (world-space normals of the displaced hits; plain hits grey), <out>_depth.png
and <out>_instance.png (plain geometry grey, every displaced instance a colour of its own, misses black).

    python tools/tfdm_view.py --scene --nrtdsm [--size 256] [--width 960] [--height-px 540] [--out tfdm_view]

--scene --nrtdsm: the same scene with the wall an NRTDSM member of the set (gfx_tfdm_set_add_nrtdsm; the ground stays TFDM), the same
three images through the same ONE gfx_trace_scene call.  With --render or --restir the set is bound through
gfx_scene_bind_displaced_kinds and rendered.

    python tools/tfdm_view.py --scene --shell [box|bunny] [--tiles 16] [--width 960] [--height-px 540] [--out tfdm_view]

--scene --shell: the same scene with the wall a shell member of the set (gfx_tfdm_set_add_shell: the "One Box" shell or the 309-face
bunny, --tiles x --tiles over the wall's mesh; the ground stays TFDM), through ONE gfx_trace_scene_ex call.  The same three images
and <out>_geom.png, from the call's side output: the shell geometry of the hit as a colour, its tile as a checkerboard; black where
the winner is no shell member.  With --render or --restir the set is rendered as with --nrtdsm, the shell geometry under a material
of its own.

    python tools/tfdm_view.py --scene --render [--frames 64] [--size 256] [--width 960] [--height-px 540] [--out tfdm_view]

--render: the same scene under an emissive rectangle, path traced through the bound instance set (gfx_scene_bind_displaced: the
G-buffer pass and the baseline path tracer), --frames accumulated frames, written tone-mapped as <out>_render.png.

    python tools/tfdm_view.py --scene --restir [--frames 64] [--size 256] [--width 960] [--height-px 540] [--out tfdm_view]

--restir: the scene of --render by ReSTIR DI under a binding that carries GFX_DISPLACED_RESTIR (G-buffer, initial + temporal, two
spatial passes, shading; the shadow rays are the scene's any-hit query), --frames accumulated frames, written tone-mapped as
<out>_restir.png.

    python tools/tfdm_view.py --scene --regir [--nrtdsm | --shell] [--frames 64] [--size 256] [--width 960] [--height-px 540] [--out tfdm_view]

--regir: the scene of --render through the ReGIR frame loop under a binding that carries GFX_DISPLACED_REGIR (G-buffer, build cells --
temporal after frame 0 --, GFX_PT_PATH_TRACE_REGIR, update last access), the grid over the scene's bounds joined with the set's
(gfx_tfdm_set_bounds: the displaced members are not in the BVH8), --frames accumulated frames, written tone-mapped as <out>_regir.png.

    python tools/tfdm_view.py --scene --restir --move N [--step 0.02] [--size 256] [--width 960] [--height-px 540] [--out tfdm_view]

--move N: N frames of the --restir scene with the wall translating by --step along x per frame (gfx_tfdm_set_move + commit before each
frame after the first) and the ground fixed; temporal reuse is on and nothing is accumulated.  Writes the last frame as
<out>_move.png and its motion vectors as <out>_motion.png (red / green = 0.5 + mv / 16 pixels: grey stands still).

    python tools/tfdm_view.py --ripple N [--nrtdsm] [--scene [--render | --restir]] [--size 256] [--out tfdm_view]

--ripple N: N frames of a travelling ripple written into the middle quarter of the height map by a torch expression on the device;
each frame is one gfx_tfdm_update_heights (gfx_nrtdsm_update_heights) of that sub-rectangle, with --scene one gfx_tfdm_set_commit,
and the frame's trace or render.  No micro-geometry is rebuilt: the pyramid above the rectangle, the per-triangle boxes and a refit
of the tree.  With --scene the map of the wall's object moves (without --nrtdsm the ground shares that object).  The images are those
of the last frame; with --restir nothing is accumulated (with --render the frames accumulate, so the ripple blurs)."""
import argparse
import json
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gfxexp_amd import api  # noqa: E402
import tfdm_common as K  # noqa: E402


def _local(a):
    return api.TFDM_BOX if a.box else api.TFDM_BILINEAR if a.bilinear else api.TFDM_TWO_TRIANGLE


class Ripple:
    """The middle quarter of a map, rippling: frame k is the map's own values plus a damped ring wave of phase k, clipped to [0, 1]."""

    def __init__(self, heights):
        size = heights.shape[0]
        self.rect = (size // 4, size // 4, max(size // 2, 1), max(size // 2, 1))
        x0, y0, w, h = self.rect
        self.base = torch.from_numpy(np.ascontiguousarray(heights[y0:y0 + h, x0:x0 + w], np.float32)).cuda()
        yy, xx = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(w, device="cuda", dtype=torch.float32), indexing="ij")
        self.r = torch.sqrt((xx - 0.5 * w) ** 2 + (yy - 0.5 * h) ** 2)
        self.damp = torch.exp(-self.r / (0.35 * w))

    def apply(self, obj, k, stream):
        x0, y0, w, h = self.rect
        src = torch.clamp(self.base + 0.15 * torch.sin(0.35 * self.r - 0.6 * k) * self.damp, 0.0, 1.0).contiguous()
        obj.update_heights(src.data_ptr(), x0, y0, w, h, stream=stream)      # returns when the update is done: `src` may go


def _depth_image(dist, hit, n):
    depth = np.zeros((n, 4), np.float32)
    depth[:, 3] = 1
    if hit.any():
        d = dist[hit]
        depth[hit, :3] = (1.0 - 0.9 * (d - d.min()) / max(float(d.max() - d.min()), 1e-30))[:, None]
    return depth


def scene_render(a):
    hs, (v, t, heights, gp), instances, slot, pos, target = K.lit_mixed_scene(a.size)
    gp.localIntersection = _local(a)
    warm = api.GfxMaterial()
    warm.bsdfType = 0                                       # GFX_BSDF_LAMBERT: the material of the shell geometry of a --shell wall
    warm.a = (C.c_float * 3)(0.8, 0.45, 0.25)
    shell_mat = hs.add_material(warm)
    ctx = api.Context(0)
    hs.upload(ctx)
    accel = ctx.accel_build()
    ctx.lights_build_static()
    tf = api.Tfdm(ctx, v, t, heights, gp)
    # --nrtdsm / --shell: the wall (the last instance) as in scene_view; such a set is bound through gfx_scene_bind_displaced_kinds,
    # a shell wall with one material per shell geometry
    wall = api.Nrtdsm(ctx, v, t, heights, api.tfdm_params(h_scale=gp.hScale, tex_scale=(gp.texScale[0], gp.texScale[1]))) if a.nrtdsm else None
    if a.shell:
        wall = api.Shell(ctx, v, t, [K.shell_geom(a.shell)], api.shell_params(h_scale=0.5 * K.extent(v), tex_scale=(a.tiles, a.tiles)))
    tset = api.TfdmSet(ctx)
    for k, (m, uid) in enumerate(instances):
        tset.add(wall if wall is not None and k == len(instances) - 1 else tf, m, uid)
    tset.commit()
    if wall is None:
        ctx.bind_displaced(tset, [slot] * len(instances), restir=a.restir, regir=a.regir)
    else:
        members = [slot] * (len(instances) - 1) + [(slot, [shell_mat]) if a.shell else slot]
        ctx.bind_displaced_kinds(tset, members, restir=a.restir, regir=a.regir)
    w, h = a.width, a.height_px
    if a.regir:
        frames = K.RegirFrames(ctx, accel, w, h, K.joined_bounds(hs.bounds(), tset))
    else:
        frames = K.RestirFrames(ctx, accel, w, h) if a.restir else K.PathTraceFrames(ctx, accel, w, h)
    cam = K.look_at_camera(w, h, pos, target)
    stream = torch.cuda.current_stream().cuda_stream
    if a.move:
        return scene_move(a, ctx, tset, instances, frames, cam, stream)
    ripple = Ripple(heights) if a.ripple else None
    for k in range(a.ripple or a.frames):
        if ripple:
            ripple.apply(wall if wall is not None else tf, k, stream)
            tset.commit(stream)
        frames.frame(k, cam, stream=stream, **({"accumulate": False} if ripple and a.restir else {}))
    beauty = frames.beauty()
    ctx.bind_displaced_kinds(None)
    image = a.out + ("_restir.png" if a.restir else "_regir.png" if a.regir else "_render.png")
    api.save_image_sdr(image, beauty, w, h, api.sdr_config(brightness=1.0, tone_map=True, gamma=True))
    g0 = frames.t["gb0_%d" % (((a.ripple or a.frames) - 1) % 2)].cpu().numpy().view(np.uint32).reshape(-1, 4)[:, 0]
    print(json.dumps({"scene": "teapot on displaced ground, displaced wall, emissive rectangle", "size": int(heights.shape[0]), "frames": a.ripple or a.frames, "ripple": bool(a.ripple),
                      "displaced_pixel_share": round(float(((g0 != api.GFX_INVALID_SLOT) & (g0 >= api.GBUFFER_DISPLACED)).mean()), 4),
                      "renderer": "restir_di" if a.restir else "regir" if a.regir else "path_tracer", "wall": "nrtdsm" if a.nrtdsm else "shell" if a.shell else "tfdm", "mean_radiance": round(float(beauty[:, :3].mean()), 5), "images": [image]}))
    return 0


def scene_move(a, ctx, tset, instances, frames, cam, stream):
    """--move: the wall (instance 1) translates along x, one gfx_tfdm_set_move + commit per frame; the ground stays."""
    w, h = a.width, a.height_px
    wall = np.array(instances[1][0], np.float32)
    for k in range(a.move):
        if k:
            m = wall.copy()
            m[0, 3] += a.step * k
            tset.move(1, m)
            tset.commit(stream)
        frames.frame(k, cam, stream=stream, accumulate=False)
    beauty = frames.beauty()
    ctx.bind_displaced(None)
    b = (a.move - 1) % 2
    g0 = frames.t["gb0_%d" % b].cpu().numpy().view(np.uint32).reshape(-1, 4)[:, 0]
    mv = frames.t["gb1_%d" % b].cpu().numpy().view(np.float32).reshape(-1, 2)
    image, motion = a.out + "_move.png", a.out + "_motion.png"
    api.save_image_sdr(image, beauty, w, h, api.sdr_config(brightness=1.0, tone_map=True, gamma=True))
    img = np.zeros((w * h, 4), np.float32)
    img[:, :2] = np.clip(0.5 + mv / 16.0, 0.0, 1.0)
    img[:, 2:] = (0.5, 1.0)
    api.save_image_sdr(motion, img, w, h, api.sdr_config(brightness=1.0, tone_map=False, gamma=False))
    is_wall, is_ground = g0 == (api.GBUFFER_DISPLACED | 1), g0 == api.GBUFFER_DISPLACED
    speed = np.hypot(mv[:, 0], mv[:, 1])
    print(json.dumps({"scene": "teapot on displaced ground, displaced wall translating by %g per frame" % a.step, "frames": a.move,
                      "wall_pixel_share": round(float(is_wall.mean()), 4),
                      "wall_motion_pixels": round(float(speed[is_wall].mean()), 3) if is_wall.any() else None,
                      "ground_motion_pixels": round(float(speed[is_ground].mean()), 5) if is_ground.any() else None,
                      "mean_radiance": round(float(beauty[:, :3].mean()), 5), "images": [image, motion]}))
    return 0


def scene_view(a):
    plain, (v, t, heights, gp), instances, pos, target = K.mixed_scene(a.size)
    gp.localIntersection = _local(a)
    ctx = api.Context(0)
    plain.upload(ctx)
    accel = ctx.accel_build()
    tf = api.Tfdm(ctx, v, t, heights, gp)
    # --nrtdsm: the last instance (the wall) is an NRTDSM object of the same mesh, map and height scale
    wall = api.Nrtdsm(ctx, v, t, heights, api.tfdm_params(h_scale=gp.hScale, tex_scale=(gp.texScale[0], gp.texScale[1]))) if a.nrtdsm else None
    if a.shell:         # ... or a shell object over the same mesh; one unit of shell height is half a tile high, as the shell view's default
        wall = api.Shell(ctx, v, t, [K.shell_geom(a.shell)], api.shell_params(h_scale=0.5 * K.extent(v), tex_scale=(a.tiles, a.tiles)))
    tset = api.TfdmSet(ctx)
    for k, (m, uid) in enumerate(instances):
        tset.add(wall if wall is not None and k == len(instances) - 1 else tf, m, uid)
    tset.commit()
    w, h = a.width, a.height_px
    n = w * h
    org, dirs = api.camera_rays(K.look_at_camera(w, h, pos, target), w, h)
    d_org, d_dir = torch.from_numpy(org).cuda(), torch.from_numpy(dirs).cuda()
    d_out = torch.zeros(n * 8, dtype=torch.int32, device="cuda")
    d_cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    d_part = torch.zeros(n * 4, dtype=torch.int32, device="cuda") if a.shell else None
    stream = torch.cuda.current_stream().cuda_stream
    ripple = Ripple(heights) if a.ripple else None
    for k in range(max(a.ripple, 1)):
        if ripple:
            ripple.apply(wall if wall is not None else tf, k, stream)
            tset.commit(stream)
            d_cnt.zero_()
        api.trace_scene(ctx, accel, tset, api.TRACE_CLOSEST, d_org.data_ptr(), d_dir.data_ptr(), n, d_out.data_ptr(), d_cnt.data_ptr(), stream=stream,
                        d_shell_part=d_part.data_ptr() if a.shell else 0)
    torch.cuda.synchronize()
    hits = d_out.cpu().numpy().view(api.SCENE_HIT_DTYPE)
    cnt = d_cnt.cpu().numpy()
    where = hits["where"]
    miss, is_plain = where == api.GFX_INVALID_SLOT, where == api.SCENE_PLAIN
    disp = ~miss & ~is_plain
    sdr = api.sdr_config(brightness=1.0, tone_map=False, gamma=False)
    img = np.zeros((n, 4), np.float32)
    img[:, 3] = 1
    img[is_plain, :3] = 0.5
    img[disp, :3] = hits["normal"][disp] * 0.5 + 0.5
    api.save_image_sdr(a.out + "_normal.png", img, w, h, sdr)
    api.save_image_sdr(a.out + "_depth.png", _depth_image(hits["dist"], ~miss, n), w, h, sdr)
    palette = np.array([(0.9, 0.3, 0.2), (0.2, 0.6, 0.9), (0.3, 0.8, 0.3), (0.9, 0.8, 0.2), (0.7, 0.3, 0.8), (0.2, 0.8, 0.8)], np.float32)
    ids = np.zeros((n, 4), np.float32)
    ids[:, 3] = 1
    ids[is_plain, :3] = 0.5
    ids[disp, :3] = palette[(where[disp] >> 1) % len(palette)]
    api.save_image_sdr(a.out + "_instance.png", ids, w, h, sdr)
    images = [a.out + "_normal.png", a.out + "_depth.png", a.out + "_instance.png"]
    if a.shell:
        part = d_part.cpu().numpy().view(api.SCENE_SHELL_PART_DTYPE)
        on_shell = disp & (tset.read()["pad0"][np.where(disp, where >> 1, 0)] == api.INSTANCE_SHELL)
        geo = np.zeros((n, 4), np.float32)
        geo[:, 3] = 1
        checker = 0.6 + 0.4 * ((part["tile"][on_shell, 0] + part["tile"][on_shell, 1]) & 1)
        geo[on_shell, :3] = palette[part["shellGeom"][on_shell] % len(palette)] * checker[:, None]
        api.save_image_sdr(a.out + "_geom.png", geo, w, h, sdr)
        images.append(a.out + "_geom.png")
    print(json.dumps({"scene": "teapot on displaced ground, displaced wall", "kinds": [int(k) for k in tset.read()["pad0"]], "size": int(heights.shape[0]), "instances": len(tset), "rays": n,
                      "plain_share": round(float(is_plain.mean()), 4),
                      "instance_shares": [round(float((disp & (where >> 1 == k)).mean()), 4) for k in range(len(tset))],
                      "miss_share": round(float(miss.mean()), 4), "aabb_tests_per_ray": round(float(cnt[0]) / n, 2),
                      "leaf_tests_per_ray": round(float(cnt[1]) / n, 2), "world_box_tests_per_ray": round(float(cnt[4]) / n, 2),
                      "traversals_per_ray": round(float(cnt[5]) / n, 2),
                      "images": images}))
    return 0


def shell_view(a):
    v, t, pos, target, up = K.base_mesh(a.mesh)
    geom = K.shell_geom(a.shell)
    # one unit of shell height is --scale tiles high: s = hScale / tiles
    gp = api.shell_params(h_scale=a.scale * K.extent(v), tex_scale=(a.tiles, a.tiles), tex_rotation=a.rotation)
    ctx = api.Context(0)
    sh = api.Shell(ctx, v, t, [geom], gp)
    w, h = a.width, a.height_px
    n = w * h
    org, dirs = api.camera_rays(K.look_at_camera(w, h, pos, target, up=up), w, h)
    d_org, d_dir = torch.from_numpy(org).cuda(), torch.from_numpy(dirs).cuda()
    d_out = torch.zeros(n * 12, dtype=torch.int32, device="cuda")
    d_cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    sh.trace(api.TRACE_CLOSEST, d_org.data_ptr(), d_dir.data_ptr(), n, d_out.data_ptr(), d_cnt.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    hits = d_out.cpu().numpy().view(api.SHELL_HIT_DTYPE)
    cnt = d_cnt.cpu().numpy()
    hit = hits["primIndex"] != api.GFX_INVALID_SLOT
    sdr = api.sdr_config(brightness=1.0, tone_map=False, gamma=False)
    img = np.zeros((n, 4), np.float32)
    img[:, 3] = 1
    img[hit, :3] = hits["normal"][hit] * 0.5 + 0.5
    api.save_image_sdr(a.out + "_normal.png", img, w, h, sdr)
    api.save_image_sdr(a.out + "_depth.png", _depth_image(hits["dist"], hit, n), w, h, sdr)
    palette = np.array([(0.9, 0.3, 0.2), (0.2, 0.6, 0.9), (0.3, 0.8, 0.3), (0.9, 0.8, 0.2), (0.7, 0.3, 0.8), (0.2, 0.8, 0.8), (0.8, 0.5, 0.2), (0.5, 0.5, 0.9)], np.float32)
    ids = np.zeros((n, 4), np.float32)
    ids[:, 3] = 1
    checker = 0.6 + 0.4 * ((hits["tile"][hit, 0] + hits["tile"][hit, 1]) & 1)
    ids[hit, :3] = palette[hits["shellGeom"][hit] % len(palette)] * checker[:, None]
    api.save_image_sdr(a.out + "_geom.png", ids, w, h, sdr)
    print(json.dumps({"query": "shell", "shell": a.shell, "mesh": a.mesh, "tiles": a.tiles, "shell_triangles": int(len(geom[1])), "triangles": int(len(t)), "rays": n,
                      "hit_share": round(float(hit.mean()), 4), "box_tests_per_ray": round(float(cnt[0]) / n, 2), "leaf_tests_per_ray": round(float(cnt[1]) / n, 2),
                      "base_triangles_per_ray": round(float(cnt[3]) / n, 2), "device_bytes": sh.device_bytes(),
                      "images": [a.out + "_normal.png", a.out + "_depth.png", a.out + "_geom.png"]}))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default=None, choices=["quad", "bunny", "teapot"])      # the quad; with --nrtdsm the teapot
    ap.add_argument("--height")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--scale", type=float, default=0.05)
    ap.add_argument("--level", type=int, default=0)
    mode = ap.add_mutually_exclusive_group()
    mode.add_argument("--box", action="store_true")
    mode.add_argument("--bilinear", action="store_true")
    ap.add_argument("--tex-scale", type=float, default=1.0)
    ap.add_argument("--rotation", type=float, default=0.0)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height-px", type=int, default=540)
    ap.add_argument("--out", default="tfdm_view")
    ap.add_argument("--nrtdsm", action="store_true")
    ap.add_argument("--shell", nargs="?", const="box", default=None, choices=["box", "bunny"])
    ap.add_argument("--tiles", type=float, default=16.0)
    ap.add_argument("--scene", action="store_true")
    ap.add_argument("--render", action="store_true")
    ap.add_argument("--restir", action="store_true")
    ap.add_argument("--regir", action="store_true")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--move", type=int, default=0)
    ap.add_argument("--step", type=float, default=0.02)
    ap.add_argument("--ripple", type=int, default=0)
    a = ap.parse_args()
    if a.mesh is None:
        a.mesh = "teapot" if a.nrtdsm and not a.scene else "quad"
    if a.move and not (a.scene and a.restir):
        ap.error("--move goes with --scene --restir")
    if a.ripple and (a.shell or a.move or a.height):
        ap.error("--ripple writes into the procedural height map of a TFDM or an NRTDSM object; it goes with neither --shell, --move nor --height")
    if a.regir and (not a.scene or a.restir or a.move or a.ripple):
        ap.error("--regir goes with --scene, and with neither --restir, --move nor --ripple")
    if a.render or a.restir or a.regir:
        if a.shell and a.nrtdsm:
            ap.error("--scene takes the wall as --nrtdsm or as --shell, not both")
        return scene_render(a)
    if a.scene:
        if a.shell and a.nrtdsm:
            ap.error("--scene takes the wall as --nrtdsm or as --shell, not both")
        return scene_view(a)
    if a.shell:
        if "--scale" not in sys.argv:
            a.scale = 0.5
        return shell_view(a)
    heights = api.tfdm_load_height(a.height) if a.height else K.procedural_map(a.size)
    v, t, pos, target, up = K.base_mesh(a.mesh)
    gp = api.tfdm_params(h_scale=a.scale * K.extent(v), tex_scale=(a.tex_scale, a.tex_scale), tex_rotation=a.rotation, target_mip_level=a.level,
                         local_intersection=_local(a))
    ctx = api.Context(0)
    if a.nrtdsm:
        if a.box or a.bilinear or a.level:
            ap.error("--nrtdsm has one local intersection and descends to level 0")
        tf = api.Nrtdsm(ctx, v, t, heights, gp)
    else:
        tf = api.Tfdm(ctx, v, t, heights, gp)
    w, h = a.width, a.height_px
    org, dirs = api.camera_rays(K.look_at_camera(w, h, pos, target, up=up), w, h)
    d_org, d_dir = torch.from_numpy(org).cuda(), torch.from_numpy(dirs).cuda()
    d_out = torch.zeros(w * h * 8, dtype=torch.int32, device="cuda")
    d_cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ripple = Ripple(heights) if a.ripple else None
    for k in range(max(a.ripple, 1)):
        if ripple:
            ripple.apply(tf, k, stream)
            d_cnt.zero_()
        tf.trace(api.TRACE_CLOSEST, d_org.data_ptr(), d_dir.data_ptr(), w * h, d_out.data_ptr(), d_cnt.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    hits = d_out.cpu().numpy().view(api.TFDM_HIT_DTYPE)
    cnt = d_cnt.cpu().numpy()
    hit = hits["primIndex"] != api.GFX_INVALID_SLOT
    img = np.zeros((w * h, 4), np.float32)
    img[:, 3] = 1
    img[hit, :3] = hits["normal"][hit] * 0.5 + 0.5
    sdr = api.sdr_config(brightness=1.0, tone_map=False, gamma=False)
    api.save_image_sdr(a.out + "_normal.png", img, w, h, sdr)
    depth = np.zeros((w * h, 4), np.float32)
    depth[:, 3] = 1
    if hit.any():
        d = hits["dist"][hit]
        depth[hit, :3] = (1.0 - 0.9 * (d - d.min()) / max(float(d.max() - d.min()), 1e-30))[:, None]
    api.save_image_sdr(a.out + "_depth.png", depth, w, h, sdr)
    print(json.dumps({"query": "nrtdsm" if a.nrtdsm else "tfdm", "mesh": a.mesh, "size": int(heights.shape[0]), "triangles": int(len(t)), "rays": w * h, "hit_share": round(float(hit.mean()), 4),
                      "aabb_tests_per_ray": round(float(cnt[0]) / (w * h), 2), "leaf_tests_per_ray": round(float(cnt[1]) / (w * h), 2),
                      "base_triangles_per_ray": round(float(cnt[3]) / (w * h), 2), "device_bytes": tf.device_bytes(),
                      "images": [a.out + "_normal.png", a.out + "_depth.png"]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
