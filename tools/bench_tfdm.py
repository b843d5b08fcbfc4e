"""gfx_tfdm_trace against the only other way to trace a height-mapped surface, the tessellated mesh in the scene BVH8.

    python tools/bench_tfdm.py [--size 1024] [--iters 20] [--width 1920] [--height 1080] [--step-timeout 300] [--variants a,b,...]

1920 x 1080 primary rays on a procedural size x size height map: on the unit quad and on the teapot (15 704 base triangles), for
the Box, the TwoTriangle and the Bilinear (Newton) local intersection at map levels 0 and 2; and the same quad rays through gfx_trace on the quad
tessellated to 2 x size x size triangles.  Per variant: microseconds per launch (HIP events around --iters launches after a
warm-up), Mrays/s, texel AABB tests / leaf tests / base triangles per ray from a counting launch of its own, and the device bytes
of either representation.  Beside them the crack-free NRTDSM query (gfx_nrtdsm_trace, "nrtdsm") on the same mesh, map and rays, with
its own device bytes.  --variants: only these (two_triangle_l0, box_l2, bilinear_l0, nrtdsm, ...), for a library that lacks one.
Shell mapping (gfx_shell_trace): the steps shell_box and shell_bunny trace the "One Box" and the 309-face bunny as shell meshes at
--tiles x --tiles (64) tiles on the quad, and the same tiles instantiated as ordinary triangles through gfx_trace on the same rays,
with the device bytes of either.  --steps: only these steps (tfdm_quad, tfdm_teapot, mesh_quad, shell_box, shell_bunny).
Prints one JSON line.

Every GPU step is a child process of its own under a time limit (--step-timeout seconds); the first step that fails or runs out of
time ends the run, and nothing more is started on the GPU after it."""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

STEPS = ["tfdm_quad", "tfdm_teapot", "mesh_quad", "shell_box", "shell_bunny"]
VARIANTS = [("two_triangle_l0", 1, 0), ("two_triangle_l2", 1, 2), ("box_l0", 0, 0), ("box_l2", 0, 2), ("bilinear_l0", 4, 0), ("bilinear_l2", 4, 2)]


def _arg(argv, name, default):
    return type(default)(argv[argv.index(name) + 1]) if name in argv else default


def timed(fn, iters, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def shell_step(name, tiles, iters, w, h):
    """gfx_shell_trace on the quad against gfx_trace on the same tiles instantiated as ordinary triangles."""
    import torch
    from gfxexp_amd import api
    import tfdm_common as K
    v, t, pos, target, up = K.base_mesh("quad")
    geom = K.shell_geom("box" if name == "shell_box" else "bunny")
    h_scale = 6.0 if name == "shell_box" else 1.0        # at 64 tiles: a box half a tile high, a bunny one tile high
    org, dirs = api.camera_rays(K.look_at_camera(w, h, pos, target, up=up), w, h)
    n = w * h
    d_org, d_dir = torch.from_numpy(org).cuda(), torch.from_numpy(dirs).cuda()
    d_out = torch.zeros(n * 12, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ctx = api.Context(0)
    sh = api.Shell(ctx, v, t, [geom], api.shell_params(h_scale=h_scale, tex_scale=(float(tiles), float(tiles))))
    secs = timed(lambda: sh.trace(api.TRACE_CLOSEST, d_org.data_ptr(), d_dir.data_ptr(), n, d_out.data_ptr(), stream=stream), iters)
    hits = d_out.cpu().numpy().view(api.SHELL_HIT_DTYPE)[:n]
    d_cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    sh.trace(api.TRACE_CLOSEST, d_org.data_ptr(), d_dir.data_ptr(), n, d_out.data_ptr(), d_cnt.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    cnt = d_cnt.cpu().numpy()
    shell_hit = hits["primIndex"] != api.GFX_INVALID_SLOT
    out = {"tiles": tiles, "shell_triangles": int(len(geom[1])), "rays": n,
           "shell": {"us": round(secs * 1e6, 1), "Mrays_per_s": round(n / secs / 1e6, 1), "hit_share": round(float(shell_hit.mean()), 4),
                     "box_tests_per_ray": round(float(cnt[0]) / n, 2), "leaf_tests_per_ray": round(float(cnt[1]) / n, 2),
                     "base_triangles_per_ray": round(float(cnt[3]) / n, 2), "device_bytes": sh.device_bytes()}}
    sh.close()
    mv, mt = K.instantiated_shell_on_quad(geom, tiles, h_scale)
    s = api.HostScene()
    g = s.add_geom(mv, mt, s.add_material_traditional((0.5, 0.5, 0.5), (0, 0, 0), 0.3))
    s.add_instance(s.add_group([g]), api.make_transform())
    s.upload(ctx)
    accel = ctx.accel_build()
    st = ctx.accel_stats(accel)
    d_hit = torch.zeros(n * 8, dtype=torch.int32, device="cuda")
    secs = timed(lambda: ctx.trace(accel, api.TRACE_CLOSEST, d_org.data_ptr(), d_dir.data_ptr(), n, d_hit.data_ptr(), stream=stream), iters)
    mesh_hit = d_hit.cpu().numpy().view(api.HIT_DTYPE)[:n]["triIndex"] != api.GFX_INVALID_SLOT
    out["mesh"] = {"triangles": int(len(mt)), "us": round(secs * 1e6, 1), "Mrays_per_s": round(n / secs / 1e6, 1), "hit_share": round(float(mesh_hit.mean()), 4),
                   "bvh_bytes": int(st["nodes"] * (64 + 16) + st["triRecords"] * (64 + 12)), "scene_geometry_bytes": int(mv.nbytes + mt.nbytes)}
    out["hit_or_miss_differs_share"] = round(float((mesh_hit != shell_hit).mean()), 6)
    out["memory_ratio_mesh_over_shell"] = round((out["mesh"]["bvh_bytes"] + out["mesh"]["scene_geometry_bytes"]) / out["shell"]["device_bytes"], 1)
    out["time_ratio_shell_over_mesh"] = round(out["shell"]["us"] / out["mesh"]["us"], 2)
    return out


def step(name, size, iters, w, h, only=None, tiles=64):
    import torch
    from gfxexp_amd import api
    import tfdm_common as K
    if name.startswith("shell_"):
        return shell_step(name, tiles, iters, w, h)
    heights = K.procedural_map(size)
    mesh = "teapot" if name == "tfdm_teapot" else "quad"
    v, t, pos, target, up = K.base_mesh(mesh)
    h_scale = 0.05 * K.extent(v) if mesh == "quad" else 0.01 * K.extent(v)
    org, dirs = api.camera_rays(K.look_at_camera(w, h, pos, target, up=up), w, h)
    n = w * h
    d_org, d_dir = torch.from_numpy(org).cuda(), torch.from_numpy(dirs).cuda()
    d_out = torch.zeros(n * 8, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ctx = api.Context(0)
    out = {"base_triangles": int(len(t)), "rays": n}
    if name == "mesh_quad":
        mv, mt = K.tessellated_quad(heights, h_scale)
        s = api.HostScene()
        g = s.add_geom(mv, mt, s.add_material_traditional((0.5, 0.5, 0.5), (0, 0, 0), 0.3))
        s.add_instance(s.add_group([g]), api.make_transform())
        s.upload(ctx)
        accel = ctx.accel_build()
        st = ctx.accel_stats(accel)
        secs = timed(lambda: ctx.trace(accel, api.TRACE_CLOSEST, d_org.data_ptr(), d_dir.data_ptr(), n, d_out.data_ptr(), stream=stream), iters)
        hits = d_out.cpu().numpy().view(api.HIT_DTYPE)[:n]
        d_cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
        ctx.trace(accel, api.TRACE_CLOSEST, d_org.data_ptr(), d_dir.data_ptr(), n, d_out.data_ptr(), d_counters=d_cnt.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        cnt = d_cnt.cpu().numpy()
        # 64-byte nodes and triangle records, a 16-byte link per node, 12 bytes of ids per record; and the scene's own vertex / index buffers
        out.update({"triangles": int(len(mt)), "us": round(secs * 1e6, 1), "Mrays_per_s": round(n / secs / 1e6, 1),
                    "hit_share": round(float((hits["triIndex"] != api.GFX_INVALID_SLOT).mean()), 4),
                    "bvh_bytes": int(st["nodes"] * (64 + 16) + st["triRecords"] * (64 + 12)), "scene_geometry_bytes": int(mv.nbytes + mt.nbytes),
                    "node_fetches_per_ray": round(float(cnt[0]) / n, 2), "triangle_fetches_per_ray": round(float(cnt[1]) / n, 2)})
        return out
    out["variants"] = {}
    tf = None
    for vname, local, level in VARIANTS:
        if only and vname not in only:
            continue
        gp = api.tfdm_params(h_scale=h_scale, target_mip_level=level, local_intersection=local)
        if tf is None:
            tf = api.Tfdm(ctx, v, t, heights, gp)
        else:
            tf.set_params(gp)
        secs = timed(lambda: tf.trace(api.TRACE_CLOSEST, d_org.data_ptr(), d_dir.data_ptr(), n, d_out.data_ptr(), stream=stream), iters)
        hits = d_out.cpu().numpy().view(api.TFDM_HIT_DTYPE)[:n]
        d_cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
        tf.trace(api.TRACE_CLOSEST, d_org.data_ptr(), d_dir.data_ptr(), n, d_out.data_ptr(), d_cnt.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        cnt = d_cnt.cpu().numpy()
        out["variants"][vname] = {"us": round(secs * 1e6, 1), "Mrays_per_s": round(n / secs / 1e6, 1),
                                  "hit_share": round(float((hits["primIndex"] != api.GFX_INVALID_SLOT).mean()), 4),
                                  "aabb_tests_per_ray": round(float(cnt[0]) / n, 2), "leaf_tests_per_ray": round(float(cnt[1]) / n, 2),
                                  "base_triangles_per_ray": round(float(cnt[3]) / n, 2)}
    if not only or "nrtdsm" in only:
        # the crack-free query (csrc/nrtdsm/) on the same mesh, map and rays: one variant, level 0
        nr = api.Nrtdsm(ctx, v, t, heights, api.tfdm_params(h_scale=h_scale))
        secs = timed(lambda: nr.trace(api.TRACE_CLOSEST, d_org.data_ptr(), d_dir.data_ptr(), n, d_out.data_ptr(), stream=stream), iters)
        hits = d_out.cpu().numpy().view(api.TFDM_HIT_DTYPE)[:n]
        d_cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
        nr.trace(api.TRACE_CLOSEST, d_org.data_ptr(), d_dir.data_ptr(), n, d_out.data_ptr(), d_cnt.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        cnt = d_cnt.cpu().numpy()
        out["nrtdsm"] = {"us": round(secs * 1e6, 1), "Mrays_per_s": round(n / secs / 1e6, 1),
                         "hit_share": round(float((hits["primIndex"] != api.GFX_INVALID_SLOT).mean()), 4),
                         "aabb_tests_per_ray": round(float(cnt[0]) / n, 2), "leaf_tests_per_ray": round(float(cnt[1]) / n, 2),
                         "base_triangles_per_ray": round(float(cnt[3]) / n, 2), "device_bytes": nr.device_bytes()}
        nr.close()
    if tf is None:
        return out
    out["device_bytes"] = tf.device_bytes()
    out["pyramid_and_heights_bytes"] = tf.size_of(api.TFDM_READ_PYRAMID, 0) * 4 // 3 + tf.size_of(api.TFDM_READ_HEIGHTS, 0) * 4 // 3
    return out


def main(argv):
    size, iters = _arg(argv, "--size", 1024), _arg(argv, "--iters", 20)
    w, h = _arg(argv, "--width", 1920), _arg(argv, "--height", 1080)
    only = _arg(argv, "--variants", "")
    tiles, steps = _arg(argv, "--tiles", 64), _arg(argv, "--steps", "")
    if "--step" in argv:
        print("STEP_RESULT " + json.dumps(step(argv[argv.index("--step") + 1], size, iters, w, h, only.split(",") if only else None, tiles)))
        return 0
    limit = _arg(argv, "--step-timeout", 300)
    result = {"metric": "tfdm_trace", "size": size, "iters": iters, "width": w, "height": h}
    for name in (steps.split(",") if steps else STEPS):
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, "--size", str(size), "--iters", str(iters),
               "--width", str(w), "--height", str(h), "--tiles", str(tiles)] + (["--variants", only] if only else [])
        r = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("STEP_RESULT ")]
        if r.returncode != 0 or not line:
            result["failed_step"] = {"name": name, "exit_status": r.returncode, "stderr_tail": r.stderr[-2000:]}
            print(json.dumps(result))
            return 1
        result[name] = json.loads(line[-1][len("STEP_RESULT "):])
    q, m = result.get("tfdm_quad", {}), result.get("mesh_quad", {})
    if "device_bytes" in q and m:
        result["memory_ratio_mesh_over_tfdm"] = round((m["bvh_bytes"] + m["scene_geometry_bytes"]) / q["device_bytes"], 2)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
