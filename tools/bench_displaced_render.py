"""Rendering displaced instances against rendering their tessellation, for an MI355X.

    python tools/bench_displaced_render.py [--regir] [--nrtdsm | --shell] [--size 1024] [--frames 20] [--width 1920] [--height 1080] [--max-len 5] [--step-timeout 300]

The scene of tfdm_common.lit_mixed_scene (a plain teapot on a displaced ground quad, a displaced wall behind it, an emissive
rectangle above, one size x size height map), G-buffer pass + baseline path tracer per frame:

  displaced     the two quads as a bound instance set (gfx_scene_bind_displaced): the scene query in every trace
  tessellated   the two quads tessellated into the BVH8 (two triangles per texel), rendered by the existing tracer with
                "fuse_passes" 1, so both sides run the same wavefront form

With --nrtdsm / --shell one more row, the scene of tools/bench_scene_trace.py --nrtdsm / --shell rendered:

  displaced_nrtdsm   the wall an NRTDSM member of the same mesh and map, the set bound through gfx_scene_bind_displaced_kinds
  displaced_shell    the wall a shell member (the "One Box" shell at 64 x 64 tiles, a material of its own), bound the same way: the
                     shell-aware renderer kernels and k_scene_instances_shell in every trace

and the result has "<row>_over_displaced_ms".

With --regir every row renders a ReGIR frame instead (build cells, temporal after frame 0; GFX_PT_PATH_TRACE_REGIR; update last access:
tfdm_common.RegirFrames) over a grid of 16 x 8 x 16 cells on the scene's bounds joined with the set's (gfx_tfdm_set_bounds), the
displaced rows through a binding that carries GFX_DISPLACED_REGIR; the metric is "displaced_render_regir".  Timing, kernel shares
and bytes as without it.

Per side: milliseconds per frame (HIP events around --frames frames after 3 warm-up frames), the per-kernel times of one more frame
from the context's timers, and the device bytes of the geometry (displaced: the object and the instance table; tessellated: BVH8
nodes and triangle records at 64 bytes each, plus the vertex and index pools).  Prints one JSON line.

Every GPU step is a child process of its own under a time limit (--step-timeout seconds); the first step that fails or runs out of
time ends the run, and nothing more is started on the GPU after it."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

STEPS = ["displaced", "tessellated"]
KIND_STEPS = {"--nrtdsm": "displaced_nrtdsm", "--shell": "displaced_shell"}
SHELL_TILES = 64            # tools/bench_scene_trace.py


def _arg(argv, name, default):
    return type(default)(argv[argv.index(name) + 1]) if name in argv else default


def step(name, size, frames, w, h, max_len, regir=False):
    import torch
    from gfxexp_amd import api
    import tfdm_common as K
    tess = name == "tessellated"
    hs, (v, t, heights, gp), instances, slot, pos, target = K.lit_mixed_scene(size, tessellate=tess)
    shell_mat = hs.add_material_traditional((0.8, 0.45, 0.25), (0.0, 0.0, 0.0), 0.0)
    ctx = api.Context(0)
    hs.upload(ctx)
    accel = ctx.accel_build()
    ctx.lights_build_static()
    stats = ctx.accel_stats(accel)
    out = {"bvh_triangles": stats["triangles"]}
    if tess:
        ctx.tunable_set("fuse_passes", 1)
        # BVH8 items, and one copy of the tessellated quad in the vertex and index pools ((size + 1)^2 vertices, 2 size^2 triangles)
        out["device_bytes"] = 64 * (stats["nodes"] + stats["triRecords"]) + 44 * (size + 1) ** 2 + 12 * 2 * size * size
    else:
        tf = api.Tfdm(ctx, v, t, heights, gp)
        wall = None         # the objects of tools/bench_scene_trace.py
        if name == "displaced_nrtdsm":
            wall = api.Nrtdsm(ctx, v, t, heights, api.tfdm_params(h_scale=gp.hScale, tex_scale=(gp.texScale[0], gp.texScale[1])))
        if name == "displaced_shell":
            wall = api.Shell(ctx, v, t, [api.shell_box()], api.shell_params(h_scale=8.0 / SHELL_TILES, tex_scale=(float(SHELL_TILES), float(SHELL_TILES))))
        tset = api.TfdmSet(ctx)
        for k, (m, uid) in enumerate(instances):
            tset.add(wall if wall is not None and k == len(instances) - 1 else tf, m, uid)
        tset.commit()
        if wall is None:
            ctx.bind_displaced(tset, [slot] * len(instances), regir=regir)
        else:
            ctx.bind_displaced_kinds(tset, [slot] * (len(instances) - 1) + [(slot, [shell_mat]) if name == "displaced_shell" else slot], regir=regir)
        out["device_bytes"] = tf.device_bytes() + (wall.device_bytes() if wall is not None else 0) + api.TFDM_RECORD_BYTES * len(instances)
    fr = K.RegirFrames(ctx, accel, w, h, K.joined_bounds(hs.bounds(), None if tess else tset)) if regir else K.PathTraceFrames(ctx, accel, w, h)
    cam = K.look_at_camera(w, h, pos, target)
    stream = torch.cuda.current_stream().cuda_stream
    for k in range(3):
        fr.frame(k, cam, max_len, stream)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(frames):
        fr.frame(3 + k, cam, max_len, stream)
    b.record()
    b.synchronize()
    out["ms_per_frame"] = round(a.elapsed_time(b) / frames, 4)
    ctx.timing_enable(True)
    fr.frame(3 + frames, cam, max_len, stream)
    torch.cuda.synchronize()
    out["kernel_ms"] = {k: round(ms, 4) for k, (ms, calls) in sorted(ctx.timing_collect().items())}
    ctx.timing_enable(False)
    out["mean_radiance"] = round(float(fr.beauty()[:, :3].mean()), 5)
    if not tess:
        ctx.bind_displaced_kinds(None)
    return out


def main(argv):
    size, frames, max_len = _arg(argv, "--size", 1024), _arg(argv, "--frames", 20), _arg(argv, "--max-len", 5)
    w, h = _arg(argv, "--width", 1920), _arg(argv, "--height", 1080)
    if "--step" in argv:
        print("STEP_RESULT " + json.dumps(step(argv[argv.index("--step") + 1], size, frames, w, h, max_len, "--regir" in argv)))
        return 0
    limit = _arg(argv, "--step-timeout", 300)
    result = {"metric": "displaced_render_regir" if "--regir" in argv else "displaced_render", "size": size, "frames": frames, "width": w, "height": h, "max_len": max_len}
    steps = STEPS + [KIND_STEPS[f] for f in KIND_STEPS if f in argv]
    for name in steps:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, "--size", str(size), "--frames", str(frames),
               "--width", str(w), "--height", str(h), "--max-len", str(max_len)] + (["--regir"] if "--regir" in argv else [])
        r = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("STEP_RESULT ")]
        if r.returncode != 0 or not line:
            result["failed_step"] = {"name": name, "exit_status": r.returncode, "stderr_tail": r.stderr[-2000:]}
            print(json.dumps(result))
            return 1
        result[name] = json.loads(line[-1][len("STEP_RESULT "):])
    result["tessellated_over_displaced_ms"] = round(result["tessellated"]["ms_per_frame"] / result["displaced"]["ms_per_frame"], 3)
    result["tessellated_over_displaced_bytes"] = round(result["tessellated"]["device_bytes"] / result["displaced"]["device_bytes"], 1)
    for name in steps[len(STEPS):]:
        result[name + "_over_displaced_ms"] = round(result[name]["ms_per_frame"] / result["displaced"]["ms_per_frame"], 3)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
