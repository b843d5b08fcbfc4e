"""ReSTIR DI over a bound set of displaced instances, for an MI355X.

    python tools/bench_displaced_restir.py [--nrtdsm | --shell] [--size 1024] [--frames 20] [--width 1920] [--height 1080] [--step-timeout 300]

The scene of tfdm_common.lit_mixed_scene (tools/tfdm_view.py --scene under its emissive rectangle).  A frame is the G-buffer pass,
INITIAL_AND_TEMPORAL_BIASED (INITIAL_RIS in frame 0), two SPATIAL_BIASED passes and SHADING.

  displaced     the two quads as an instance set bound with GFX_DISPLACED_RESTIR: every shadow ray is the scene's any-hit query
  tessellated   the two quads tessellated into the BVH8 (two triangles per texel), "fuse_passes" 1: the same three-kernel form

With --nrtdsm / --shell one more row, the scene of tools/bench_scene_trace.py --nrtdsm / --shell: "displaced_nrtdsm" (the wall an NRTDSM
member) or "displaced_shell" (the wall the "One Box" shell at 64 x 64 tiles under a material of its own), the set bound through
gfx_scene_bind_displaced_kinds with GFX_DISPLACED_RESTIR; the result has "<row>_over_displaced_ms".

displaced / tessellated: milliseconds per frame (HIP events around --frames frames after 3 warm-up frames), per-kernel times of one
more frame from the context's timers, device bytes of the geometry (as tools/bench_displaced_render.py counts them).  Prints one JSON line.

    python tools/bench_displaced_restir.py --move [--size 1024] [--frames 20] [--width 1920] [--height 1080]

--move: the cost of the motion path.  Two steps over the displaced scene, each with one change of the wall's transform and one
gfx_tfdm_set_commit per frame inside the timed loop: "move" changes it with gfx_tfdm_set_move (the wall's pixels get a motion vector
and the temporal pass reprojects through it), "teleport" with gfx_tfdm_set_transform (no motion: the loop as it ran before moves
existed).  The wall translates by 0.01 per frame along x.  move_minus_teleport_ms is the difference of the two ms_per_frame.

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
MOVE_STEPS = ["move", "teleport"]
KIND_STEPS = {"--nrtdsm": "displaced_nrtdsm", "--shell": "displaced_shell"}
SHELL_TILES = 64            # tools/bench_scene_trace.py


def _arg(argv, name, default):
    return type(default)(argv[argv.index(name) + 1]) if name in argv else default


def _setup(size, tess, kind=None):
    from gfxexp_amd import api
    import tfdm_common as K
    hs, (v, t, heights, gp), instances, slot, pos, target = K.lit_mixed_scene(size, tessellate=tess)
    shell_mat = hs.add_material_traditional((0.8, 0.45, 0.25), (0.0, 0.0, 0.0), 0.0)
    ctx = api.Context(0)
    hs.upload(ctx)
    accel = ctx.accel_build()
    ctx.lights_build_static()
    stats = ctx.accel_stats(accel)
    out = {"bvh_triangles": stats["triangles"]}
    keep = None
    if tess:
        ctx.tunable_set("fuse_passes", 1)
        out["device_bytes"] = 64 * (stats["nodes"] + stats["triRecords"]) + 44 * (size + 1) ** 2 + 12 * 2 * size * size
    else:
        tf = api.Tfdm(ctx, v, t, heights, gp)
        wall = None         # the objects of tools/bench_scene_trace.py
        if kind == "displaced_nrtdsm":
            wall = api.Nrtdsm(ctx, v, t, heights, api.tfdm_params(h_scale=gp.hScale, tex_scale=(gp.texScale[0], gp.texScale[1])))
        if kind == "displaced_shell":
            wall = api.Shell(ctx, v, t, [api.shell_box()], api.shell_params(h_scale=8.0 / SHELL_TILES, tex_scale=(float(SHELL_TILES), float(SHELL_TILES))))
        tset = api.TfdmSet(ctx)
        for k, (m, uid) in enumerate(instances):
            tset.add(wall if wall is not None and k == len(instances) - 1 else tf, m, uid)
        tset.commit()
        if wall is None:
            ctx.bind_displaced(tset, [slot] * len(instances), restir=True)
        else:
            ctx.bind_displaced_kinds(tset, [slot] * (len(instances) - 1) + [(slot, [shell_mat]) if kind == "displaced_shell" else slot], restir=True)
        out["device_bytes"] = tf.device_bytes() + (wall.device_bytes() if wall is not None else 0) + api.TFDM_RECORD_BYTES * len(instances)
        keep = (tf, tset, instances)
    return ctx, accel, keep, pos, target, out


def step_frames(name, size, frames, w, h):
    import torch
    import tfdm_common as K
    ctx, accel, keep, pos, target, out = _setup(size, name == "tessellated", name if name in KIND_STEPS.values() else None)
    fr = K.RestirFrames(ctx, accel, w, h)
    cam = K.look_at_camera(w, h, pos, target)
    stream = torch.cuda.current_stream().cuda_stream
    change = None
    if name in MOVE_STEPS:
        import numpy as np
        tset = keep[1]
        wall = np.array(keep[2][1][0], np.float32)        # instance 1 of the scene: the wall

        def change(k):
            m = wall.copy()
            m[0, 3] += 0.01 * k
            (tset.move if name == "move" else tset.set_transform)(1, m)
            tset.commit(stream)
    for k in range(3):
        if change:
            change(k)
        fr.frame(k, cam, stream=stream)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(frames):
        if change:
            change(3 + k)
        fr.frame(3 + k, cam, stream=stream)
    b.record()
    b.synchronize()
    out["ms_per_frame"] = round(a.elapsed_time(b) / frames, 4)
    ctx.timing_enable(True)
    fr.frame(3 + frames, cam, stream=stream)
    torch.cuda.synchronize()
    out["kernel_ms"] = {k: round(ms, 4) for k, (ms, calls) in sorted(ctx.timing_collect().items())}
    ctx.timing_enable(False)
    out["mean_radiance"] = round(float(fr.beauty()[:, :3].mean()), 5)
    ctx.bind_displaced_kinds(None)
    return out


def main(argv):
    size, frames = _arg(argv, "--size", 1024), _arg(argv, "--frames", 20)
    w, h = _arg(argv, "--width", 1920), _arg(argv, "--height", 1080)
    if "--step" in argv:
        name = argv[argv.index("--step") + 1]
        print("STEP_RESULT " + json.dumps(step_frames(name, size, frames, w, h)))
        return 0
    limit = _arg(argv, "--step-timeout", 300)
    move = "--move" in argv
    result = {"metric": "displaced_restir_move" if move else "displaced_restir", "size": size, "frames": frames, "width": w, "height": h}
    steps = MOVE_STEPS if move else STEPS + [KIND_STEPS[f] for f in KIND_STEPS if f in argv]
    for name in steps:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, "--size", str(size), "--frames", str(frames),
               "--width", str(w), "--height", str(h)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("STEP_RESULT ")]
        if r.returncode != 0 or not line:
            result["failed_step"] = {"name": name, "exit_status": r.returncode, "stderr_tail": r.stderr[-2000:]}
            print(json.dumps(result))
            return 1
        result[name] = json.loads(line[-1][len("STEP_RESULT "):])
    if move:
        result["move_minus_teleport_ms"] = round(result["move"]["ms_per_frame"] - result["teleport"]["ms_per_frame"], 4)
        print(json.dumps(result))
        return 0
    result["tessellated_over_displaced_ms"] = round(result["tessellated"]["ms_per_frame"] / result["displaced"]["ms_per_frame"], 3)
    result["tessellated_over_displaced_bytes"] = round(result["tessellated"]["device_bytes"] / result["displaced"]["device_bytes"], 1)
    for name in steps[len(STEPS):]:
        result[name + "_over_displaced_ms"] = round(result[name]["ms_per_frame"] / result["displaced"]["ms_per_frame"], 3)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
