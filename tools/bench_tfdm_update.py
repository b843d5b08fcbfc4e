"""gfx_tfdm_update_heights / gfx_nrtdsm_update_heights against the only other way to a new height map, creating the object again.

    python tools/bench_tfdm_update.py [--size 1024] [--iters 20] [--runs 2] [--step-timeout 300] [--steps a,b,...] [--scene]

A size x size procedural map on the unit quad and on the teapot (15 704 base triangles), for TFDM (TwoTriangle) and NRTDSM.  Per
step and per rectangle (16 x 16, 128 x 128 and the whole map, each in the map's middle): the host wall time of one update_heights
call (the call is synchronous: it returns after the work on the stream is done), median / min / max over --iters calls after a
warm-up, and the same call's four phases by HIP events on the stream (gfx_timing_enable: value check, height mips + pyramid,
per-triangle boxes, refit), mean microseconds per call.  Beside it, in the same process, create: a new object from the new map on the
host (the host's mips included, which is what a caller without update_heights has to do), wall time, median / min / max.  All of it
--runs times over, so the spread between runs shows.

--scene: the frame time of the lit scene of tools/tfdm_view.py --scene --restir at 960 x 540 with one 128 x 128 update of the wall's
map + gfx_tfdm_set_commit per frame, against the same frames without them (wall time per frame over --iters frames, per run).

Steps: tfdm_quad, tfdm_teapot, nrtdsm_quad, nrtdsm_teapot, scene (only with --scene).  Prints one JSON line.  Every step is a child
process of its own under a time limit (--step-timeout seconds); the first step that fails or runs out of time ends the run, and
nothing more is started on the GPU after it."""
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

STEPS = ["tfdm_quad", "tfdm_teapot", "nrtdsm_quad", "nrtdsm_teapot"]
PHASES = ["tfdm_update_check", "tfdm_update_pyramid", "tfdm_update_prim", "tfdm_update_refit"]


def _arg(argv, name, default):
    return type(default)(argv[argv.index(name) + 1]) if name in argv else default


def _stats(seconds):
    a = np.asarray(seconds) * 1e6
    return {"median_us": round(float(np.median(a)), 1), "min_us": round(float(a.min()), 1), "max_us": round(float(a.max()), 1)}


def object_step(name, size, iters, runs):
    import torch
    from gfxexp_amd import api
    import tfdm_common as K
    kind, mesh = name.split("_")
    v, t, _, _, _ = K.base_mesh(mesh)
    heights = np.clip(K.procedural_map(size), 0, 1).astype(np.float32)
    gp = api.tfdm_params(h_scale=0.05 * K.extent(v))
    cls = api.Nrtdsm if kind == "nrtdsm" else api.Tfdm
    ctx = api.Context(0)
    obj = cls(ctx, v, t, heights, gp)
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(1)
    out = {"triangles": int(len(t)), "size": size, "device_bytes_before": obj.device_bytes(), "runs": []}
    for _ in range(runs):
        run = {}
        for side in (16, 128, size):
            side = min(side, size)
            x0 = y0 = (size - side) // 2
            srcs = [torch.from_numpy(np.clip(heights[y0:y0 + side, x0:x0 + side] + rng.uniform(-0.1, 0.1, (side, side)), 0, 1).astype(np.float32)).cuda() for _ in range(4)]
            torch.cuda.synchronize()
            for k in range(3):
                obj.update_heights(srcs[k % 4].data_ptr(), x0, y0, side, side, stream=stream)
            ctx.timing_collect()
            ctx.timing_enable(True)
            wall = []
            for k in range(iters):
                t0 = time.perf_counter()
                obj.update_heights(srcs[k % 4].data_ptr(), x0, y0, side, side, stream=stream)
                wall.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            phases = ctx.timing_collect()
            ctx.timing_enable(False)
            r = _stats(wall)
            r["phases_us"] = {p.replace("tfdm_update_", ""): round(1e3 * phases[p][0] / max(phases[p][1], 1), 1) for p in PHASES if p in phases}
            run["update_%dx%d" % (side, side)] = r
        new = np.clip(heights + rng.uniform(-0.1, 0.1, heights.shape), 0, 1).astype(np.float32)
        wall = []
        for k in range(max(iters // 4, 3) + 1):
            t0 = time.perf_counter()
            fresh = cls(ctx, v, t, new, gp)
            wall.append(time.perf_counter() - t0)
            fresh.close()
        run["create"] = _stats(wall[1:])
        out["runs"].append(run)
    out["device_bytes_after"] = obj.device_bytes()
    return out


def scene_step(size, iters, runs, w=960, h=540):
    import torch
    from gfxexp_amd import api
    import tfdm_common as K
    hs, (v, t, heights, gp), instances, slot, pos, target = K.lit_mixed_scene(size)
    heights = np.clip(heights, 0, 1).astype(np.float32)
    ctx = api.Context(0)
    hs.upload(ctx)
    accel = ctx.accel_build()
    ctx.lights_build_static()
    ground, wall = api.Tfdm(ctx, v, t, heights, gp), api.Tfdm(ctx, v, t, heights, gp)
    tset = api.TfdmSet(ctx)
    for k, (m, uid) in enumerate(instances):
        tset.add(wall if k == len(instances) - 1 else ground, m, uid)
    tset.commit()
    ctx.bind_displaced(tset, [slot] * len(instances), restir=True)
    frames = K.RestirFrames(ctx, accel, w, h)
    cam = K.look_at_camera(w, h, pos, target)
    stream = torch.cuda.current_stream().cuda_stream
    side = min(128, size)
    x0 = y0 = (size - side) // 2
    rng = np.random.default_rng(2)
    srcs = [torch.from_numpy(np.clip(heights[y0:y0 + side, x0:x0 + side] + rng.uniform(-0.1, 0.1, (side, side)), 0, 1).astype(np.float32)).cuda() for _ in range(4)]
    out = {"width": w, "height": h, "size": size, "runs": []}
    index = 0
    for _ in range(runs):
        run = {}
        for label, update in (("frame", False), ("frame_with_update_and_commit", True)):
            secs = []
            for k in range(iters + 3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if update:
                    wall.update_heights(srcs[k % 4].data_ptr(), x0, y0, side, side, stream=stream)
                    tset.commit(stream)
                frames.frame(index, cam, stream=stream, accumulate=False)
                torch.cuda.synchronize()
                if k >= 3:
                    secs.append(time.perf_counter() - t0)
                index += 1
            run[label] = _stats(secs)
        out["runs"].append(run)
    ctx.bind_displaced(None)
    return out


def child(argv):
    name = argv[argv.index("--child") + 1]
    size, iters, runs = _arg(argv, "--size", 1024), _arg(argv, "--iters", 20), _arg(argv, "--runs", 2)
    print(json.dumps(scene_step(size, iters, runs) if name == "scene" else object_step(name, size, iters, runs)))
    return 0


def main(argv):
    if "--child" in argv:
        return child(argv)
    steps = _arg(argv, "--steps", ",".join(STEPS + (["scene"] if "--scene" in argv else []))).split(",")
    limit = _arg(argv, "--step-timeout", 300)
    passed = [x for k in ("--size", "--iters", "--runs") if k in argv for x in (k, argv[argv.index(k) + 1])]
    result = {"bench": "tfdm_update", "steps": {}}
    for s in steps:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", s] + passed, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            result["failed"] = {"step": s, "why": "ran out of time (%d s)" % limit}
            break
        if r.returncode != 0:
            result["failed"] = {"step": s, "rc": r.returncode, "stderr": r.stderr[-2000:]}
            break
        result["steps"][s] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(result))
    return 1 if "failed" in result else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
