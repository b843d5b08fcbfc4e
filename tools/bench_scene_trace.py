"""gfx_trace_scene against the chain of calls it replaces.

    python tools/bench_scene_trace.py [--nrtdsm | --shell] [--size 1024] [--iters 20] [--width 1920] [--height 1080] [--step-timeout 300]

1920 x 1080 primary rays on the scene of tfdm_common.mixed_scene (a plain teapot on a displaced ground quad, a displaced wall behind
it, one size x size height map):

  call    one gfx_trace_scene
  call_bilinear   the same call with the wall an instance of a GFX_TFDM_BILINEAR object of the same mesh and map (the ground stays
          TwoTriangle): the set then runs the Bilinear-capable instance phase
  chain   gfx_trace, then per instance a ray transform on the user's side (torch), gfx_tfdm_trace with tmax = the best distance so
          far, and a merge (torch): what a caller had to do before

With --nrtdsm the steps are

  call_nrtdsm    one gfx_trace_scene on the set whose wall is an NRTDSM member (gfx_tfdm_set_add_nrtdsm) of the same mesh and map:
                 the mixed instance phase, k_scene_instances_mixed
  chain_nrtdsm   the chain that call replaces: gfx_trace, then per member the torch ray transform, gfx_tfdm_trace (the ground) or
                 gfx_nrtdsm_trace (the wall) with tmax = the best distance so far, and the torch merge

both in the same run, and the result has "chain_nrtdsm_over_call_nrtdsm".  With --shell they are

  call_shell     one gfx_trace_scene on the set whose wall is a shell member (gfx_tfdm_set_add_shell): the "One Box" shell at
                 64 x 64 tiles over the wall's mesh; the ground stays TFDM.  The instance phase is k_scene_instances_shell
  chain_shell    the chain that call replaces: gfx_trace, then per member the torch ray transform, gfx_tfdm_trace (the ground) or
                 gfx_shell_trace (the wall, 48-byte hits) with tmax = the best distance so far, and the torch merge

and the result has "chain_shell_over_call_shell".

Per step: microseconds per launch (HIP events around --iters launches after 3 warm-up launches), Mrays/s; for the call the
traversal counters per ray from a counting launch of its own; and whether both agree on hit or miss and on the distance (the
chain's torch transform is not the library's arithmetic to the bit, so the comparison is a tolerance, not the tests' equality).
Prints one JSON line.  The kernel shares come from a separate run:

    rocprofv3 --kernel-trace --stats -- python tools/bench_scene_trace.py --step call

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

STEPS = ["call", "call_bilinear", "chain"]
NRTDSM_STEPS = ["call_nrtdsm", "chain_nrtdsm"]
SHELL_STEPS = ["call_shell", "chain_shell"]
SHELL_TILES = 64


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


def step(name, size, iters, w, h):
    import torch
    from gfxexp_amd import api
    import tfdm_common as K
    plain, (v, t, heights, gp), instances, pos, target = K.mixed_scene(size)
    ctx = api.Context(0)
    plain.upload(ctx)
    accel = ctx.accel_build()
    tf = api.Tfdm(ctx, v, t, heights, gp)
    tset = api.TfdmSet(ctx)
    smooth = None
    if name == "call_bilinear":
        gp_smooth = api.tfdm_params(h_scale=gp.hScale, tex_scale=(gp.texScale[0], gp.texScale[1]), local_intersection=api.TFDM_BILINEAR)
        smooth = api.Tfdm(ctx, v, t, heights, gp_smooth)
    if name in NRTDSM_STEPS:
        smooth = api.Nrtdsm(ctx, v, t, heights, api.tfdm_params(h_scale=gp.hScale, tex_scale=(gp.texScale[0], gp.texScale[1])))
    if name in SHELL_STEPS:         # the box is about as high as a tile is wide (tests/shell_host.py quad_box: 2.0 at 4 tiles)
        smooth = api.Shell(ctx, v, t, [api.shell_box()], api.shell_params(h_scale=8.0 / SHELL_TILES, tex_scale=(float(SHELL_TILES), float(SHELL_TILES))))
    objects = [smooth if smooth is not None and k == len(instances) - 1 else tf for k in range(len(instances))]
    for obj, (m, uid) in zip(objects, instances):
        tset.add(obj, m, uid)
    tset.commit()
    n = w * h
    org, dirs = api.camera_rays(K.look_at_camera(w, h, pos, target), w, h)
    d_org, d_dir = torch.from_numpy(org).cuda(), torch.from_numpy(dirs).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    out = {"rays": n, "instances": len(tset), "plain_triangles": plain.counts()["triangles"]}
    d_scene = torch.zeros(n * 8, dtype=torch.int32, device="cuda")

    def call():
        api.trace_scene(ctx, accel, tset, api.TRACE_CLOSEST, d_org.data_ptr(), d_dir.data_ptr(), n, d_scene.data_ptr(), stream=stream)

    if name in ("call", "call_bilinear", "call_nrtdsm", "call_shell"):
        secs = timed(call, iters)
        d_cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
        api.trace_scene(ctx, accel, tset, api.TRACE_CLOSEST, d_org.data_ptr(), d_dir.data_ptr(), n, d_scene.data_ptr(), d_cnt.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        cnt = d_cnt.cpu().numpy()
        where = d_scene.cpu().numpy().view(api.SCENE_HIT_DTYPE)["where"]
        disp = where < api.SCENE_PLAIN
        out.update({"us": round(secs * 1e6, 1), "Mrays_per_s": round(n / secs / 1e6, 1),
                    "instance_shares": [round(float((disp & (where >> 1 == k)).mean()), 4) for k in range(len(tset))],
                    "plain_share": round(float((where == api.SCENE_PLAIN).mean()), 4), "miss_share": round(float((where == api.GFX_INVALID_SLOT).mean()), 4),
                    "aabb_tests_per_ray": round(float(cnt[0]) / n, 2), "leaf_tests_per_ray": round(float(cnt[1]) / n, 2),
                    "base_triangles_per_ray": round(float(cnt[3]) / n, 2), "world_box_tests_per_ray": round(float(cnt[4]) / n, 2),
                    "traversals_per_ray": round(float(cnt[5]) / n, 2)})
        return out
    # the chain: the user's side of it in torch
    table = tset.read()
    w2o = [torch.from_numpy(table[k]["worldToObj"].reshape(3, 4).copy()).cuda() for k in range(len(table))]
    d_plain = torch.zeros(n * 4, dtype=torch.int32, device="cuda")
    words = [12 if isinstance(o, api.Shell) else 8 for o in objects]       # a gfx_shell_hit is 48 bytes
    d_hit = torch.zeros(n * max(words), dtype=torch.int32, device="cuda")
    d_oo, d_od = torch.empty_like(d_org), torch.empty_like(d_dir)
    best = torch.empty(n, dtype=torch.float32, device="cuda")
    where = torch.empty(n, dtype=torch.int32, device="cuda")

    def chain():
        ctx.trace(accel, api.TRACE_CLOSEST, d_org.data_ptr(), d_dir.data_ptr(), n, d_plain.data_ptr(), stream=stream)
        ph = d_plain.view(n, 4)
        plain_hit = ph[:, 3] != -1
        torch.where(plain_hit, ph[:, 0].view(torch.float32), d_dir[:, 3], out=best)
        where.copy_(torch.where(plain_hit, torch.full_like(where, -2), torch.full_like(where, -1)))
        for k, m in enumerate(w2o):
            d_oo[:, :3] = d_org[:, :3] @ m[:, :3].T + m[:, 3]
            d_oo[:, 3] = d_org[:, 3]
            d_od[:, :3] = d_dir[:, :3] @ m[:, :3].T
            d_od[:, 3] = best
            objects[k].trace(api.TRACE_CLOSEST, d_oo.data_ptr(), d_od.data_ptr(), n, d_hit.data_ptr(), stream=stream)
            th = d_hit[:n * words[k]].view(n, words[k])
            win = th[:, 3] != -1
            torch.where(win, th[:, 0].view(torch.float32), best, out=best)
            where.copy_(torch.where(win, torch.full_like(where, k), where))

    secs = timed(chain, iters)
    call()
    torch.cuda.synchronize()
    scene = d_scene.cpu().numpy().view(api.SCENE_HIT_DTYPE)
    cw, cb = where.cpu().numpy(), best.cpu().numpy()
    sw = np.where(scene["where"] == api.GFX_INVALID_SLOT, -1, np.where(scene["where"] == api.SCENE_PLAIN, -2, (scene["where"] >> 1).astype(np.int64)))
    same = sw == cw
    both = same & (sw != -1)
    out.update({"us": round(secs * 1e6, 1), "Mrays_per_s": round(n / secs / 1e6, 1), "same_winner_share": round(float(same.mean()), 6),
                "worst_relative_distance_difference": float((np.abs(scene["dist"][both] - cb[both]) / np.maximum(1.0, cb[both])).max()) if both.any() else None})
    return out


def main(argv):
    size, iters = _arg(argv, "--size", 1024), _arg(argv, "--iters", 20)
    w, h = _arg(argv, "--width", 1920), _arg(argv, "--height", 1080)
    if "--step" in argv:
        print("STEP_RESULT " + json.dumps(step(argv[argv.index("--step") + 1], size, iters, w, h)))
        return 0
    limit = _arg(argv, "--step-timeout", 300)
    result = {"metric": "scene_trace", "size": size, "iters": iters, "width": w, "height": h}
    steps = NRTDSM_STEPS if "--nrtdsm" in argv else SHELL_STEPS if "--shell" in argv else STEPS
    for name in steps:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, "--size", str(size), "--iters", str(iters),
               "--width", str(w), "--height", str(h)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("STEP_RESULT ")]
        if r.returncode != 0 or not line:
            result["failed_step"] = {"name": name, "exit_status": r.returncode, "stderr_tail": r.stderr[-2000:]}
            print(json.dumps(result))
            return 1
        result[name] = json.loads(line[-1][len("STEP_RESULT "):])
    if steps is NRTDSM_STEPS:
        result["chain_nrtdsm_over_call_nrtdsm"] = round(result["chain_nrtdsm"]["us"] / result["call_nrtdsm"]["us"], 3)
    elif steps is SHELL_STEPS:
        result["chain_shell_over_call_shell"] = round(result["chain_shell"]["us"] / result["call_shell"]["us"], 3)
    else:
        result["chain_over_call"] = round(result["chain"]["us"] / result["call"]["us"], 3)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
