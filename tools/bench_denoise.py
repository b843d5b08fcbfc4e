"""The SVGF denoiser (gfx_denoise) on the configs[2] workload at 1920x1080: biased ReSTIR DI on the textured street stand-in through
api.RestirRenderer, then the output chain (copy-to-linear, depth and emissive guides) and the denoiser, default settings unless
given.  Times at least 200 gfx_denoise calls with HIP events after a warm-up, alternating two rendered frames of a moving camera,
and prints one JSON line: ms per call, bytes and VALU operations per pixel from the shapes; under `rocprofv3 --kernel-trace --stats -- python tools/bench_denoise.py` the per-kernel split
is in rocprofv3's own stats file.  bench.py is not involved: its headline is the reference's frame without the denoiser."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gfxexp_amd import api  # noqa: E402
from gfxexp_amd import scenes  # noqa: E402


def shape_model(st, with_depth):
    """Bytes moved and fp32 VALU operations per (surface) pixel, counted from the kernels' shapes (not measured)."""
    taps = 25 if st.kernel == api.DENOISE_GAUSS5X5 else 9
    temporal_bytes = 16 * 3 + 8 + (4 if with_depth else 0) + 4 * (4 + 16 + 16 + 8) + (16 + 8 + 4 + 16) + 16   # inputs, 4 taps, history, (L, var)
    stage_bytes = 2 * 16 + 16                     # the two 16-B records once per pixel from L2/LDS tiles, one 16-B write
    last_extra = 32                               # beauty + albedo in the last stage
    # per tap: bounds/background tests ~6, depth weight ~10 + gm_exp ~14, normal weight 5 + 7 squarings, luminance 5,
    # luminance weight ~4 + gm_exp ~14, accumulation 4 + 2 = ~71; per pixel: 3x3 variance ~30, gradient ~8, division / sqrt ~10
    tap_ops = 71 if with_depth else 47
    stage_ops = (taps - 1) * tap_ops + 48
    return {"bytes_per_pixel": temporal_bytes + st.numStages * stage_bytes + (last_extra if st.numStages else 0),
            "valu_ops_per_pixel": 80 + st.numStages * stage_ops, "taps_per_stage": taps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--stages", type=int, default=5)
    ap.add_argument("--kernel", type=int, default=0)
    ap.add_argument("--no-depth", action="store_true")
    args = ap.parse_args()
    import torch
    W, H = 1920, 1080
    ctx = api.Context(0)
    scenes.bench_street(textured=True).upload(ctx)
    cfg = api.RestirRenderer.default_config(W, H, api.RENDERER_BIASED)
    cfg.camera = api.make_camera(W, H, pos=(1.5, 2.2, 52.0), pitch=4.0, yaw=181.5)
    r = api.RestirRenderer(ctx, cfg)
    st = api.denoiser_default_settings()
    st.numStages, st.kernel = args.stages, args.kernel
    den = api.Denoiser(ctx, W, H, st)
    n = W * H
    s = torch.cuda.current_stream().cuda_stream
    # two rendered frames, the camera moved between them, denoised alternately: every call reprojects through real flow with
    # disocclusions (history lengths restart where the view changed), not a still frame whose history only grows
    frames = []
    for k in range(2):
        r.set_camera(api.make_camera(W, H, pos=(1.5 + 0.4 * k, 2.2, 52.0 - 0.6 * k), pitch=4.0, yaw=181.5 + 0.7 * k))
        for _ in range(2):
            r.render_frame(s)
        sp, fp, cur, base, _ = r.params()
        ctx.restir_set_params(sp, fp, cur, base)
        b = [torch.zeros((n, c), dtype=torch.float32, device="cuda") for c in (4, 4, 4, 2, 1)] + [torch.zeros(n, dtype=torch.int32, device="cuda")]
        ctx.restir_copy_to_linear(b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), b[3].data_ptr(), s)
        ctx.restir_copy_depth_to_linear(b[4].data_ptr(), s)
        ctx.restir_copy_emissive_to_linear(b[5].data_ptr(), s)
        frames.append(b)
    # frame 1's motion vectors lead back to frame 0; going from frame 1 to frame 0 uses them negated (an approximation: they are
    # frame 1's pixels' vectors, which is all a timing run needs)
    rev = -frames[1][3]
    out = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    flows = [rev, frames[1][3]]
    calls = [0]

    def call(first=False):
        k = calls[0] % 2
        b = frames[k]
        den.denoise(b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), flows[k].data_ptr(), out.data_ptr(),
                    depth=0 if args.no_depth else b[4].data_ptr(), emissive=b[5].data_ptr(), first=first, stream=s)
        calls[0] += 1

    call(first=True)
    for _ in range(args.warmup):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.calls):
        call()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / args.calls
    surface = float((frames[0][4] != float("inf")).float().mean())
    hist_len = den.history()["length"]
    lengths = np.frombuffer(ctx.read_device(hist_len, n * 4).tobytes(), np.uint32)
    out = {"workload": "gfx_denoise, configs[2] frame (biased ReSTIR DI, textured street stand-in) 1920x1080",
           "settings": {f: getattr(st, f) for f, _ in st._fields_}, "depth": not args.no_depth, "calls": args.calls,
           "ms_per_call": round(ms, 4), "surface_fraction": round(surface, 4),
           "history_fallback_fraction": round(float(((lengths > 0) & (lengths < 4)).mean()), 4),
           "per_kernel": "not measured in-process: rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/bench_denoise.py"}
    out.update(shape_model(st, not args.no_depth))
    print(json.dumps(out))
    den.close()
    r.close()


if __name__ == "__main__":
    main()
