"""Temporal anti-aliasing (gfx_taa_apply) on the configs[2] workload at 1920x1080: biased ReSTIR DI on the textured street stand-in
through api.RestirRenderer with jitter on, then the output chain (copy-to-linear, depth and emissive guides, the TAA flow).  With the
protocol of tools/bench_denoise.py (two rendered frames of a moving camera, applied alternately, the second frame's flows negated for
the way back) it times with HIP events, after a warm-up, at least 200 calls of gfx_taa_apply alone, of gfx_denoise alone and of the
gfx_denoise + gfx_taa_apply chain, and prints one JSON line: ms per call of each and the bytes per pixel of the TAA kernel from its
shape.  Under `rocprofv3 --kernel-trace --stats -- python tools/bench_taa.py` the per-kernel split is in rocprofv3's own stats file.
bench.py is not involved: its headline is the reference's frame without the output chain."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gfxexp_amd import api  # noqa: E402
from gfxexp_amd import scenes  # noqa: E402

AIM_MS = 0.040


def taa_bytes_per_pixel():
    """Bytes per pixel the TAA kernel moves, from its shape (not measured): the colour once (the 18 x 18 tile re-reads 27 % more,
    mostly from L2), the flow, about one float4 of unique history (the four taps of neighbouring pixels share lines), and two float4
    writes (output and history)."""
    return {"color": 16, "flow": 8, "history_unique": 16, "writes": 32, "total": 72}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--history-length", type=int, default=16)
    args = ap.parse_args()
    if args.calls < 200:
        ap.error("--calls must be at least 200")
    import torch
    W, H = 1920, 1080
    ctx = api.Context(0)
    scenes.bench_street(textured=True).upload(ctx)
    cfg = api.RestirRenderer.default_config(W, H, api.RENDERER_BIASED)
    cfg.camera = api.make_camera(W, H, pos=(1.5, 2.2, 52.0), pitch=4.0, yaw=181.5)
    cfg.enableJittering = 1
    r = api.RestirRenderer(ctx, cfg)
    den = api.Denoiser(ctx, W, H)
    taa = api.TemporalAA(ctx, W, H, args.history_length)
    n = W * H
    s = torch.cuda.current_stream().cuda_stream
    frames = []
    for k in range(2):
        r.set_camera(api.make_camera(W, H, pos=(1.5 + 0.4 * k, 2.2, 52.0 - 0.6 * k), pitch=4.0, yaw=181.5 + 0.7 * k))
        for _ in range(2):
            r.render_frame(s)
        sp, fp, cur, base, _ = r.params()
        ctx.restir_set_params(sp, fp, cur, base)
        b = [torch.zeros((n, c), dtype=torch.float32, device="cuda") for c in (4, 4, 4, 2, 1)] + [torch.zeros(n, dtype=torch.int32, device="cuda")]
        b.append(torch.zeros((n, 2), dtype=torch.float32, device="cuda"))
        ctx.restir_copy_to_linear(b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), b[3].data_ptr(), s)
        ctx.restir_copy_depth_to_linear(b[4].data_ptr(), s)
        ctx.restir_copy_emissive_to_linear(b[5].data_ptr(), s)
        ctx.restir_copy_taa_flow_to_linear(b[6].data_ptr(), s)
        frames.append(b)
    flows = [-frames[1][3], frames[1][3]]               # the denoiser's: the motion vectors
    taa_flows = [-frames[1][6], frames[1][6]]           # TAA's: without the jitter offset
    denoised = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    out = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    calls = [0]

    def call(mode, first=False):
        k = calls[0] % 2
        b = frames[k]
        if mode in ("denoise", "chain"):
            den.denoise(b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), flows[k].data_ptr(), denoised.data_ptr(), depth=b[4].data_ptr(),
                        emissive=b[5].data_ptr(), first=first, stream=s)
        if mode in ("taa", "chain"):
            color = denoised if mode == "chain" else b[0]
            taa.apply(color.data_ptr(), taa_flows[k].data_ptr(), out.data_ptr(), first=first, stream=s)
        calls[0] += 1

    def timed(mode):
        call(mode, first=True)
        for _ in range(args.warmup):
            call(mode)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            call(mode)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.calls

    ms = {mode: timed(mode) for mode in ("taa", "denoise", "chain")}
    model = taa_bytes_per_pixel()
    res = {"workload": "gfx_taa_apply, configs[2] frames (biased ReSTIR DI, textured street stand-in, jitter on) 1920x1080",
           "history_length": args.history_length, "calls": args.calls,
           "taa_ms_per_call": round(ms["taa"], 4), "taa_aim_ms": AIM_MS, "taa_within_aim": ms["taa"] <= AIM_MS,
           "denoise_ms_per_call": round(ms["denoise"], 4), "chain_ms_per_call": round(ms["chain"], 4),
           "taa_bytes_per_pixel_model": model,
           "taa_effective_TBps": round(model["total"] * n / (ms["taa"] * 1e-3) / 1e12, 3),
           "finite_output": bool(torch.isfinite(out).all()),
           "per_kernel": "not measured in-process: rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/bench_taa.py"}
    print(json.dumps(res))
    taa.close()
    den.close()
    r.close()


if __name__ == "__main__":
    main()
