"""Temporal anti-aliasing on the GPU (gfx_taa_apply, gfxexp_amd/csrc/denoise/taa.hip): bit parity of the output and of the history
with the CPU restatement of tests/taa_ref.cpp on random inputs and on rendered jittered frames (before and after gfx_denoise), the
argument checks, the anti-aliasing itself against an accumulated reference, and the -jitter / -taa options of restir_di_headless."""
import numpy as np
import pytest

from gfxexp_amd import api
from tests import taa_ref as ref
from tests import util
from tests.test_gpu_denoise import Frames

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="session")
def taa(tmp_path_factory):
    return ref.compile_ref(tmp_path_factory.mktemp("taa_ref_gpu"))


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _history_np(ctx, t, n):
    return ctx.read_device(t.history(), n * 16).view(np.float32).reshape(n, 4)


def _run_both(taa, ctx, w, h, frames, lengths, tag):
    """frames: (color float4[n], flow float2[n]) per call; lengths: historyLength per call (set_history_length when it changes).
    Runs every call through the GPU and the restatement and asserts bit equality of the output and of the history."""
    import torch
    n = w * h
    t = api.TemporalAA(ctx, w, h, lengths[0])
    out = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    hist = ref.empty_history(w, h)
    try:
        for f, ((color, flow), N) in enumerate(zip(frames, lengths)):
            if f > 0 and N != lengths[f - 1]:
                t.set_history_length(N)
            c, fl = _dev(color), _dev(flow)
            t.apply(c.data_ptr(), fl.data_ptr(), out.data_ptr(), first=f == 0, stream=_stream())
            torch.cuda.synchronize()
            want, hist = ref.run(taa, w, h, N, color, flow, f == 0, hist)
            util.assert_same_bits("%s frame %d N %d output" % (tag, f, N), out.cpu().numpy(), want)
            util.assert_same_bits("%s frame %d N %d history" % (tag, f, N), _history_np(ctx, t, n), hist)
        return hist
    finally:
        t.close()


def _random_frame(rng, w, h):
    color = rng.uniform(0.0, 3.0, (h * w, 4)).astype(np.float32)
    flow = rng.uniform(-2.5, 2.5, (h, w, 2)).astype(np.float32)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    # border cases: previous position exactly 0, just under W / H, just outside, far off screen, NaN, integer flow
    flow[:, 0, 0] = xx[:, 0] + 0.5                                  # P.x = 0
    flow[:, 1, 0] = xx[:, 1] + 0.5 - np.float32(w) + np.float32(1e-3)   # P.x just under W
    flow[0, :, 1] = yy[0] + 0.5 - np.float32(h) + np.float32(1e-3)      # P.y just under H
    flow[-1, :, 1] = yy[-1] + 0.5 + np.float32(1e-3)                   # P.y just below 0: off screen
    flow[5:9, 5:9] = (40.0, -25.0)
    flow[20, 20] = (np.nan, 0.0)
    flow[30:33, 40:60] = (2.0, -1.0)
    return color, flow.reshape(-1, 2)


def test_parity_random_odd_size(built_lib, taa):
    """97 x 61 (not a multiple of 16): fractional, border, off-screen and NaN flow; N 1, 16, 256 and changes mid-sequence."""
    w, h = 97, 61
    rng = np.random.default_rng(7)
    ctx = api.Context(0)
    frames = [_random_frame(rng, w, h) for _ in range(6)]
    for lengths in ([1] * 4, [16] * 6, [256] * 6, [16, 16, 1, 1, 256, 4]):
        _run_both(taa, ctx, w, h, frames[:len(lengths)], lengths, "random")


class TaaFrames(Frames):
    """Frames of test_gpu_denoise.py plus, per frame, the flow of gfx_restir_copy_taa_flow_to_linear (index 6)."""

    def render(self):
        import torch
        b = super().render()
        if len(b) == 6:
            b.append(torch.zeros((self.w * self.h, 2), dtype=torch.float32, device="cuda"))
        self.ctx.restir_copy_taa_flow_to_linear(b[6].data_ptr(), _stream())
        torch.cuda.synchronize()
        return b


@pytest.fixture(scope="module")
def jittered_street():
    fr = TaaFrames(160, 96, 6, enableJittering=1)
    yield fr
    fr.close()


def test_parity_jittered_street_beauty_and_denoised(built_lib, taa, jittered_street):
    """A 6-frame moving-camera street sequence with jitter: TAA on the noisy beauty and on gfx_denoise's output, through the flow of
    gfx_restir_copy_taa_flow_to_linear (and once through the G-buffer's motion vector)."""
    import torch
    fr = jittered_street
    w, h, n = fr.w, fr.h, fr.w * fr.h
    frames = [(f[0], f[6]) for f in fr.frames]
    assert np.abs(frames[1][1]).max() > 1.0                         # the camera moved
    _run_both(taa, fr.ctx, w, h, frames, [16] * 6, "beauty")
    _run_both(taa, fr.ctx, w, h, [(f[0], f[3]) for f in fr.frames], [16] * 6, "beauty, motion vector")
    den = api.Denoiser(fr.ctx, w, h)
    out = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    denoised = []
    try:
        for f, (beauty, albedo, normal, flow, depth, emissive, _) in enumerate(fr.frames):
            dv = [_dev(a) for a in (beauty, albedo, normal, flow, depth, emissive)]
            den.denoise(dv[0].data_ptr(), dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(), out.data_ptr(), depth=dv[4].data_ptr(),
                        emissive=dv[5].data_ptr(), first=f == 0, stream=_stream())
            torch.cuda.synchronize()
            denoised.append((out.cpu().numpy().copy(), fr.frames[f][6]))
    finally:
        den.close()
    _run_both(taa, fr.ctx, w, h, denoised, [16, 16, 16, 8, 8, 8], "denoised")


def test_parity_full_hd_pair(built_lib, taa):
    fr = TaaFrames(1920, 1080, 2, enableJittering=1)
    try:
        _run_both(taa, fr.ctx, fr.w, fr.h, [(f[0], f[6]) for f in fr.frames], [16, 16], "1080p")
    finally:
        fr.close()


def test_taa_flow_removes_the_jitter_offset(built_lib):
    """Static camera with jitter: the motion vector holds each pixel's jitter offset (up to half a pixel; on background pixels the
    projection of the view direction as a point), the TAA flow is ~0 everywhere.  Moving camera without jitter: on surfaces the
    TAA flow equals the motion vector up to rounding."""
    fr = TaaFrames(160, 96, 3, moving=False, bunny=True, enableJittering=1)
    try:
        _, _, _, mv, depth, _, tf = fr.frames[-1]
        surface = np.isfinite(depth.reshape(-1))
        assert 0.3 < np.abs(mv[surface]).max() <= 0.501 and np.abs(mv[~surface]).max() > 1.0
        assert np.abs(tf).max() < 1e-3, np.abs(tf).max()
    finally:
        fr.close()
    fr = TaaFrames(160, 96, 3)
    try:
        _, _, _, mv, depth, _, tf = fr.frames[-1]
        surface = np.isfinite(depth.reshape(-1))
        assert np.abs(mv[surface]).max() > 1.0                                      # the camera moved
        assert np.abs(tf[surface] - mv[surface]).max() < 1e-2
        assert np.all(np.isfinite(tf))
    finally:
        fr.close()


def test_bad_arguments_launch_nothing(built_lib):
    import torch
    w, h = 32, 16
    n = w * h
    ctx = api.Context(0)
    L = api.lib()
    t = api.TemporalAA(ctx, w, h)
    color = torch.rand((n, 4), dtype=torch.float32, device="cuda")
    flow = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    out = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    t.apply(color.data_ptr(), flow.data_ptr(), out.data_ptr(), first=True, stream=_stream())
    torch.cuda.synchronize()
    hp = t.history()
    before = _history_np(ctx, t, n).copy()
    out.fill_(7.0)
    c, f, o = color.data_ptr(), flow.data_ptr(), out.data_ptr()
    C = api.C
    bad = [(t.inputs(c, f, width=w + 1), o), (t.inputs(c, f, height=h - 1), o), (t.inputs(0, f), o), (t.inputs(c, 0), o),
           (t.inputs(c, f), 0), (t.inputs(c, f), c), (t.inputs(c, f), hp)]
    for inp, dst in bad:
        assert L.gfx_taa_apply(ctx.h, None, t.h, C.byref(inp), 0, C.c_void_p(dst or None)) == 1
    assert L.gfx_taa_apply(ctx.h, None, t.h, None, 0, C.c_void_p(o)) == 1
    assert L.gfx_taa_apply(ctx.h, None, None, C.byref(t.inputs(c, f)), 0, C.c_void_p(o)) == 1
    torch.cuda.synchronize()
    assert torch.all(out == 7.0)
    assert t.history() == hp                                        # no call went through: the history did not flip
    assert np.array_equal(_history_np(ctx, t, n), before)
    for bad_n in (0, 257):
        assert L.gfx_taa_set_history_length(t.h, C.c_uint32(bad_n)) == 1
        h_ = C.c_void_p()
        assert L.gfx_taa_create(ctx.h, C.c_uint32(w), C.c_uint32(h), C.c_uint32(bad_n), C.byref(h_)) == 1 and not h_.value
    for size in ((0, h), (w, 0), (16385, 4)):
        h_ = C.c_void_p()
        assert L.gfx_taa_create(ctx.h, C.c_uint32(size[0]), C.c_uint32(size[1]), C.c_uint32(16), C.byref(h_)) == 1
    assert L.gfx_taa_set_history_length(t.h, C.c_uint32(256)) == 0 and L.gfx_taa_set_history_length(t.h, C.c_uint32(1)) == 0
    t.close()


# quality: the renderer of test_gpu_denoise.py's quality test (bunny scene, static camera, 1 spp, default biased ReSTIR) with jitter.
# Measured on an MI355X: noisy / TAA 10.4 and SVGF / (SVGF + TAA) 10.4 at frame 32; asserted with 2x margin.
QUALITY_FRAME = 32
TAA_RATIO_FLOOR = 5.0
SVGF_TAA_RATIO_FLOOR = 5.0


def test_taa_lowers_the_error(built_lib):
    """Static camera, jitter on, 1 spp, no accumulation, TAA through gfx_restir_copy_taa_flow_to_linear's flow: at frame 32 the TAA
    output (N = 16) is closer (MSE over the image) to the mean of 1024 jittered frames than the noisy frame 32, by at least
    TAA_RATIO_FLOOR, and SVGF + TAA closer than SVGF alone by at least SVGF_TAA_RATIO_FLOOR.  The ratios are printed."""
    import torch
    w, h = 160, 96
    n = w * h
    fr = TaaFrames(w, h, 0, moving=False, bunny=True, enableJittering=1)
    d = api.Denoiser(fr.ctx, w, h)
    t_noisy, t_den = api.TemporalAA(fr.ctx, w, h, 16), api.TemporalAA(fr.ctx, w, h, 16)
    bufs = [torch.zeros((n, 4), dtype=torch.float32, device="cuda") for _ in range(3)]    # denoised, TAA(beauty), TAA(denoised)
    acc = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    try:
        for f in range(1024):
            b = fr.render()
            s = _stream()
            if f < QUALITY_FRAME:
                d.denoise(b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), b[3].data_ptr(), bufs[0].data_ptr(), depth=b[4].data_ptr(),
                          emissive=b[5].data_ptr(), first=f == 0, stream=s)
                t_noisy.apply(b[0].data_ptr(), b[6].data_ptr(), bufs[1].data_ptr(), first=f == 0, stream=s)
                t_den.apply(bufs[0].data_ptr(), b[6].data_ptr(), bufs[2].data_ptr(), first=f == 0, stream=s)
                fr.r.outputs_consumed(s)
                if f == QUALITY_FRAME - 1:
                    torch.cuda.synchronize()
                    shots = [b[0][:, :3].double().clone()] + [x[:, :3].double().clone() for x in bufs]
            acc += b[0].double()
        torch.cuda.synchronize()
        mean = acc[:, :3] / 1024
        noisy, den, taa_noisy, taa_den = (float(((x - mean) ** 2).mean()) for x in shots)
        print("TAA MSE at frame %d: noisy %.4g, TAA %.4g (ratio %.2f); SVGF %.4g, SVGF + TAA %.4g (ratio %.2f)"
              % (QUALITY_FRAME, noisy, taa_noisy, noisy / taa_noisy, den, taa_den, den / taa_den))
        assert taa_noisy * TAA_RATIO_FLOOR <= noisy, (noisy, taa_noisy)
        assert taa_den * SVGF_TAA_RATIO_FLOOR <= den, (den, taa_den)
    finally:
        t_noisy.close()
        t_den.close()
        d.close()
        fr.close()


@pytest.mark.parametrize("opts", [["-jitter", "-taa", 16], ["-denoise", "-taa"]])
def test_cli_taa_writes_a_finite_image(built_lib, tmp_path, opts):
    from tests.test_headless_cli import _read_pfm, _run, _scene_args
    out = str(tmp_path / "taa.pfm")
    d = _run(_scene_args() + ["-size", 160, 96, "-frames", 4, "-out", out] + opts)
    assert d["taa_ms"] > 0 and d["taa_history_length"] == 16
    if "-denoise" in opts:
        assert d["denoise_ms"] > 0
    img = _read_pfm(out)
    assert img.shape == (96, 160, 3) and np.all(np.isfinite(img)) and img.max() > 0
