"""SVGF denoiser (gfx_denoise, gfxexp_amd/csrc/denoise/denoise.hip): what the algorithm does, on the CPU restatement of its specification
(tests/denoise_ref.cpp; tests/test_gpu_denoise.py holds the kernels to it bit for bit), and the -denoise option of
restir_di_headless."""
import json
import subprocess

import numpy as np
import pytest

from gfxexp_amd import api, build
from tests import denoise_ref as ref


@pytest.fixture(scope="session")
def dn(tmp_path_factory):
    return ref.compile_ref(tmp_path_factory.mktemp("denoise_ref"))


class Settings:
    """The defaults of gfx_denoiser_default_settings (no library call: these tests need no build)."""

    def __init__(self, **kw):
        self.numStages, self.kernel, self.feedbackStage = 5, 0, 1
        self.sigmaZ, self.sigmaN, self.sigmaL, self.minAlpha = 1.0, 128.0, 4.0, 0.2
        for k, v in kw.items():
            setattr(self, k, v)


def _plane(w, h, n=(0.0, 0.0, 1.0), albedo=0.5):
    normal = np.zeros((h, w, 4), np.float32); normal[..., :3] = n; normal[..., 3] = 1
    alb = np.full((h, w, 4), albedo, np.float32); alb[..., 3] = 1
    return normal, alb


def _noisy(rng, light, albedo, sigma):
    beauty = np.zeros(albedo.shape, np.float32)
    beauty[..., :3] = (light * (1 + sigma * rng.standard_normal(albedo.shape[:2] + (1,)))).astype(np.float32) * albedo[..., :3]
    beauty[..., 3] = 1
    return beauty


def test_default_settings_match_the_header(built_lib):
    st = api.denoiser_default_settings()
    want = Settings()
    for f, _ in st._fields_:
        assert getattr(st, f) == pytest.approx(getattr(want, f)), f


def test_flat_plane_noise_drops_tenfold(dn):
    w = h = 48
    rng = np.random.default_rng(1)
    normal, alb = _plane(w, h)
    beauty = _noisy(rng, 1.0, alb, 0.3)
    zero = np.zeros((h, w, 2), np.float32)
    out, _ = ref.run(dn, w, h, Settings(), beauty, alb, normal, zero, None, True, ref.empty_history(w, h))
    out = out.reshape(h, w, 4)
    inner = (slice(4, -4), slice(4, -4))
    v_in, v_out = beauty[inner][..., 0].var(), out[inner][..., 0].var()
    assert v_out * 10 <= v_in, (v_in, v_out)
    assert abs(out[inner][..., 0].mean() - beauty[inner][..., 0].mean()) < 0.01 * beauty[inner][..., 0].mean()


@pytest.mark.parametrize("use_depth", [False, True])
def test_no_leak_across_a_crease(dn, use_depth):
    """Two planes at 90 degrees, lit 1 and unlit: the normal weight is pow(0, 128) = 0 across the edge."""
    w, h = 48, 32
    rng = np.random.default_rng(2)
    normal, alb = _plane(w, h)
    normal[:, w // 2:, :3] = (1.0, 0.0, 0.0)
    light = np.ones((h, w, 1), np.float32); light[:, w // 2:] = 0
    beauty = _noisy(rng, light, alb, 0.4)
    depth = np.full((h, w), 10.0, np.float32) if use_depth else None
    zero = np.zeros((h, w, 2), np.float32)
    out, _ = ref.run(dn, w, h, Settings(), beauty, alb, normal, zero, depth, True, ref.empty_history(w, h))
    out = out.reshape(h, w, 4)
    assert out[:, w // 2:w // 2 + 2, :3].max() < 0.01
    lit_in, lit_out = beauty[:, 2:w // 2, 0].mean(), out[:, 2:w // 2, 0].mean()
    assert abs(lit_out - lit_in) <= 0.01 * lit_in
    assert abs(out[:, w // 2:, 0].mean() - beauty[:, w // 2:, 0].mean()) <= 0.01 * 0.5   # both ~0: 1 % of the lit side's level


def _sequence(dn, frames, settings, shift=1, depth=None, first_every=None, mutate=None):
    w, h = 40, 24
    rng = np.random.default_rng(3)
    normal, alb = _plane(w, h)
    flow = np.zeros((h, w, 2), np.float32); flow[..., 0] = shift
    hist = ref.empty_history(w, h)
    for f in range(frames):
        beauty = _noisy(rng, 1.0, alb, 0.2)
        nrm = normal
        dep = depth
        if mutate:
            nrm, dep = mutate(f, normal.copy(), None if depth is None else depth.copy())
        first = f == 0 or (first_every is not None and f == first_every)
        _, hist = ref.run(dn, w, h, settings, beauty, alb, nrm, flow, dep, first, hist)
    return hist["length"].reshape(h, w)


def test_integer_flow_carries_history(dn):
    """flow = (1, 0): pixel x takes pixel x - 1's history, exactly one tap; lengths count up, the left column restarts."""
    lengths = _sequence(dn, 6, Settings(numStages=2))
    assert np.all(lengths[:, 0] == 1)
    for x in range(1, 40):
        assert np.all(lengths[:, x] == min(6, x + 1)), (x, lengths[:, x])


def test_normal_flip_depth_jump_and_first_frame_reset(dn):
    depth = np.full((24, 40), 5.0, np.float32)

    def flip(f, n, d):
        if f == 4:
            n[10:14, 10:20, 2] = -1.0
        return n, d

    def jump(f, n, d):
        if f == 4:
            d[10:14, 10:20] = 7.0
        return n, d

    for mutate, dep in ((flip, None), (jump, depth)):
        lengths = _sequence(dn, 5, Settings(), shift=0, depth=dep, mutate=mutate)
        assert np.all(lengths[10:14, 10:20] == 1)
        assert np.all(lengths[:10] == 5) and np.all(lengths[14:] == 5)
    lengths = _sequence(dn, 5, Settings(), shift=0, first_every=3)
    assert np.all(lengths == 2)


def test_zero_stages_is_demodulate_blend_remodulate(dn):
    w, h = 20, 12
    rng = np.random.default_rng(4)
    normal, alb = _plane(w, h)
    alb[..., :3] = rng.uniform(0.0, 1.0, (h, w, 3)).astype(np.float32)
    alb[0, :5, :3] = 0.0005                               # below the 1e-3 threshold: neither divided nor multiplied
    b0, b1 = (_noisy(rng, 1.0, alb, 0.5) for _ in range(2))
    b1[..., 3] = 0.25
    zero = np.zeros((h, w, 2), np.float32)
    st = Settings(numStages=0)
    o0, hist = ref.run(dn, w, h, st, b0, alb, normal, zero, None, True, ref.empty_history(w, h))
    o1, hist = ref.run(dn, w, h, st, b1, alb, normal, zero, None, False, hist)
    a = alb.reshape(-1, 4)[:, :3]
    big = a > np.float32(1e-3)
    demod = lambda b: np.where(big, b.reshape(-1, 4)[:, :3] / np.where(big, a, 1), b.reshape(-1, 4)[:, :3]).astype(np.float32)
    remod = lambda L: np.where(big, L * a, L).astype(np.float32)
    L0, L1 = demod(b0), demod(b1)
    assert np.array_equal(o0[:, :3].view(np.uint32), remod(L0).view(np.uint32))
    half = np.float32(0.5)                                 # n = 2: alpha = max(1/2, 0.2)
    blended = (half * L0 + half * L1).astype(np.float32)
    assert np.array_equal(o1[:, :3].view(np.uint32), remod(blended).view(np.uint32))
    assert np.all(o1[:, 3] == np.float32(0.25))
    assert np.all(hist["length"] == 2)


@pytest.mark.parametrize("use_depth", [False, True])
def test_background_passes_through_bit_for_bit(dn, use_depth):
    w, h = 24, 16
    rng = np.random.default_rng(5)
    normal, alb = _plane(w, h)
    beauty = rng.standard_normal((h, w, 4)).astype(np.float32) * 100
    depth = np.full((h, w), 3.0, np.float32)
    bg = np.zeros((h, w), bool); bg[:, :9] = True; bg[3, 15] = True
    if use_depth:
        depth[bg] = np.inf
    else:
        normal[bg, :3] = 0.0
    zero = np.zeros((h, w, 2), np.float32)
    for st in (Settings(), Settings(numStages=0), Settings(kernel=2, numStages=3)):
        out, hist = ref.run(dn, w, h, st, beauty, alb, normal, zero, depth if use_depth else None, True, ref.empty_history(w, h))
        out = out.reshape(h, w, 4)
        assert np.array_equal(out[bg].view(np.uint32), beauty[bg].view(np.uint32))
        assert np.all(hist["length"].reshape(h, w)[bg] == 0) and np.all(hist["length"].reshape(h, w)[~bg] == 1)
        assert np.all(np.isfinite(out[~bg]))


def test_emissive_pixels_pass_through_and_are_no_neighbour(dn):
    """An emitting surface (the emissive guide) is background: its beauty comes out unchanged, its history is invalid, and what it
    holds does not reach the other pixels -- the same output elsewhere whatever the emitter's beauty."""
    w, h = 32, 24
    rng = np.random.default_rng(6)
    normal, alb = _plane(w, h)
    beauty = _noisy(rng, 1.0, alb, 0.3)
    emissive = np.zeros((h, w), np.uint32); emissive[10:13, 14:18] = 1
    zero = np.zeros((h, w, 2), np.float32)
    depth = np.full((h, w), 4.0, np.float32)
    outs = []
    for glow in (50.0, 5e4):
        b = beauty.copy(); b[10:13, 14:18, :3] = glow
        for dep in (None, depth):
            out, hist = ref.run(dn, w, h, Settings(), b, alb, normal, zero, dep, True, ref.empty_history(w, h), emissive=emissive)
            out = out.reshape(h, w, 4)
            assert np.array_equal(out[10:13, 14:18].view(np.uint32), b[10:13, 14:18].view(np.uint32))
            assert np.all(hist["length"].reshape(h, w)[10:13, 14:18] == 0)
            outs.append(out)
    em = emissive.astype(bool)
    for k in (0, 1):
        assert np.array_equal(outs[k][~em].view(np.uint32), outs[k + 2][~em].view(np.uint32))
        assert outs[k][~em][:, :3].max() < 1.0                 # nothing of the 50 / 5e4 leaked into the plane lit at 0.5


def _cli(args):
    return subprocess.run([build.CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def test_cli_denoise_option(built_lib):
    scene = ["-name", "r", "-emittance", 5, 5, 5, "-rectangle", 1.0, 1.0, "-inst", "r", "-size", 64, 48, "-dry-run"]
    r = _cli(scene + ["-denoise", 3])
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout)["denoise_stages"] == 3
    r = _cli(["-denoise"] + scene)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout)["denoise_stages"] == 5
    assert "denoise_stages" not in json.loads(_cli(scene).stdout)
    for bad in ("6", "-1", "12"):
        r = _cli(scene + ["-denoise", bad])
        assert r.returncode != 0 and "-denoise" in r.stderr, (bad, r.stderr)
    r = _cli(scene + ["-renderer", "nrc", "-denoise"])
    assert r.returncode != 0
