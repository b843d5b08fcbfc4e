"""The synthetic denoiser sequences of tests/denoise_cases.py on the CPU restatement alone (tests/denoise_ref.cpp): they reach the history
classes, the partly off-screen footprints, the length cap and the rounding of halves that tests/test_gpu_denoise_edges.py compares the
kernels on, so a comparison that passes there is not an empty one.  The coverage figures are conditions on the generator: if one fails,
the generator changes, not the figure."""
import numpy as np
import pytest

from tests import denoise_cases as cases
from tests import denoise_ref as ref


@pytest.fixture(scope="session")
def dn(tmp_path_factory):
    return ref.compile_ref(tmp_path_factory.mktemp("denoise_ref_cases"))


class Settings:
    """The defaults of gfx_denoiser_default_settings (no library call: these tests need no build)."""

    def __init__(self, **kw):
        self.numStages, self.kernel, self.feedbackStage = 5, 0, 1
        self.sigmaZ, self.sigmaN, self.sigmaL, self.minAlpha = 1.0, 128.0, 4.0, 0.2
        for k, v in kw.items():
            setattr(self, k, v)


def _run(dn, w, h, st, frames, with_depth, with_emissive, firsts=(0,)):
    """The restatement over a sequence: yields (f, frame, output, history written, history read)."""
    hist = ref.empty_history(w, h)
    for f, fr in enumerate(frames):
        beauty, albedo, normal, flow, depth, emissive = fr
        prev = hist
        out, hist = ref.run(dn, w, h, st, beauty, albedo, normal, flow, depth if with_depth else None, f in firsts, prev,
                            emissive=emissive.view(np.uint32) if with_emissive else None)
        yield f, fr, out, hist, prev


BIG = [s for s in cases.SIZES if min(s) >= 15]
GUIDES = [(True, True), (True, False), (False, True), (False, False)]


def test_the_generator_holds_what_it_says():
    for w, h in cases.SIZES:
        frames = cases.sequence(w, h)
        assert len(frames) == cases.FRAMES
        on_bound = above_bound = False                       # even one pixel meets both within the sequence
        for f, (beauty, albedo, normal, flow, depth, emissive) in enumerate(frames):
            n = w * h
            assert [a.shape for a in frames[f]] == [(n, 4), (n, 4), (n, 4), (n, 2), (n,), (n,)]
            assert all(a.dtype == np.float32 for a in frames[f][:5]) and emissive.dtype == np.int32
            assert np.isfinite(beauty).all() and np.isfinite(albedo).all() and np.isfinite(normal).all()
            assert not np.isnan(depth).any() and (np.isfinite(depth) | (depth == np.inf)).all()
            fx = np.array([cases.reprojected(p % w, flow[p, 0]) for p in range(n)])
            fy = np.array([cases.reprojected(p // w, flow[p, 1]) for p in range(n)])
            on_bound |= bool((fx == -1).any() or (fy == -1).any())
            above_bound |= bool((fx == np.nextafter(np.float32(-1), np.float32(0))).any() or
                                (fy == np.nextafter(np.float32(-1), np.float32(0))).any())
            if min(w, h) >= 15:
                for v, size in ((fx, w), (fy, h)):
                    assert (v == -1).any() and (v == np.nextafter(np.float32(-1), np.float32(0))).any()
                    assert ((v > -1) & (v < np.float32(-1 + 2.0 ** -22))).sum() > 2          # pixel 1 as well
                    assert ((v < size) & (v > size - 1) & (np.floor(v) == size - 1)).any()
                still = (flow == 0).all(axis=1).reshape(h, w)[2:-1, 2:-1]          # away from the border cases: 40 % less the far block
                assert still.mean() > 0.25 and np.isnan(flow).sum() == 1 and np.isinf(flow).sum() == 1
                assert ((flow[:, 0] == 40) & (flow[:, 1] == -25)).sum() >= 4
                a = albedo[:, :3]
                for v in cases.ALBEDO_EDGE:
                    assert (a == v).any()
                assert 0.01 < (a == cases.ALBEDO_EDGE[0]).any(axis=1).mean() < 0.12
                bg_d, bg_n = cases.background(frames[f], True, False), cases.background(frames[f], False, False)
                assert bg_d.any() and np.array_equal(bg_d, bg_n)
                assert (emissive != 0).any() and not (bg_d & (emissive != 0)).any()
                band = cases.layout(w, h)[0]
                assert set(np.unique(band)) == {0, 1, 2}
        assert on_bound and above_bound, (w, h)
        d01 = float(np.dot(cases.NORMALS[0].astype(np.float64), cases.NORMALS[1].astype(np.float64)))
        assert abs(d01 - 0.95) < 1e-6 and abs(np.dot(cases.NORMALS[2], cases.NORMALS[0])) == 0 and abs(np.dot(cases.NORMALS[2], cases.NORMALS[1])) == 0


@pytest.mark.parametrize("size", BIG, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("with_depth,with_emissive", GUIDES)
def test_sequences_cover_the_history_classes(dn, size, with_depth, with_emissive):
    w, h = size
    frames = cases.sequence(w, h)
    length = None
    for f, fr, out, hist, prev in _run(dn, w, h, Settings(numStages=0), frames, with_depth, with_emissive):
        if f > 0:
            sw, nf, partly = cases.reproject(w, h, fr, frames[f - 1], prev["length"], with_depth, with_emissive)
            # a footprint partly off screen yet accepted, in every frame after the first
            assert partly.any(), f
            # and the recomputation agrees with the restatement on every length
            want = cases.new_length(sw, nf)
            want[cases.background(fr, with_depth, with_emissive)] = 0
            assert np.array_equal(want, hist["length"])
        length = hist["length"]
    n = float(w * h)
    share = [(length == 0).sum(), (length == 1).sum() / n, ((length >= 2) & (length <= 3)).sum() / n, (length >= 4).sum() / n]
    print("%dx%d depth %d emissive %d: len 0: %d px, 1: %.1f %%, 2-3: %.1f %%, >= 4: %.1f %%" % (
        w, h, with_depth, with_emissive, share[0], 100 * share[1], 100 * share[2], 100 * share[3]))
    assert share[0] >= 1
    assert share[1] >= 0.02 and share[2] >= 0.02 and share[3] >= 0.02


@pytest.mark.parametrize("size", cases.SIZES, ids=lambda s: "%dx%d" % s)
def test_every_setting_ends_finite(dn, size):
    """Finite inputs (the flow's NaN and inf give no tap and reach no stored value): finite output and history at every size."""
    w, h = size
    frames = cases.sequence(w, h)
    for kw in cases.SETTINGS:
        for with_depth, with_emissive in GUIDES[::3]:
            for f, fr, out, hist, prev in _run(dn, w, h, Settings(**kw), frames, with_depth, with_emissive):
                assert np.isfinite(out).all() and np.isfinite(hist["lighting"]).all() and np.isfinite(hist["moments"]).all(), (kw, f)


def test_length_stops_at_255(dn):
    w, h = 9, 7
    frames = cases.cap_sequence(w, h)
    assert len(frames) == 258
    for f, fr, out, hist, prev in _run(dn, w, h, Settings(numStages=1), frames, True, False):
        assert np.all(hist["length"] == min(f + 1, 255)), f            # call f + 1: 254 after call 254, 255 from call 255 on
        assert np.isfinite(out).all()


def test_halves_round_away_from_zero(dn):
    w, h = 9, 7
    halves, even = 0, False
    for f, fr, out, hist, prev in _run(dn, w, h, Settings(numStages=1), cases.half_sequence(w, h), False, False):
        if f < cases.HALF_FLOW_FROM:
            continue
        sw, nf, _ = cases.reproject(w, h, fr, fr, prev["length"], False, False)
        assert np.all(sw > 0)
        mean = nf / sw
        k = np.floor(mean)
        half = mean - k == np.float32(0.5)
        if f == cases.HALF_FLOW_FROM:
            assert np.all(prev["length"].reshape(h, w)[:, :4] == 2) and np.all(prev["length"].reshape(h, w)[:, 4:] == 5)
            assert half.reshape(h, w)[:, 4].all() and np.all(mean.reshape(h, w)[:, 4] == np.float32(3.5))
        assert half.any(), f
        assert np.array_equal(hist["length"][half], (k[half] + 2).astype(np.uint32))          # k + 0.5 rounds to k + 1, then + 1
        assert np.array_equal(hist["length"], cases.new_length(sw, nf))
        halves += int(half.sum())
        even |= bool((k[half] % 2 == 0).any())
    assert halves >= h
    assert even                                            # a half above an even k: rounding ties to even would give k + 1 there


# ---------------------------------------------------------------- the invariants, here on the restatement's own output
@pytest.mark.parametrize("size", cases.SIZES, ids=lambda s: "%dx%d" % s)
def test_invariants_hold_on_the_restatement(dn, size):
    w, h = size
    frames = cases.sequence(w, h)
    seen = 0
    for with_depth, with_emissive in GUIDES:
        for kw in (dict(numStages=0), dict(numStages=5), dict(numStages=2, kernel=cases.GAUSS5X5)):
            for f, fr, out, hist, prev in _run(dn, w, h, Settings(**kw), frames, with_depth, with_emissive):
                seen += cases.check_background(fr, out, hist, with_depth, with_emissive)
        _, fr, out, hist, _ = next(_run(dn, w, h, Settings(numStages=0), frames, with_depth, with_emissive))
        assert cases.check_zero_stages_first_frame(fr, out, with_depth, with_emissive) > 0 or w * h < 4
        black = list(frames[0])
        black[1] = frames[0][1].copy(); black[1][:, :3] = 0.0
        for kernel in (cases.BOX3X3, cases.GAUSS3X3, cases.GAUSS5X5):
            st = Settings(numStages=1, feedbackStage=1, kernel=kernel)
            _, fr, out, hist, _ = next(_run(dn, w, h, st, [tuple(black)], with_depth, with_emissive))
            assert cases.check_one_stage_within_footprint(w, h, kernel, fr, hist, with_depth, with_emissive) > 0
    assert seen > 0 or w * h < 4
