"""-m gpu: the launch plan of every pass -- which kernels one frame's passes launch and how often, as the timers of
gfx_timing_collect count them -- against tests/golden/launch_plans.json.

The bit-exact tests cannot see a sequencer that renders the right image through the wrong form (the wavefront form instead of the
one-kernel form, a launch too many); this can.  The golden was recorded once, with the library built from the sources BEFORE the
host sequencing of pathtrace.hip / restir.hip was split up, by running this module as a script:

    python -m tests.test_gpu_launch_plan tests/golden/launch_plans.json

The test never rewrites it.  A case is a function that returns {step: {timer name: calls}}; a step whose launch carries no timer
(GFX_PT_NRC_COUNT_QUERIES: one untimed single-thread kernel) is recorded as {} and so only pins that nothing timed runs in it.  A
case's contexts are released when it returns (api.Context.__del__; the test collects garbage after each case).  The scenes are the bunny scene at
96 x 64 (352 x 256 for path regeneration, as test_path_regeneration_changes_no_pixel) and the displaced worlds of
tests/test_gpu_displaced_regir.py."""
import gc
import json
import os
import sys

import pytest

from gfxexp_amd import api
from tests import util

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_plans.json")
W, H = 96, 64

# The two size thresholds that choose a form under "fuse_passes" 0, for the 256 CUs of an MI355X and the default pixel map
# (64 x 64-pixel supertiles of 16 blocks, their number rounded up to a multiple of 8: restir_common.hip.h make_pixel_grid).
#   pathtrace_launch `small`:        launchWaves <= waveSlots + waveSlots / 2 with waveSlots = 256 * 16 = 4096 and four waves per block:
#                                    launchBlocks <= 1536 = 96 supertiles.   768 x 512 is 12 x 8 = 96, 832 x 512 is 13 x 8 = 104.
#   restir_launch `fusableLaunch`:   2 * launchWaves <= 9 * waveSlots with waveSlots = 256 * 4 * 4 = 4096:
#                                    launchBlocks <= 4608 = 288 supertiles.  1152 x 1024 is 18 x 16 = 288, 1216 x 1024 is 19 x 16 = 304.
PT_SMALL_AT, PT_SMALL_ABOVE = (768, 512), (832, 512)
RESTIR_FUSABLE_AT, RESTIR_FUSABLE_ABOVE = (1152, 1024), (1216, 1024)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _plan(ctx):
    """The launches since the last call: {timer name: calls}."""
    import torch
    torch.cuda.synchronize()
    return {name: int(calls) for name, (_, calls) in sorted(ctx.timing_collect().items())}


class Rig:
    """One context over the bunny scene with every per-pixel buffer on the device, timing enabled."""

    def __init__(self, w=W, h=H, tunables=None, regir=False, nrc=False):
        self.w, self.h = w, h
        self.ctx = ctx = api.Context(0)
        for name, value in (tunables or {}).items():
            ctx.tunable_set(name, value)
        self.hs = hs = util.bunny_scene()
        hs.upload(ctx)
        self.accel = ctx.accel_build()
        ctx.lights_build_static()
        self.cam = api.make_camera(w, h, pos=(1.5, 5.0, 14.0), pitch=12.0, yaw=186.0)
        self.dev = util.DeviceBuffers(util.PixelBuffers(w, h))
        self.s = self.dev.static_params()
        self.rb = self.nb = None
        if regir:
            self.rb = util.RegirBuffers(hs.bounds(), (8, 4, 8))
            ctx.regir_set_params(self.rb.device_params())
        if nrc:
            self.nb = util.NrcBuffers(w, h, hs.bounds())
            self.nb.to_device()
        ctx.timing_enable(True)

    def params(self, frame=0, cur=0, base=0, **kw):
        base_kw = dict(frameIndex=frame, bufferIndex=frame % 2, resetFlowBuffer=int(frame == 0), numAccumFrames=0)
        base_kw.update(kw)
        self.f = util.frame_params(api.GfxRestirFrameParams, api.GfxCamera, self.w, self.h, self.cam, travHandle=self.accel, **base_kw)
        self.ctx.lights_build_instances(_stream())
        self.ctx.restir_set_params(self.s, self.f, cur, base, _stream())
        if self.nb is not None:
            self.ctx.nrc_set_render_params(self.nb.device_params(12345, 54321, frame == 0))
        _plan(self.ctx)                  # (what the light build launched is not part of a pass)

    def pt(self, pass_id, max_len=0, rows=(0, 0)):
        self.ctx.pt_launch(pass_id, self.w, self.h, max_len, rows[0], rows[1], _stream())
        return _plan(self.ctx)

    def restir(self, pass_id, cur=0, base=0):
        self.ctx.restir_set_params(self.s, self.f, cur, base, _stream())
        self.ctx.restir_launch(pass_id, self.w, self.h, _stream())
        return _plan(self.ctx)


# ---------------------------------------------------------------- baseline path tracer
def _baseline(w, h, max_len, **tunables):
    def run():
        r = Rig(w, h, tunables)
        r.params()
        return {"gbuffer": r.pt(api.PT_SETUP_GBUFFERS), "path trace": r.pt(api.PT_PATH_TRACE_BASELINE, max_len)}
    return run


# ---------------------------------------------------------------- ReGIR
def _regir(**tunables):
    def run():
        r = Rig(W, H, tunables, regir=True)
        out = {}
        for frame in range(2):           # the second frame builds its cells with temporal reuse: the four ReGIR pass ids in all
            r.params(frame)
            build = api.PT_REGIR_BUILD_CELLS_TEMPORAL if frame else api.PT_REGIR_BUILD_CELLS
            for tag, pass_id in (("gbuffer", api.PT_SETUP_GBUFFERS), ("build cells", build), ("path trace", api.PT_PATH_TRACE_REGIR),
                                 ("update last access", api.PT_REGIR_UPDATE_LAST_ACCESS)):
                out["frame %d %s" % (frame, tag)] = r.pt(pass_id, 5)
        return out
    return run


# ---------------------------------------------------------------- NRC
def _restir_passes_before_the_nrc_tracer(r, out):
    """Initial RIS and two biased spatial passes, as tests/test_gpu_nrc_render.py sequences them; returns the reservoir they end in."""
    cur = 0
    out["restir initial"] = r.restir(api.PASS_INITIAL_RIS, cur, 0)
    for i in range(2):
        out["restir spatial %d" % i] = r.restir(api.PASS_SPATIAL_BIASED, cur, 5 * i)
        cur = (cur + 1) % 2
    r.ctx.restir_set_params(r.s, r.f, cur, 10, _stream())


def _nrc_tracer(nee, max_len):
    """nee: 0 the tracer's own light sample, 1 ReGIR, 2 the ReSTIR reservoirs.  max_len 0: unlimited bounces, the live count read
    back every fourth bounce."""
    def run():
        r = Rig(W, H, None, regir=nee == 1, nrc=True)
        r.params()
        out = {"gbuffer": r.pt(api.PT_SETUP_GBUFFERS, max_len)}
        if nee == 1:
            out["build cells"] = r.pt(api.PT_REGIR_BUILD_CELLS, max_len)
        if nee == 2:
            _restir_passes_before_the_nrc_tracer(r, out)
        out["preprocess"] = r.pt(api.PT_NRC_PREPROCESS, max_len)
        out["path trace"] = r.pt((api.PT_PATH_TRACE_NRC, api.PT_PATH_TRACE_NRC_REGIR, api.PT_PATH_TRACE_NRC_RESTIR)[nee], max_len)
        return out
    return run


def _nrc_small_passes():
    r = Rig(W, H, None, nrc=True)
    r.params()
    out = {"gbuffer": r.pt(api.PT_SETUP_GBUFFERS), "preprocess": r.pt(api.PT_NRC_PREPROCESS), "path trace": r.pt(api.PT_PATH_TRACE_NRC, 3)}
    for tag, pass_id in (("accumulate", api.PT_NRC_ACCUMULATE), ("propagate", api.PT_NRC_PROPAGATE), ("shuffle", api.PT_NRC_SHUFFLE),
                         ("visualize", api.PT_NRC_VISUALIZE_PREDICTION), ("count queries", api.PT_NRC_COUNT_QUERIES)):
        out[tag] = r.pt(pass_id)
    out["accumulate rows 16..48"] = r.pt(api.PT_NRC_ACCUMULATE, 0, (16, 48))     # the one small pass that honours a row band
    return out


# ---------------------------------------------------------------- ReSTIR
ORIGINAL_PASSES = (("gbuffer", api.PASS_SETUP_GBUFFERS), ("initial", api.PASS_INITIAL_RIS), ("initial + temporal biased", api.PASS_INITIAL_TEMPORAL_BIASED),
                   ("initial + temporal unbiased", api.PASS_INITIAL_TEMPORAL_UNBIASED), ("spatial biased", api.PASS_SPATIAL_BIASED),
                   ("spatial unbiased", api.PASS_SPATIAL_UNBIASED), ("shading", api.PASS_SHADING), ("spatial biased + shading", api.PASS_SPATIAL_BIASED_AND_SHADING))
REARCH_PASSES = (("light presampling", api.PASS_LIGHT_PRESAMPLING), ("per-pixel RIS", api.PASS_PER_PIXEL_RIS)) + \
    tuple(("trace shadow rays %d" % k, api.PASS_TRACE_SHADOW_RAYS + k) for k in range(7)) + \
    tuple(("shade and resample %d" % k, api.PASS_SHADE_AND_RESAMPLE + k) for k in range(4))


def _restir_every_pass(fuse):
    def run():
        r = Rig(W, H, {"fuse_passes": fuse})
        out = {}
        r.params(0)
        out["gbuffer frame 0"] = r.restir(api.PASS_SETUP_GBUFFERS)
        r.params(1)                      # a second frame, so that the temporal passes have a previous one
        for tag, pass_id in ORIGINAL_PASSES:
            out[tag] = r.restir(pass_id)
        r.params(1, numSpatialNeighbors=1)
        for tag, pass_id in REARCH_PASSES:
            out[tag] = r.restir(pass_id)
        return out
    return run


def _restir_initial(**tunables):
    def run():
        r = Rig(W, H, tunables)
        r.params()
        return {"gbuffer": r.restir(api.PASS_SETUP_GBUFFERS), "initial": r.restir(api.PASS_INITIAL_RIS)}
    return run


def _restir_gbuffer(fuse):
    def run():
        r = Rig(W, H, {"fuse_passes": fuse})
        r.params()
        return {"gbuffer": r.restir(api.PASS_SETUP_GBUFFERS)}
    return run


def _restir_frame(w, h):
    def run():
        r = Rig(w, h)
        r.params()
        return {tag: r.restir(pass_id) for tag, pass_id in (("gbuffer", api.PASS_SETUP_GBUFFERS), ("initial", api.PASS_INITIAL_RIS),
                                                            ("spatial biased", api.PASS_SPATIAL_BIASED), ("shading", api.PASS_SHADING))}
    return run


# ---------------------------------------------------------------- a bound displaced set
def _displaced(kinds):
    """The plain bound set of tests/test_gpu_displaced_regir.py World, or its KWorld (a kinds binding over a set with a shell member),
    bound with GFX_DISPLACED_REGIR: G-buffer, baseline tracer, the ReGIR passes."""
    def run():
        from tests import test_gpu_displaced_kinds as DK
        from tests import test_gpu_displaced_regir as G
        from tests import test_gpu_displaced_render as DR
        world = G.KWorld() if kinds else G.World()
        cam = DK.CAMS[0] if kinds else DR.camera(0)
        ctx = world.ctx
        try:
            world.bind(world.sc.set, regir=True)
            fr = G.Regir(world.sc, world.bounds)
            ctx.timing_enable(True)
            fr.params(0, cam)
            _plan(ctx)
            out = {}
            for tag, pass_id, max_len in (("gbuffer", api.PT_SETUP_GBUFFERS, 0), ("baseline", api.PT_PATH_TRACE_BASELINE, 3),
                                          ("build cells", api.PT_REGIR_BUILD_CELLS, 0), ("regir", api.PT_PATH_TRACE_REGIR, 3),
                                          ("update last access", api.PT_REGIR_UPDATE_LAST_ACCESS, 0)):
                fr.launch(pass_id, max_len)
                out[tag] = _plan(ctx)
            return out
        finally:
            world.unbind()
    return run


CASES = {
    "baseline fuse_passes 2": _baseline(W, H, 5, fuse_passes=2),
    "baseline fuse_passes 1 path length 1": _baseline(W, H, 1, fuse_passes=1),
    "baseline fuse_passes 1 path length 2": _baseline(W, H, 2, fuse_passes=1),
    "baseline fuse_passes 1 path length 5": _baseline(W, H, 5, fuse_passes=1),
    "baseline pt_regen 1": _baseline(352, 256, 5, fuse_passes=2, pt_regen=1),
    "baseline fuse_passes 0 at the small-launch threshold": _baseline(*PT_SMALL_AT, 2),
    "baseline fuse_passes 0 above the small-launch threshold": _baseline(*PT_SMALL_ABOVE, 2),
    "regir fused": _regir(fuse_passes=2),
    "regir wavefront pt_overlap 0": _regir(fuse_passes=1, pt_overlap=0),
    "regir wavefront pt_overlap 1": _regir(fuse_passes=1, pt_overlap=1),
    "nrc max_len 3": _nrc_tracer(0, 3),
    "nrc max_len 0": _nrc_tracer(0, 0),
    "nrc regir max_len 3": _nrc_tracer(1, 3),
    "nrc regir max_len 0": _nrc_tracer(1, 0),
    "nrc restir max_len 3": _nrc_tracer(2, 3),
    "nrc restir max_len 0": _nrc_tracer(2, 0),
    "nrc small passes": _nrc_small_passes,
    "restir every pass fuse_passes 1": _restir_every_pass(1),
    "restir every pass fuse_passes 2": _restir_every_pass(2),
    "restir candidate_split 1": _restir_initial(fuse_passes=1, candidate_split=1),
    "restir candidate_split 2": _restir_initial(fuse_passes=1, candidate_split=2),
    "restir candidate_split 4": _restir_initial(fuse_passes=1, candidate_split=4),
    "restir candidate_split 1 fused": _restir_initial(fuse_passes=2, candidate_split=1),
    "restir candidate_split 2 fused": _restir_initial(fuse_passes=2, candidate_split=2),
    "restir candidate_split 4 fused": _restir_initial(fuse_passes=2, candidate_split=4),
    "restir candidate_prefilter 0": _restir_initial(fuse_passes=1, candidate_prefilter=0),
    "restir candidate_prefilter 1": _restir_initial(fuse_passes=1, candidate_prefilter=1),
    "restir gbuffer fuse_passes 1": _restir_gbuffer(1),
    "restir gbuffer fuse_passes 2": _restir_gbuffer(2),
    "restir fuse_passes 0 at the fusable threshold": _restir_frame(*RESTIR_FUSABLE_AT),
    "restir fuse_passes 0 above the fusable threshold": _restir_frame(*RESTIR_FUSABLE_ABOVE),
    "displaced plain bound set": _displaced(False),
    "displaced kinds binding with a shell member": _displaced(True),
}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_names_exactly_the_cases():
    with open(GOLDEN) as f:
        assert sorted(json.load(f)) == sorted(CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_launch_plan(built_lib, golden, case):
    got = CASES[case]()
    gc.collect()
    assert got == golden[case], "%s\n got  %s\n want %s" % (case, json.dumps(got, sort_keys=True), json.dumps(golden[case], sort_keys=True))


if __name__ == "__main__":
    out = {}
    for name in sorted(CASES):
        out[name] = CASES[name]()
        print(name, json.dumps(out[name], sort_keys=True), flush=True)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
