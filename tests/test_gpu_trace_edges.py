"""-m gpu: the adversarial trace cases of tests/trace_cases.py on the HIP LBVH -> BVH8 build and its traversal (k_trace, and
trace_wave_local inside the one-kernel path tracer).  For every scene and ray set: closest hits equal the oracle's brute force bit
for bit and any hits its occlusion, on every ray whose brute-force answer a traversal can decide (trace_cases.decidable; no
traversal reports a hit nearer than the brute force on the others), and the GPU agrees with the float64 reference on every robust
ray.  The deep nest makes k_trace spill its LDS stack; a transform update deepens a split tree in place."""
import ctypes

import numpy as np
import pytest

from gfxexp_amd import api
from tests import trace_cases as tc
from tests import util
from tests.test_gpu_pathtrace import run_pt_both
from tests.trace_cases import SCENES, STATES, all_rays, flat_hits, oracle_for

pytestmark = pytest.mark.gpu

DEEP_MIN_LEVELS = 15
# pinhole rays through the corner the nest converges to: a 0.002-degree field from 0.7 units away passes within ~2e-5 of it (level 15 and deeper)
NEST_CAM, NEST_LOOK = (-0.4, -0.35, -0.45), (1e-6, 1.2e-6, 0.8e-6)


def build(case, ctx, final=False, upload=True):
    """The case's scene on the GPU (animated instances declared, the leaf size set); final=True: then the transform update."""
    if upload:
        case.hs.upload(ctx)
    for slot in case.dynamic:
        ctx.instance_set_dynamic(slot)
    if case.max_leaf:
        ctx.accel_set_max_leaf(case.max_leaf)
    accel = ctx.accel_build()
    if final:
        for slot, xfm in case.moves.items():
            ctx.instance_set_transform(slot, xfm)
        assert ctx.accel_build(handle=accel) == accel
    return accel


def check_rays(case, ctx, accel, osc, ref, org, dirs, what, counters=False):
    """GPU closest / any hit of one ray set against the brute force and the float64 reference -> (robust hits, robust misses, counters)."""
    brute = osc.trace(2, org, dirs)
    dec = tc.decidable(case, org, dirs, flat_hits(brute), brute["dist"])
    gpu, cnt = util.gpu_trace(ctx, accel, api.TRACE_CLOSEST, org, dirs, counters=True) if counters else \
        (util.gpu_trace(ctx, accel, api.TRACE_CLOSEST, org, dirs), None)
    ids = util.accel_tri_ids(ctx, accel)
    util.compare_closest(gpu[dec], ids, brute[dec], osc.tri_ids(), f"{what} vs brute force")
    assert not np.any(gpu["dist"] < brute["dist"]), f"{what}: a closest hit nearer than the brute force"
    occ = util.gpu_trace(ctx, accel, api.TRACE_ANY, org, dirs)
    want = (brute["triIndex"] != api.GFX_INVALID_SLOT).astype(np.uint32)
    assert np.array_equal(occ[dec], want[dec]), f"{what}: any hit differs on {np.count_nonzero(occ[dec] != want[dec])} rays"
    hit = gpu["triIndex"] != api.GFX_INVALID_SLOT
    flat = np.full(len(org), -1, np.int64)
    flat[hit] = case.flat_index(ids[gpu["triIndex"][hit]])
    assert np.all(flat[hit] >= 0)
    return tc.check_against_reference(ref.classify(org, dirs), flat, gpu["dist"], what) + (cnt,)


def check_case(case, ctx, accel, osc, seed=0):
    ref = tc.Reference(case)
    totals = np.zeros(3, np.int64)
    for set_name, (org, dirs) in all_rays(case, osc, seed).items():
        h, m, _ = check_rays(case, ctx, accel, osc, ref, org, dirs, f"{case.name}/{set_name}")
        totals += (h, m, len(org))
    print(f"{case.name}: {totals[0]} robust hits + {totals[1]} robust misses of {totals[2]} rays agree with float64")
    return totals


@pytest.mark.parametrize("name,final", STATES)
def test_closest_and_any_hit_on_adversarial_rays(built_lib, name, final):
    case = SCENES[name]()
    ctx = api.Context(0)
    accel = build(case, ctx, final)
    if final:
        case.set_state(True)
    osc = oracle_for(case, final)
    assert ctx.accel_stats(accel)["triRecords"] == len(case.tris64)
    totals = check_case(case, ctx, accel, osc)
    assert totals[0] > 0 and totals[1] > 0


@pytest.mark.parametrize("n", tc.SIZES)
def test_sizes_under_every_leaf_size(built_lib, n):
    """1..9 triangles (the one-node subtree up to 8), 63..65 and 4097, built with 1, 2 and 4 triangles per leaf."""
    for max_leaf in (1, 2, 4):
        case = tc.sizes_case(n, max_leaf)
        ctx = api.Context(0)
        accel = build(case, ctx)
        stats = ctx.accel_stats(accel)
        assert stats["triRecords"] == n and (stats["nodes"] == 1) == (n <= 8)
        check_case(case, ctx, accel, oracle_for(case), seed=n)
        ctx.close()


def _nest_rays():
    return util.pinhole_rays(64, 64, NEST_CAM, NEST_LOOK, fov_y_deg=0.002)


def test_deep_nest_spills_the_k_trace_stack(built_lib):
    case = tc.deep_case()
    ctx = api.Context(0)
    accel = build(case, ctx)
    depth = ctx.accel_stats(accel)["maxDepth"]
    osc = oracle_for(case)
    org, dirs = _nest_rays()
    h, m, cnt = check_rays(case, ctx, accel, osc, tc.Reference(case), org, dirs, "deep nest", counters=True)
    print(f"deep nest: maxDepth {depth}, k_trace stack spills {cnt[3]} over {cnt[2]} rays, {h} robust hits")
    assert depth >= DEEP_MIN_LEVELS, f"the nest collapsed to {depth} levels"
    assert cnt[3] > 0, "no ray of the deep nest spilled its LDS stack"
    assert h > 0


def test_animated_update_deepens_the_split_tree(built_lib):
    """Declared-animated levels lined up side by side (shallow), then moved into the nest by a transform update: the in-place
    rebuild of the animated subtree reports the new depth, k_trace spills on it, and closest / any hits equal the oracle rebuilt
    from scratch and its brute force."""
    case = tc.animated_deep_case()
    ctx = api.Context(0)
    accel = build(case, ctx)
    before = ctx.accel_stats(accel)
    for slot, xfm in case.moves.items():
        ctx.instance_set_transform(slot, xfm)
    assert ctx.accel_build(handle=accel) == accel
    after = ctx.accel_stats(accel)
    print(f"animated nest: maxDepth {before['maxDepth']} -> {after['maxDepth']}")
    assert after["maxDepth"] > before["maxDepth"] and after["maxDepth"] >= DEEP_MIN_LEVELS
    case.set_state(True)
    osc = oracle_for(case, final=True)
    org, dirs = _nest_rays()
    _, _, cnt = check_rays(case, ctx, accel, osc, tc.Reference(case), org, dirs, "deepened nest", counters=True)
    assert cnt[3] > 0
    gpu = util.gpu_trace(ctx, accel, api.TRACE_CLOSEST, org, dirs)
    util.compare_closest(gpu, util.accel_tri_ids(ctx, accel), osc.trace(0, org, dirs), osc.tri_ids(), "deepened nest vs the oracle's traversal")


def _nest_camera(width, height):
    """A GfxCamera at NEST_CAM looking at the nest's corner (orientation columns: left, up, forward), a 0.004-degree field."""
    f = np.asarray(NEST_LOOK, np.float64) - np.asarray(NEST_CAM, np.float64)
    f /= np.linalg.norm(f)
    left = np.cross((0.0, 1.0, 0.0), f)
    left /= np.linalg.norm(left)
    up = np.cross(f, left)
    cam = api.make_camera(width, height, pos=NEST_CAM, fov_y_deg=0.004)
    cam.orientation = (ctypes.c_float * 9)(*np.stack([left, up, f], axis=1).astype(np.float32).reshape(9).tolist())
    return cam


@pytest.mark.parametrize("animated", [False, True])
def test_one_kernel_path_tracer_on_the_deep_nest(built_lib, animated):
    """trace_wave_local (k_pt_fused) sizes its stack spill by the tree's depth (local_spill_depth): on the deep nest, and on the
    split tree a transform update made deep after the build, every buffer equals the oracle's."""
    case = tc.animated_deep_case() if animated else tc.deep_case()

    def build_deep(ctx, osc):
        accel = build(case, ctx, final=animated, upload=False)       # run_pt_both has uploaded the scene
        if animated:
            for slot, xfm in case.moves.items():
                osc.set_instance_transform(slot, xfm)
            osc.commit()
        assert ctx.accel_stats(accel)["maxDepth"] >= DEEP_MIN_LEVELS
        return accel

    diffs = run_pt_both(case.hs, 96, 64, frames=2, max_len=3, camera=_nest_camera(96, 64), fuse=2, build=build_deep)
    assert not diffs, "\n".join(diffs)
