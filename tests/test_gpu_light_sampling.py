"""-m gpu: the emitter distributions (gfxexp_amd/csrc/lights.hip, read back with gfx_lights_read) and the light sampler of the
passes (shading.hip.h, run by the inspection entry gfx_lights_sample) against the CPU oracle, bit for bit, on the scenes of
tests/light_scenes.py.  tests/test_light_sampling_cpu.py holds the oracle against the float64 definition, so equality here puts
the kernels under that definition too."""
import functools

import numpy as np
import pytest

from gfxexp_amd import api
from tests import light_scenes as LS, util

pytestmark = pytest.mark.gpu
F = np.float32
MODES = (api.LIGHTS_SAMPLE, api.LIGHTS_SAMPLE_SEARCH, api.LIGHTS_SAMPLE_SOLID_ANGLE)


def gpu_sample(ctx, mode, u3, shading_point=(0, 0, 0)):
    import torch
    u = np.zeros((len(u3), 4), F)
    u[:, :3] = u3
    d_u = torch.from_numpy(u).cuda()
    d_out = torch.zeros(len(u) * 16, dtype=torch.float32, device="cuda")
    ctx.lights_sample(mode, d_u.data_ptr(), len(u), d_out.data_ptr(), shading_point, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(api.LIGHT_SAMPLE_DTYPE).reshape(len(u))


def assert_equals_oracle(what, layout, got, oracle, table_used):
    ls, pd, ids = oracle
    assert np.array_equal(got["record"], layout.record_of(ids)), f"{what}: picked record differs on {np.count_nonzero(got['record'] != layout.record_of(ids))} samples"
    assert np.array_equal(got["instSlot"], ids[:, 0]), what
    util.assert_same_bits(what + " density", got["areaPDensity"], pd)
    util.assert_same_bits(what + " emittance", got["emittance"], ls[:, 0:3])
    util.assert_same_bits(what + " position", got["position"], ls[:, 3:6])
    util.assert_same_bits(what + " normal", got["normal"], ls[:, 6:9])
    assert np.array_equal(got["atInfinity"], ls[:, 9].astype(np.uint32)), what
    assert np.all(got["tableUsed"] == table_used), what
    assert np.all(got["pad"] == 0), what


class Gpu:
    def __init__(self, name):
        self.c = LS.case(name)
        self.ctx = api.Context(0)
        self.c.hs.upload(self.ctx)
        self.ctx.lights_build_static()
        self.ctx.lights_build_instances()
        self.info = self.ctx.lights_table_info()


@functools.lru_cache(maxsize=None)
def gpu(name):
    return Gpu(name)


def _same_distribution(what, got, want):
    util.assert_same_bits(what + " weights", got[0], want[0])
    util.assert_same_bits(what + " cdf", got[1], want[1])
    util.assert_same_bits(what + " integral", F(got[2]), F(want[2]))


@pytest.mark.parametrize("name", list(LS.SCENES))
def test_distributions_equal_the_oracle(built_lib, name):
    g = gpu(name)
    c, ctx = g.c, g.ctx
    _same_distribution(f"{name} level 0", ctx.lights_read(0), c.l0)           # always whole: the chunked scan
    for slot, t in c.l2.items():
        _same_distribution(f"{name} geometry {slot}", ctx.lights_read(2, slot), t)
    n = len(c.layout.insts)
    if n > 5000:
        rng = np.random.default_rng(17)
        near = [i for b in (4096, 8192) for i in range(b - 2, b + 3) if i < n]
        which = sorted(set([0, n - 1] + near + [int(i) for i in rng.choice(n, 256, replace=False)]))
    else:
        which = range(n)
    empty = (np.zeros(0, F), np.zeros(0, F), 0.0)
    for ii in which:
        _same_distribution(f"{name} instance {ii}", ctx.lights_read(1, ii), c.l1.get(ii, empty))
    # the table's state
    print(f"\n{name}: {g.info}")
    assert g.info["records"] == c.layout.num_records
    if n <= 65536:
        assert g.info["usable"] == 1 and g.info["verified"] == g.info["records"], g.info
    else:
        print(f"{name}: above the instance guide's 65536 entries the interval table reports usable = {g.info['usable']}")      # not promised either way
        # (the guide's own flag lives in a device word no entry of the C ABI reads; that it has withdrawn shows only in mode 1 still
        # equalling the oracle through the plain search, test_sampler_equals_the_oracle)


@pytest.mark.parametrize("name", list(LS.SCENES))
def test_sampler_equals_the_oracle(built_lib, name):
    g = gpu(name)
    c, ctx, lay = g.c, g.ctx, g.c.layout
    usable = g.info["usable"]
    # the stratified sweep at (u0, u1) = (1/2, 1/2)
    u = np.full((c.n, 3), 0.5, F)
    u[:, 0] = LS.sweep_ul(c.n)
    sweep = [gpu_sample(ctx, m, u) for m in MODES[:2]]
    assert_equals_oracle(f"{name} sweep, sample_light", lay, sweep[0], c.sweep, usable)
    assert_equals_oracle(f"{name} sweep, three searches", lay, sweep[1], c.sweep, 0)
    for f in api.LIGHT_SAMPLE_DTYPE.names:
        if f != "tableUsed":
            util.assert_same_bits(f"{name} mode 0 against mode 1, {f}", sweep[0][f], sweep[1][f])
    # selection numbers exactly on an entry of the instance-level CDF
    ul, _ = LS.tie_ul(c.l0)
    if len(ul):
        tie = np.full((len(ul), 3), 0.5, F)
        tie[:, 0] = ul
        on_ties = c.osc.sample_light_ids((0, 0, 0), tie)
        assert_equals_oracle(f"{name} instance boundaries, sample_light", lay, gpu_sample(ctx, MODES[0], tie), on_ties, usable)
        assert_equals_oracle(f"{name} instance boundaries, three searches", lay, gpu_sample(ctx, MODES[1], tie), on_ties, 0)
    # 8 x 8 positions on each of the chosen records
    want, ul = LS.choose_records(lay, c.rec, c.counts, seed=31, extra=(LS.MIRRORED_INSTANCE,) if name == "transforms" else ())
    grid = np.concatenate([np.repeat(ul, 64)[:, None], np.tile(LS.grid_u01(), (len(want), 1))], 1).astype(F)
    on_records = c.osc.sample_light_ids((0, 0, 0), grid)
    assert_equals_oracle(f"{name} grid, sample_light", lay, gpu_sample(ctx, MODES[0], grid), on_records, usable)
    assert_equals_oracle(f"{name} grid, three searches", lay, gpu_sample(ctx, MODES[1], grid), on_records, 0)
    # solid-angle sampling: the grids and a coarser sweep from three shading points (inside the scene, far outside, the origin --
    # in the emitters' plane y = 0 for the instance-count scenes)
    b = c.hs.bounds().astype(np.float64)
    centre, size = 0.5 * (b[:3] + b[3:]), np.linalg.norm(b[3:] - b[:3])
    coarse = np.full((1 << 14, 3), 0.25, F)
    coarse[:, 0] = LS.sweep_ul(1 << 14)
    both = np.concatenate([grid, coarse])
    for sp in (centre + 0.1 * size, centre + np.array([3.0, 20.0, -7.0]) * size, np.zeros(3)):
        sp = sp.astype(F)
        assert_equals_oracle(f"{name} solid angle from {sp}", lay, gpu_sample(ctx, MODES[2], both, sp), c.osc.sample_light_ids(sp, both, solid_angle=True), 0)


def test_record_order_matches_positions(built_lib):
    """The mapping (instance, geometry, primitive) -> record used above, checked against geometry: a sample the kernel reports on
    record r lies in the world-space triangle that the definition (tests/light_ref.py) lists at r."""
    g = gpu("transforms")
    c = g.c
    want, ul = LS.choose_records(c.layout, c.rec, c.counts, seed=2)
    grid = np.concatenate([np.repeat(ul, 64)[:, None], np.tile(LS.grid_u01(), (len(want), 1))], 1).astype(F)
    got = gpu_sample(g.ctx, api.LIGHTS_SAMPLE, grid)
    assert np.array_equal(got["record"].reshape(-1, 64), np.repeat(want[:, None], 64, 1).astype(np.uint32))
    ids, tris, _, _, _ = c.ref.records()
    tri = tris[want]
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    nrm = np.cross(e1, e2)
    d = got["position"].astype(np.float64).reshape(-1, 64, 3) - tri[:, None, 0]
    nn = np.einsum("ij,ij->i", nrm, nrm)[:, None]
    bb = np.einsum("nmj,nj->nm", np.cross(d, e2[:, None]), nrm) / nn
    cc = np.einsum("nmj,nj->nm", np.cross(e1[:, None], d), nrm) / nn
    assert np.all(bb >= -1e-4) and np.all(cc >= -1e-4) and np.all(bb + cc <= 1 + 1e-4)
    assert np.all(np.abs(np.einsum("nmj,nj->nm", d, nrm)) / np.sqrt(nn) <= 1e-4)


def test_zero_weight_emitters(built_lib):
    hs = LS.zero_weight_scene()
    osc = util.feed_oracle(hs)
    lay = LS.Layout(hs)
    ctx = api.Context(0)
    hs.upload(ctx)
    ctx.lights_build_static()
    ctx.lights_build_instances()
    assert ctx.lights_table_info()["usable"] == 0
    u = np.full((256, 3), 0.5, F)
    u[:, 0] = LS.sweep_ul(256)
    sp = np.array([0.3, 1.0, 0.3], F)
    for m in MODES:
        got = gpu_sample(ctx, m, u, sp)
        assert np.all(got["areaPDensity"] == 0) and np.all(got["record"] == LS.NONE)
        assert_equals_oracle(f"zero weight, mode {m}", lay, got, osc.sample_light_ids(sp, u, solid_angle=m == MODES[2]), 0)


def test_animated_emitter(built_lib):
    hs = LS.animated_scene()
    osc = util.feed_oracle(hs)
    lay = LS.Layout(hs)
    ctx = api.Context(0)
    hs.upload(ctx)
    ctx.instance_set_dynamic(LS.ANIMATED_INSTANCE)
    accel = ctx.accel_build()
    ctx.lights_build_static()
    ctx.lights_build_instances()
    u = np.random.default_rng(8).random((4096, 3)).astype(F)
    sp = np.array([1.0, 3.0, 1.0], F)

    def frame():
        assert ctx.lights_table_info()["usable"] == 1
        out = []
        for m in MODES:
            got = gpu_sample(ctx, m, u, sp)
            assert_equals_oracle(f"animated, mode {m}", lay, got, osc.sample_light_ids(sp, u, solid_angle=m == MODES[2]), 1 if m == MODES[0] else 0)
            out.append(got)
        return out[0], ctx.lights_read(0), ctx.lights_read(1, LS.ANIMATED_INSTANCE)

    before = frame()
    frames = [before]
    for xfm in LS.ANIMATED_MOVES:
        ctx.instance_set_transform(LS.ANIMATED_INSTANCE, xfm)
        osc.set_instance_transform(LS.ANIMATED_INSTANCE, xfm)
        assert ctx.accel_build(handle=accel) == accel
        with pytest.raises(api.GfxError, match="not built"):            # moved, distributions not rebuilt yet
            gpu_sample(ctx, api.LIGHTS_SAMPLE, u[:4])
        ctx.lights_build_instances()
        osc.commit()
        frames.append(frame())
        _same_distribution("animated level 0", frames[-1][1], osc.lights_read(0))
    moved = frames[0][0]["instSlot"] == LS.ANIMATED_INSTANCE
    assert np.any(moved)
    # a translation: the same picks at other positions, every distribution unchanged
    assert np.array_equal(frames[1][0]["record"], frames[0][0]["record"])
    assert np.all(np.any(frames[1][0]["position"][moved] != frames[0][0]["position"][moved], axis=1))
    util.assert_same_bits("positions of the others", frames[1][0]["position"][~moved], frames[0][0]["position"][~moved])
    _same_distribution("level 0 after a translation", frames[1][1], frames[0][1])
    _same_distribution("level 1 after a translation", frames[2][2], frames[0][2])
    # scale 2 -> 3: the instance's weight follows sx^2, the others keep theirs
    w0, w2 = frames[1][1][0].astype(np.float64), frames[2][1][0].astype(np.float64)
    assert abs(w2[LS.ANIMATED_INSTANCE] / w0[LS.ANIMATED_INSTANCE] - 9.0 / 4.0) <= 8 * 2.0 ** -24 * 9.0 / 4.0
    others = np.arange(len(w0)) != LS.ANIMATED_INSTANCE
    assert np.array_equal(w2[others], w0[others])
    assert np.any(frames[2][0]["position"][moved] != frames[1][0]["position"][moved])


def test_refusals(built_lib):
    import torch
    hs = LS.animated_scene()
    ctx = api.Context(0)
    hs.upload(ctx)
    d_u = torch.zeros(64 * 4 + 4, dtype=torch.float32, device="cuda")
    d_out = torch.zeros(64 * 16 + 4, dtype=torch.float32, device="cuda")
    with pytest.raises(api.GfxError, match="not built"):
        ctx.lights_sample(api.LIGHTS_SAMPLE, d_u.data_ptr(), 64, d_out.data_ptr())
    ctx.lights_build_static()
    ctx.lights_build_instances()
    with pytest.raises(api.GfxError, match="unknown mode"):
        ctx.lights_sample(3, d_u.data_ptr(), 64, d_out.data_ptr())
    with pytest.raises(api.GfxError, match="16-byte aligned"):
        ctx.lights_sample(api.LIGHTS_SAMPLE, d_u.data_ptr() + 4, 64, d_out.data_ptr())
    with pytest.raises(api.GfxError, match="16-byte aligned"):
        ctx.lights_sample(api.LIGHTS_SAMPLE, d_u.data_ptr(), 64, d_out.data_ptr() + 8)
    ctx.lights_sample(api.LIGHTS_SAMPLE, 0, 0, 0)                        # n == 0: nothing to do, nothing touched
    ctx.lights_sample(api.LIGHTS_SAMPLE, d_u.data_ptr(), 64, d_out.data_ptr())
    torch.cuda.synchronize()
    assert torch.all(d_out[64 * 16:] == 0)
