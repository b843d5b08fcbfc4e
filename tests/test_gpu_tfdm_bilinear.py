"""-m gpu: the Bilinear (Newton) local intersection, GFX_TFDM_BILINEAR, through the C ABI.

What the device computes is held bit for bit, in every field, against the host compilation of the same core (tests/tfdm_host.cpp,
tests/scene_trace_host.cpp, tests/displaced_host.cpp); what the core computes is held against float64 on the host side
(tests/test_tfdm_bilinear_cpu.py, whose cases and ray sets these tests reuse).  So the figures of that file -- E_mesh, the worst
|t - t64| |cos| -- are the device's too."""
import numpy as np
import pytest

from gfxexp_amd import api
from tests import displaced_host as D
from tests import scene_trace_host as S
from tests import test_gpu_displaced_render as DR
from tests import test_gpu_displaced_restir as RS
from tests import test_tfdm_bilinear_cpu as B
from tests import tfdm_host as T
from tests import util
from tests.test_gpu_scene_trace import gpu_scene_trace
from tests.test_gpu_tfdm import gpu_tfdm_trace

pytestmark = pytest.mark.gpu
INVALID = api.GFX_INVALID_SLOT


@pytest.fixture(scope="module")
def host(built_lib, tmp_path_factory):
    return T.Host(tmp_path_factory.mktemp("tfdm_host"))


@pytest.fixture(scope="module")
def shost(built_lib, tmp_path_factory):
    return S.SceneHost(tmp_path_factory.mktemp("scene_host"))


@pytest.fixture(scope="module")
def dhost(built_lib, tmp_path_factory):
    return D.DisplacedHost(tmp_path_factory.mktemp("displaced_host"))


def _leaning(mirror):
    v, t = B.leaning_quad(mirror)
    return v, t, T.two_sine_map(16), B.bilinear_params(h_scale=0.1)


CASES = {
    "flat_two_sine_16": lambda: B._flat("two_sine_16"),
    "flat_random_16": lambda: B._flat("random_16"),
    "flat_wrapped_rotated": lambda: B._flat("wrapped_rotated"),
    "flat_two_sine_32_level2": lambda: B._flat("two_sine_32_level2"),
    "leaning_plain_uv": lambda: _leaning(False),
    "leaning_mirrored_uv": lambda: _leaning(True),
}


def _rays():
    """3990 rays (not a multiple of 64): the cap rays; origins inside the layer; tmax around and tmin beyond the surface; far origins;
    rays in the base plane and along texel edges."""
    rng = np.random.default_rng(31)
    o, d = T.cap_rays(B.N_RAYS)
    n = 600
    oi, di = T.pack_rays(np.stack([rng.uniform(0.05, 0.95, n), rng.uniform(0.05, 0.95, n), rng.uniform(0.002, 0.098, n)], 1),
                         np.stack([rng.uniform(-0.7, 0.7, n), rng.uniform(-0.7, 0.7, n), rng.choice([-1.0, 1.0], n)], 1))
    ow, dw = T.cap_rays(n, seed=8)
    dw[:, 3] = rng.uniform(0.6, 1.1, n)                                  # ends somewhere around the surface
    ow[: n // 2, 3] = rng.uniform(0.7, 1.0, n // 2)                      # ... and half of them start there
    of, df = T.cap_rays(n, seed=9)
    dd = df[:, :3].astype(np.float64)
    of[:, :3] = (of[:, :3].astype(np.float64) - (64.0 / np.linalg.norm(dd, axis=1))[:, None] * dd).astype(np.float32)
    m = 690
    a = rng.uniform(0, 2 * np.pi, m)
    og, dg = T.pack_rays(np.stack([rng.uniform(-0.5, 1.5, m), np.round(rng.uniform(0, 16, m)) / 16.0, rng.choice([0.0, 0.05], m)], 1),
                         np.stack([np.cos(a), np.where(np.arange(m) % 2 == 0, 0.0, np.sin(a)), np.zeros(m)], 1))
    org, dirs = np.concatenate([o, oi, ow, of, og]), np.concatenate([d, di, dw, df, dg])
    assert len(org) == 3990 and len(org) % 64 != 0
    return np.ascontiguousarray(org, np.float32), np.ascontiguousarray(dirs, np.float32)


def _same_hits(what, got, want, names=api.TFDM_HIT_DTYPE.names):
    for f in names:
        util.assert_same_bits("%s: field %s" % (what, f), got[f], want[f])


# ---------------------------------------------------------------- 8. device against host core
@pytest.mark.parametrize("name", sorted(CASES))
def test_gfx_tfdm_trace_equals_the_host_core_bit_for_bit(built_lib, host, name):
    v, t, heights, gp = CASES[name]()
    ctx = api.Context(0)
    tf = api.Tfdm(ctx, v, t, heights, gp)
    st = host.state(v, t, heights, gp)
    assert st["params"].local == api.TFDM_BILINEAR
    util.assert_same_bits(name + ": records", tf.read_records(), st["records"])
    util.assert_same_bits(name + ": tree", tf.read_nodes(), st["nodes"])
    org, dirs = _rays()
    got, cnt = gpu_tfdm_trace(tf, api.TRACE_CLOSEST, org, dirs, counters=True)
    want, wcnt = host.trace_state(st, api.TRACE_CLOSEST, org, dirs, counters=True)
    hit = want["primIndex"] != INVALID
    assert 0.2 < hit.mean() < 0.98, "%s: %.1f %% of the rays hit" % (name, 100 * hit.mean())
    _same_hits(name + ": closest hit", got, want)
    assert np.array_equal(cnt, wcnt), "%s: counters %s on the device, %s on the host" % (name, cnt, wcnt)
    occ = gpu_tfdm_trace(tf, api.TRACE_ANY, org, dirs)
    util.assert_same_bits(name + ": any hit", occ, host.trace_state(st, api.TRACE_ANY, org, dirs))
    assert np.array_equal(occ == 1, hit) and np.all(occ <= 1)
    assert np.all(np.isfinite(got["dist"])) and np.all(np.isfinite(got["normal"])) and np.all(got["dist"][~hit] == dirs[~hit, 3])
    print("%s: %.1f %% hit; per ray %.1f texel box tests, %.2f leaf tests" % (name, 100 * hit.mean(), cnt[0] / cnt[2], cnt[1] / cnt[2]))
    tf.close()


def test_set_params_switches_between_the_three_modes(built_lib, host):
    v, t, heights, _ = CASES["leaning_plain_uv"]()
    modes = {m: api.tfdm_params(h_scale=0.1, local_intersection=m) for m in (api.TFDM_BOX, api.TFDM_TWO_TRIANGLE, api.TFDM_BILINEAR)}
    ctx = api.Context(0)
    fresh = {m: api.Tfdm(ctx, v, t, heights, gp) for m, gp in modes.items()}
    org, dirs = _rays()
    want = {m: gpu_tfdm_trace(tf, api.TRACE_CLOSEST, org, dirs) for m, tf in fresh.items()}
    assert not np.array_equal(want[api.TFDM_BILINEAR]["normal"], want[api.TFDM_TWO_TRIANGLE]["normal"])
    changed = api.Tfdm(ctx, v, t, heights, modes[api.TFDM_TWO_TRIANGLE])
    for m in (api.TFDM_BILINEAR, api.TFDM_BOX, api.TFDM_BILINEAR, api.TFDM_TWO_TRIANGLE):
        changed.set_params(modes[m])
        # records, boxes and the tree do not depend on the mode
        util.assert_same_bits("records", changed.read_records(), fresh[m].read_records())
        util.assert_same_bits("boxes", changed.read_aabbs(), fresh[m].read_aabbs())
        util.assert_same_bits("tree", changed.read_nodes(), fresh[api.TFDM_TWO_TRIANGLE].read_nodes())
        _same_hits("switched to mode %d" % m, gpu_tfdm_trace(changed, api.TRACE_CLOSEST, org, dirs), want[m])
        util.assert_same_bits("switched to mode %d, any hit" % m, gpu_tfdm_trace(changed, api.TRACE_ANY, org, dirs), gpu_tfdm_trace(fresh[m], api.TRACE_ANY, org, dirs))
    st = host.state(v, t, heights, modes[api.TFDM_BILINEAR])
    _same_hits("created as Bilinear", want[api.TFDM_BILINEAR], host.trace_state(st, api.TRACE_CLOSEST, org, dirs))


# ---------------------------------------------------------------- 9. a mixed set
GENERAL = S.affine(S.rotation((0.3, 1.0, 0.2), 35.0) @ np.diag([2.0, 1.0, 0.5]), (0.2, 0.3, 0.5))     # non-uniform scale 2 x 1 x 0.5, rotated
TILTED = S.affine(S.rotation((1.0, 0.2, 0.0), -25.0) @ np.diag([1.2, 1.2, 1.2]), (-0.3, 0.4, 0.9))


def _scene_rays(table, n=3000):
    """Rays from a shell around the instances' world boxes toward points inside them; a third with a tmin / tmax window; not a
    multiple of 64."""
    rng = np.random.default_rng(17)
    lo, hi = table["boxLo"].min(0).astype(np.float64), table["boxHi"].max(0).astype(np.float64)
    c, r = 0.5 * (lo + hi), 0.5 * np.linalg.norm(hi - lo)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = c + 1.5 * r * d
    org, dirs = T.pack_rays(o, (lo + rng.uniform(0, 1, (n, 3)) * (hi - lo)) - o)      # unnormalised: the target lies at parameter 1
    org[::3, 3] = rng.uniform(0.0, 0.9, len(org[::3]))
    dirs[::3, 3] = org[::3, 3] + rng.uniform(0.0, 0.6, len(org[::3])).astype(np.float32)
    return org[:-7].copy(), dirs[:-7].copy()


def _host_table(host, shost, v, t, heights, members):
    """members: [(gp, objToWorld, userId)]; the records carry the pointers of host states, which the second result keeps alive."""
    states = [host.state(v, t, heights, gp) for gp, _, _ in members]
    return np.concatenate([shost.instance_of_state(st, m, uid) for st, (_, m, uid) in zip(states, members)]), states


@pytest.mark.parametrize("with_bilinear", [True, False], ids=["box_two_triangle_bilinear", "box_two_triangle"])
def test_gfx_trace_scene_over_a_mixed_set(built_lib, host, shost, with_bilinear):
    """One object's mesh and map under the three modes, each under its own transform, in one set.  Without the Bilinear member the
    set runs the instantiation it ran before the mode existed: the same bits as the host core all the same."""
    v, t = B.leaning_quad(False)
    heights = T.two_sine_map(16)
    gp = {m: api.tfdm_params(h_scale=0.1, local_intersection=m) for m in (api.TFDM_BOX, api.TFDM_TWO_TRIANGLE, api.TFDM_BILINEAR)}
    members = [(gp[api.TFDM_BOX], S.affine(np.eye(3), (0, 0, 0)), 7), (gp[api.TFDM_TWO_TRIANGLE], TILTED, 8)]
    if with_bilinear:
        members.insert(1, (gp[api.TFDM_BILINEAR], GENERAL, 9))
    ctx = api.Context(0)
    objs = [api.Tfdm(ctx, v, t, heights, g) for g, _, _ in members]
    tset = api.TfdmSet(ctx)
    for k, (tf, (_, m, uid)) in enumerate(zip(objs, members)):
        assert tset.add(tf, m, uid) == k
    tset.commit()
    table, states = _host_table(host, shost, v, t, heights, members)
    dev = tset.read()
    for f in ("objToWorld", "worldToObj", "boxLo", "boxHi", "userId", "params"):
        util.assert_same_bits("InstanceRecord." + f, dev[f], table[f])
    org, dirs = _scene_rays(dev)
    got, cnt = gpu_scene_trace(ctx, 0, tset, api.TRACE_CLOSEST, org, dirs, counters=True)
    want, wcnt = shost.trace(table, None, api.TRACE_CLOSEST, org, dirs, counters=True)
    _same_hits("mixed set", got, want, api.SCENE_HIT_DTYPE.names)
    assert np.array_equal(cnt, wcnt), "counters %s on the device, %s on the host" % (cnt, wcnt)
    where = got["where"]
    hit = where != INVALID
    shares = [np.mean(hit & (where >> 1 == k)) for k in range(len(members))]
    print("closest hits per instance %s %%, miss %.1f %%" % (["%.1f" % (100 * s) for s in shares], 100 * np.mean(~hit)))
    assert all(s > 0.03 for s in shares), shares
    assert np.all(np.abs(np.linalg.norm(got["normal"][hit].astype(np.float64), axis=1) - 1) < 1e-5)
    occ = gpu_scene_trace(ctx, 0, tset, api.TRACE_ANY, org, dirs)
    util.assert_same_bits("mixed set, any hit", occ, shost.trace(table, None, api.TRACE_ANY, org, dirs))
    assert np.array_equal(occ == 1, hit)
    if with_bilinear:
        # distances are the world ray's parameter: the object-space ray (direction not renormalised, 0.5 to 2 long here) traced
        # alone finds the same parameter, and org + dist dir lies on the instance's surface box in world space
        k = 1
        mine = hit & (where >> 1 == k)
        oo, od = shost.to_object_rays(table[k:k + 1], org, dirs)
        ln = np.linalg.norm(od[mine, :3], axis=1)
        assert ln.min() < 0.8 and ln.max() > 1.25
        alone = host.trace_state(states[k], api.TRACE_CLOSEST, oo[mine], od[mine])
        util.assert_same_bits("the parameter of the object-space ray", alone["dist"], got["dist"][mine])
        p = org[mine, :3].astype(np.float64) + got["dist"][mine, None].astype(np.float64) * dirs[mine, :3].astype(np.float64)
        assert np.all(p >= dev["boxLo"][k] - 1e-6) and np.all(p <= dev["boxHi"][k] + 1e-6)
    tset.close()


# ---------------------------------------------------------------- 10. a bound set with a Bilinear member
def test_a_bound_set_with_bilinear_members_in_the_gbuffer_pass_and_restir(built_lib, host, shost, dhost):
    """The 96 x 64 scene of tests/test_gpu_displaced_render.py with its quad object switched to GFX_TFDM_BILINEAR (two of the three
    instances; the bunny stays in Box mode).  The primary hits equal the host's instance arithmetic after gfx_trace; the G-buffer of a
    displaced pixel equals the host composition fed that hit; under GFX_DISPLACED_RESTIR one ReSTIR DI frame runs, and the occlusion
    words of its shadow-ray passes equal gfx_trace_scene and the host's any-hit answer over the queue's own rays."""
    import torch
    sc = DR.Scene()
    ctx = sc.ctx
    gp = B.bilinear_params(h_scale=0.1)
    sc.tfdm[0].set_params(gp)
    sc.set.commit()
    W, H, n = DR.W, DR.H, DR.W * DR.H
    qv, qt = T.quad_mesh()
    bv, bt = T.obj_mesh("stanford_bunny_309_faces.obj")
    ext = float((bv["position"].max(0) - bv["position"].min(0)).max())
    states = {0: host.state(qv, qt, sc.heights, gp),
              1: host.state(bv, bt, sc.heights, api.tfdm_params(h_scale=0.02 * ext, local_intersection=api.TFDM_BOX, target_mip_level=1))}
    table_host = np.concatenate([shost.instance_of_state(states[o], m, 50 + k) for k, (o, m, _) in enumerate(sc.members)])
    table = sc.set.read()
    assert list(table["params"][:, 4]) == [api.TFDM_BILINEAR, api.TFDM_BILINEAR, api.TFDM_BOX]
    # the G-buffer pass
    fr = DR.Frames(sc)
    sc.bind()
    f = fr.set_params(0, DR.camera(0), None, jitter=1)
    d_org, d_dir = torch.zeros(n * 4, dtype=torch.float32, device="cuda"), torch.zeros(n * 4, dtype=torch.float32, device="cuda")
    d_hit = torch.zeros(n * 8, dtype=torch.int32, device="cuda")
    ctx.restir_primary_rays(W, H, d_org.data_ptr(), d_dir.data_ptr(), DR._stream())
    api.trace_scene(ctx, sc.accel, sc.set, api.TRACE_CLOSEST, d_org.data_ptr(), d_dir.data_ptr(), n, d_hit.data_ptr(), stream=DR._stream())
    torch.cuda.synchronize()
    org, dirs = d_org.cpu().numpy().reshape(n, 4), d_dir.cpu().numpy().reshape(n, 4)
    hits = d_hit.cpu().numpy().view(api.SCENE_HIT_DTYPE).reshape(n)
    plain = util.gpu_trace(ctx, sc.accel, api.TRACE_CLOSEST, org, dirs)
    _same_hits("primary hits", hits, shost.trace(table_host, plain, api.TRACE_CLOSEST, org, dirs), api.SCENE_HIT_DTYPE.names)
    fr.gbuffer()
    got = fr.dev.download()
    where = hits["where"]
    disp = (where != INVALID) & (where != api.SCENE_PLAIN)
    idx = np.nonzero(disp)[0]
    inst = where[idx] >> 1
    shares = [np.mean(disp & (where >> 1 == k)) for k in range(3)]
    assert all(s >= 0.02 for s in shares), shares
    base = np.zeros((len(idx), 15), np.float32)
    for k in range(3):
        base[inst == k] = D.base_verts_of(sc.meshes[k][0], sc.meshes[k][1], hits["index"][idx][inst == k])
    xy = np.stack([np.arange(n) % W, np.arange(n) // W], 1)
    ref = dhost.resolve(table, hits[idx], org[idx], dirs[idx], base, np.array(sc.slots, np.uint32)[inst], np.array([m for _, _, m in sc.members], np.uint32)[inst],
                        xy[idx], f.prevCamera, W, H, reset_flow=True)
    for k in ("g0", "g1", "g2", "g3"):
        util.assert_same_bits("gbuffer%s of displaced pixels" % k[1], DR._words(got["gb%s_0" % k[1]])[idx], DR._words(ref[k]))
    assert np.all(DR._words(got["gb0_0"])[idx, 0] == (api.GBUFFER_DISPLACED | inst))
    # one ReSTIR DI frame under GFX_DISPLACED_RESTIR
    ctx.bind_displaced(sc.set, sc.slots, restir=True)
    rs = RS.Restir(sc)
    rs.params(0, DR.camera(0))
    rs.launch(api.PASS_SETUP_GBUFFERS, 0, 0)
    occluded_by_displaced = 0
    for what, pass_id, cur, base_index in (("initial RIS", api.PASS_INITIAL_RIS, 0, 0), ("spatial", api.PASS_SPATIAL_BIASED, 0, 0),
                                           ("shading", api.PASS_SHADING, 1, RS.NB)):
        rs.launch(pass_id, cur, base_index)
        q = RS.Queue(ctx, RS.CAP)
        assert q.n > 0
        util.assert_same_bits(what + ": occlusion words against gfx_trace_scene", q.occ, RS.any_hit(ctx, sc.accel, sc.set, q))
        plain_any = RS.any_hit(ctx, sc.accel, None, q, scene=False)
        util.assert_same_bits(what + ": occlusion words against the host", q.occ, shost.trace(table_host, plain_any, api.TRACE_ANY, q.org, q.dir))
        occluded_by_displaced += int((q.occ != plain_any).sum())
    out = rs.dev.download()
    sc.unbind()
    assert occluded_by_displaced > 0, "the displaced instances occlude some shadow ray the BVH8 lets through"
    rgb = out["beauty"][:, :3]
    lit = (out["gb0_0"]["instSlot"] != INVALID) & (out["gb0_0"]["instSlot"] >= api.GBUFFER_DISPLACED)
    assert lit.mean() > 0.05 and np.isfinite(rgb).all() and rgb[lit].mean() > 1e-3, "displaced pixels receive light"


# ---------------------------------------------------------------- 11. refusals
def test_only_the_three_modes_are_accepted(built_lib):
    ctx = api.Context(0)
    v, t = T.quad_mesh()
    heights = T.two_sine_map(16)
    for bad in (2, 3, 5):
        with pytest.raises(api.GfxError, match="localIntersection"):
            api.Tfdm(ctx, v, t, heights, api.tfdm_params(h_scale=0.1, local_intersection=bad))
    assert api.TFDM_BILINEAR == 4
    tf = api.Tfdm(ctx, v, t, heights, api.tfdm_params(h_scale=0.1, local_intersection=4))
    for bad in (2, 3, 5):
        with pytest.raises(api.GfxError, match="localIntersection"):
            tf.set_params(api.tfdm_params(h_scale=0.1, local_intersection=bad))
    org, dirs = T.cap_rays(1000)
    assert (gpu_tfdm_trace(tf, api.TRACE_CLOSEST, org, dirs)["primIndex"] != INVALID).mean() > 0.5      # and the refused changes left it as it was
    tf.close()
