"""CPU: displaced instances of a scene on the host -- the host compilation of csrc/tfdm/tfdm_instance.hip.h
(tests/scene_trace_host.cpp) around the host core (tests/tfdm_host.cpp).

  * make_instance: the inverse, the refusals, the world box;
  * the world-box cull changes nothing: a host scene trace (the CPU oracle's BVH8 trace, then the host core per instance) with the
    cull is bit-equal to the same trace without it;
  * geometry, independent of the core: one displaced quad under transforms whose linear part is exact in float (a signed axis
    permutation times power-of-two scales), against the float64 brute force over the WORLD-space micro-mesh.

The distance tolerance is the one of tests/test_tfdm_cpu.py, worked out for this scene: E_mesh is measured in the same run, per
transform, as the largest |t - t64| / max(1, t64) of the oracle's BVH8 trace of the world-space tessellation against the float64
brute force, over the rays the edge rule keeps (at most 2 % are left out); the scene query is allowed 8 x E_mesh.  Measured
(printed by the test, recorded in DESIGN.md section 15): E_mesh = 3.154e-06 / 7.801e-06 / 3.771e-06 for the uniform / non-uniform /
mirrored transform, worst error of the scene query 1.20 x / 0.47 x / 1.00 x E_mesh."""
import copy

import numpy as np
import pytest

from gfxexp_amd import api
from tests import scene_trace_host as S
from tests import tfdm_host as T
from tests import util

EDGE_CAP = 0.02
INVALID = api.GFX_INVALID_SLOT


@pytest.fixture(scope="module")
def host(built_lib, tmp_path_factory):
    return T.Host(tmp_path_factory.mktemp("tfdm_host"))


@pytest.fixture(scope="module")
def shost(built_lib, tmp_path_factory):
    return S.SceneHost(tmp_path_factory.mktemp("scene_host"))


def _root(lo, hi):
    r = np.zeros(1, api.TFDM_NODE_DTYPE)
    r["lo"], r["hi"], r["count"] = lo, hi, 1
    return r


# ---------------------------------------------------------------- make_instance
def test_inverse_and_world_box(shost):
    rng = np.random.default_rng(11)
    p = T.CoreParams()
    worst = 0.0
    for i in range(200):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        m = S.affine(q @ np.diag(rng.uniform(0.5, 2.0, 3)), rng.uniform(-1, 1, 3))
        lo = rng.uniform(-5, 5, 3)
        hi = lo + rng.uniform(0.01, 8, 3)
        root = _root(lo, hi)
        rec = shost.make_instance(m, root, (1, 2, 3, 4), p, user_id=i)[0]
        assert np.array_equal(rec["objToWorld"], m.reshape(12)) and rec["userId"] == i
        a = np.vstack([rec["objToWorld"].astype(np.float64).reshape(3, 4), [0, 0, 0, 1]])
        b = np.vstack([rec["worldToObj"].astype(np.float64).reshape(3, 4), [0, 0, 0, 1]])
        worst = max(worst, np.abs(b @ a - np.eye(4)).max())
        assert np.abs(b @ a - np.eye(4)).max() <= 1e-6, "inverse x matrix is off the identity by %.3e" % np.abs(b @ a - np.eye(4)).max()
        wlo, whi = S.image_of_box(m, root["lo"][0], root["hi"][0])
        assert np.all(rec["boxLo"].astype(np.float64) < wlo) and np.all(rec["boxHi"].astype(np.float64) > whi)
        # the pad is the one the header states, not a loose box: 2^-16 x (max |coordinate| + max extent), plus the two outward
        # roundings to float (each at most one step, 2^-23 of the coordinate's power of two)
        big = np.abs(np.concatenate([wlo, whi])).max()
        pad = (big + (whi - wlo).max()) * 2.0 ** -16
        steps = 4 * 2.0 ** -23 * big
        assert np.all(wlo - rec["boxLo"] <= pad * 1.001 + steps) and np.all(rec["boxHi"] - whi <= pad * 1.001 + steps)
        assert np.all(wlo - rec["boxLo"] >= pad * 0.999) and np.all(rec["boxHi"] - whi >= pad * 0.999)
    print("worst |W M - I| over 200 rotations with per-axis scales in [0.5, 2]: %.3e" % worst)


def test_singular_and_non_finite_transforms_are_refused(shost):
    p = T.CoreParams()
    root = _root((0, 0, 0), (1, 1, 1))
    good = S.affine(np.eye(3), (1, 2, 3))
    shost.make_instance(good, root, (0, 0, 0, 0), p)
    bad = []
    for v in (np.nan, np.inf, -np.inf):
        for at in (0, 5, 11):
            m = good.copy().reshape(12)
            m[at] = v
            bad.append(("non-finite", m, "not finite"))
    bad.append(("zero", S.affine(np.zeros((3, 3)), (0, 0, 0)), "singular"))
    bad.append(("a zero scale", S.affine(np.diag([1.0, 0.0, 2.0]), (0, 0, 0)), "singular"))
    rank2 = np.array([[1.0, 2.0, 3.0], [0.5, -1.0, 0.25], [1.5, 1.0, 3.25]])        # row 2 = row 0 + row 1, exact in float
    bad.append(("rank 2", S.affine(rank2, (1, 1, 1)), "singular"))
    q = S.rotation((1, 2, 3), 40.0)
    bad.append(("rank 2 after rounding", S.affine(q @ np.diag([1.0, 1.0, 0.0]) @ q.T, (0, 0, 0)), "singular"))
    for name, m, text in bad:
        with pytest.raises(ValueError, match=text):
            shost.make_instance(m, root, (0, 0, 0, 0), p)


def test_a_root_box_that_is_not_finite_gives_the_whole_space(shost):
    rec = shost.make_instance(S.affine(np.eye(3), (0, 0, 0)), _root((-np.inf, 0, 0), (1, 1, np.inf)), (0, 0, 0, 0), T.CoreParams())[0]
    assert np.all(rec["boxLo"] == -np.inf) and np.all(rec["boxHi"] == np.inf)


# ---------------------------------------------------------------- cull == no cull
@pytest.fixture(scope="module")
def chain_scene(host, shost):
    states = [host.state(v, t, h, gp) for v, t, h, gp in S.chain_objects()]
    table = np.concatenate([shost.instance_of_state(states[o], m, user_id=100 + k) for k, (o, m) in enumerate(S.chain_instances())])
    unpadded = [S.image_of_box(m, states[o]["nodes"][0]["lo"], states[o]["nodes"][0]["hi"]) for o, m in S.chain_instances()]
    return states, table, unpadded


def test_world_box_cull_changes_nothing(shost, chain_scene):
    states, table, unpadded = chain_scene
    org, dirs = S.chain_rays(unpadded)
    extra = [S.box_rays(lo, hi, 500, seed=50 + k) for k, (lo, hi) in enumerate(unpadded)]
    org = np.concatenate([org] + [e[0] for e in extra])
    dirs = np.concatenate([dirs] + [e[1] for e in extra])
    osc = util.feed_oracle(S.plain_bunny_scene())
    for mode in (api.TRACE_CLOSEST, api.TRACE_ANY):
        plain = osc.trace(mode, org, dirs)
        culled, c1 = shost.trace(table, plain, mode, org, dirs, cull=True, counters=True)
        full, c0 = shost.trace(table, plain, mode, org, dirs, cull=False, counters=True)
        if mode == api.TRACE_CLOSEST:
            for f in api.SCENE_HIT_DTYPE.names:
                util.assert_same_bits("closest, field %s, with and without the world-box cull" % f, culled[f], full[f])
            where = culled["where"]
            shares = [np.mean(where == api.SCENE_PLAIN)] + [np.mean((where >> 1 == k) & (where < api.SCENE_PLAIN)) for k in range(len(table))]
            print("closest hits: plain %.1f %%, instances %s %%, miss %.1f %%" % (100 * shares[0], ["%.1f" % (100 * s) for s in shares[1:]], 100 * np.mean(where == INVALID)))
            assert all(s > 0.02 for s in shares), "every part of the scene is hit by some rays: %s" % shares
            miss = where == INVALID
            assert np.all(culled["dist"][miss] == dirs[miss, 3]) and np.all(culled["index"][miss] == INVALID)
            assert np.all(culled["normal"][miss | (where == api.SCENE_PLAIN)] == 0)
        else:
            assert np.array_equal(culled, full)
        print("mode %d: %d world-box tests, %d traversals with the cull, %d without" % (mode, c1[4], c1[5], c0[5]))
        assert c1[4] == c0[4] and c1[5] < c0[5] and c0[5] == c0[4]
        assert c1[2] == len(org)


def test_merge_rule_on_equal_distance(host, shost):
    """A plain hit at exactly the displaced distance stays; the same object twice under one transform reports the lower index."""
    v, t, h, gp = S.chain_objects()[0]
    st = host.state(v, t, h, gp)
    m = S.affine(S.rotation((0, 0, 1), 20.0), (0.5, 0, 0))
    table = np.concatenate([shost.instance_of_state(st, m), shost.instance_of_state(st, m)])
    org, dirs = T.cap_rays(3000)
    org[:, :3] = org[:, :3] @ m[:, :3].T.astype(np.float32) + m[:, 3]
    dirs[:, :3] = dirs[:, :3] @ m[:, :3].T.astype(np.float32)
    two = shost.trace(table, None, api.TRACE_CLOSEST, org, dirs)
    hit = two["where"] != INVALID
    assert hit.mean() > 0.3 and np.all(two["where"][hit] >> 1 == 0)
    one = shost.trace(table[:1], None, api.TRACE_CLOSEST, org, dirs)
    for f in api.SCENE_HIT_DTYPE.names:
        util.assert_same_bits("twice the same instance, field %s" % f, two[f], one[f])
    plain = np.zeros(len(org), api.HIT_DTYPE)
    plain["dist"], plain["bcB"], plain["bcC"], plain["triIndex"] = one["dist"], 0.25, 0.5, np.where(hit, 7, INVALID)
    tied = shost.trace(table, plain, api.TRACE_CLOSEST, org, dirs)
    assert np.all(tied["where"][hit] == api.SCENE_PLAIN) and np.all(tied["index"][hit] == 7) and np.all(tied["dist"] == one["dist"])
    assert np.all(tied["where"][~hit] == INVALID)


# ---------------------------------------------------------------- geometry, independent of the core
def _flag_and_cap(edge, near, what):
    flagged = edge | near
    share = flagged.mean()
    print("%s: edge rays %.2f %% + near-miss rays %.2f %% of %d" % (what, 100 * edge.mean(), 100 * (near & ~edge).mean(), len(edge)))
    assert share <= EDGE_CAP, "%s: %.2f %% of the rays are edge rays, the cap is 2 %%" % (what, 100 * share)
    return ~flagged


# linear part = signed axis permutation x power-of-two scales (exact in float), dyadic translation
EXACT = {
    "rotated_uniform": (np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]]) * 2.0, (3.25, -1.5, 0.75)),
    "non_uniform": (np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]]) @ np.diag([0.5, 2.0, 4.0]), (-2.0, 0.625, 1.25)),
    "mirrored": (np.array([[-1, 0, 0], [0, 0, 1], [0, 1, 0]]) @ np.diag([2.0, 0.25, -1.0]), (0.5, 4.0, -3.0)),
}


@pytest.fixture(scope="module")
def quad_micro_mesh(built_lib):
    v, t = T.quad_mesh()
    heights = T.two_sine_map(64)
    gp = api.tfdm_params(h_scale=0.1)
    return v, t, heights, gp, T.MicroMesh(v, t, T.mips32(heights), gp)


@pytest.mark.parametrize("name", sorted(EXACT))
def test_displaced_quad_under_exact_transforms(host, shost, quad_micro_mesh, name):
    v, t, heights, gp, mm = quad_micro_mesh
    L, tr = EXACT[name]
    L = np.asarray(L, np.float64)
    m = S.affine(L, tr)
    assert np.array_equal(m.astype(np.float64)[:, :3], L) and abs(np.linalg.det(L)) > 0
    if name == "mirrored":
        assert np.linalg.det(L) < 0
    # the world-space micro-mesh in float64, the world rays as the images of the cap rays
    world = copy.copy(mm)
    world.A, world.B, world.C = (x @ L.T + np.asarray(tr) for x in (mm.A, mm.B, mm.C))
    o, d = T.cap_rays(20000)
    org, dirs = T.pack_rays(o[:, :3].astype(np.float64) @ L.T + np.asarray(tr), d[:, :3].astype(np.float64) @ L.T)
    t64, k64, edge, near = T.brute64(world.A, world.B, world.C, org[:, :3], dirs[:, :3], org[:, 3].astype(np.float64), dirs[:, 3].astype(np.float64),
                                     clip=(mm.tA, mm.tB, mm.tC, mm.baseTc, mm.prim))
    keep = _flag_and_cap(edge, near, name)
    want_hit = np.isfinite(t64)
    # E_mesh of this transform: the oracle's BVH8 trace of the world-space tessellation against the same float64 distances
    mv, mt = world.float32_mesh()
    assert len(mt) == 2 * 64 * 64
    s = api.HostScene()
    g = s.add_geom(mv, mt, s.add_material_traditional((0.5, 0.5, 0.5), (0, 0, 0), 0.3))
    s.add_instance(s.add_group([g]), api.make_transform())
    mesh_hits = util.feed_oracle(s).trace(0, org, dirs)
    mesh_hit = mesh_hits["triIndex"] != INVALID
    assert np.array_equal(mesh_hit[keep], want_hit[keep])
    both = keep & mesh_hit
    e_mesh = float((np.abs(mesh_hits["dist"][both].astype(np.float64) - t64[both]) / np.maximum(1.0, t64[both])).max())
    print("%s: E_mesh = %.3e (BVH8 trace of the world-space tessellation against float64)" % (name, e_mesh))
    assert 0 < e_mesh < 1e-4
    # the scene query on the host: no plain geometry, one instance
    st = host.state(v, t, heights, gp)
    hits = shost.trace(shost.instance_of_state(st, m), None, api.TRACE_CLOSEST, org, dirs)
    got_hit = hits["where"] != INVALID
    assert want_hit[keep].mean() > 0.3
    bad = keep & (got_hit != want_hit)
    assert not bad.any(), "%s: hit / miss differs on %d rays, first %d" % (name, bad.sum(), np.nonzero(bad)[0][0])
    both = keep & want_hit
    bad = both & (hits["index"] != np.where(k64 >= 0, mm.prim[np.maximum(k64, 0)], -1))
    assert not bad.any(), "%s: the primitive differs on %d rays, first %d" % (name, bad.sum(), np.nonzero(bad)[0][0])
    err = np.abs(hits["dist"][both].astype(np.float64) - t64[both]) / np.maximum(1.0, t64[both])
    print("%s: worst |t - t64| / max(1, t64) = %.3e = %.2f x E_mesh over %d rays" % (name, err.max(), err.max() / e_mesh, both.sum()))
    assert err.max() <= 8 * e_mesh, "%s: ray %d is off by %.3e, 8 x E_mesh = %.3e" % (name, np.nonzero(both)[0][err.argmax()], err.max(), 8 * e_mesh)
    assert np.all(hits["where"][got_hit] >> 1 == 0) and np.all(hits["dist"][~got_hit] == dirs[~got_hit, 3])
    # world normals are unit, and frontFace is the side of the WORLD normal the ray comes from (the mirrored instance too)
    n = hits["normal"][got_hit].astype(np.float64)
    assert np.all(np.abs(np.linalg.norm(n, axis=1) - 1) < 1e-5)
    side = (dirs[got_hit, :3].astype(np.float64) * n).sum(1) / np.linalg.norm(dirs[got_hit, :3].astype(np.float64), axis=1)
    sure = np.abs(side) > 1e-4
    assert sure.mean() > 0.99 and np.array_equal((hits["where"][got_hit][sure] & 1) == 1, side[sure] < 0)
    # ... and it points away from the base plane's image on the side the height field rises to: the image of +z, up to the mirror
    up = np.linalg.inv(L).T @ np.array([0.0, 0.0, 1.0])
    above = got_hit & np.all((o[:, :2] > 0) & (o[:, :2] < 1), 1)
    assert above.sum() > 4000 and np.all((hits["where"][above] & 1) == 1) and np.all(hits["normal"][above].astype(np.float64) @ up > 0)
    # any-hit: 1 exactly where the closest-hit query finds something
    occ = shost.trace(shost.instance_of_state(st, m), None, api.TRACE_ANY, org, dirs)
    assert np.array_equal(occ == 1, got_hit)
