"""CPU: the host compilation of csrc/tfdm/tfdm_core.hip.h (tests/tfdm_host.cpp) against float64 numpy code that shares no line with it
(tests/tfdm_host.py): the min-max pyramid, the stackless texel walk, containment of the displaced surface in every box the query
tests, and hits against the explicit micro-triangle mesh traced by brute force.

The distance tolerance is not a chosen number.  E_mesh is measured in the same run: the largest |t - t64| / max(1, t64) of the
existing BVH8 trace (the CPU oracle's, which the GPU's gfx_trace equals bit for bit: tests/test_gpu_trace.py) on the tessellated
quad against the float64 brute force, over the rays the edge rule keeps.  The TFDM query is allowed 8 x E_mesh: its tangent-space
route adds an fp32 4 x 4 transform of origin and direction, a normalised interpolated normal and the corner products, a handful
of roundings of the same relative size; a wrong corner sample or level would be off by hScale / 255 and more.

Edge rule (a condition on the rays, asserted before anything is compared): rays whose float64 closest hit has a barycentric
coordinate below 1e-3 -- of the micro-triangle, or of the base triangle the hit is clipped to -- or that pass within 1e-3 outside
a nearer micro-triangle are left out; they may be at most 2 % of the rays."""
import numpy as np
import pytest

from gfxexp_amd import api
from tests import tfdm_host as T
from tests import util

EDGE_CAP = 0.02


@pytest.fixture(scope="module")
def host(built_lib, tmp_path_factory):
    return T.Host(tmp_path_factory.mktemp("tfdm_host"))


def _corner_samples32(level):
    """The tex2DLod contract at every corner of the texel grid, float32, in the contract's order: [n + 1, n + 1]."""
    h = np.ascontiguousarray(level, np.float32)
    n = h.shape[0]
    i = np.arange(n + 1)
    a, b = (i - 1) % n, i % n
    q = np.float32(0.25)
    return ((q * h[np.ix_(a, a)] + q * h[np.ix_(a, b)]) + q * h[np.ix_(b, a)]) + q * h[np.ix_(b, b)]


@pytest.mark.parametrize("name", ["two_sine_64", "random_32", "random_32_own_mips"])
def test_pyramid(host, name):
    rng = np.random.default_rng(3)
    if name == "two_sine_64":
        heights = T.two_sine_map(64)
    else:
        heights = (rng.integers(0, 256, (32, 32)).astype(np.float32) / np.float32(255)).astype(np.float32)
    size = heights.shape[0]
    mips = T.mips32(heights)
    if name == "random_32_own_mips":      # supplied levels that are NOT the mean: a coarse level may stick out of its children's range
        mips = [mips[0]] + [np.clip(m + rng.uniform(-0.2, 0.2, m.shape), 0, 1).astype(np.float32) for m in mips[1:]]
        levels = host.levels(mips)
    else:
        levels = host.levels(heights)
    for l, m in enumerate(mips):
        util.assert_same_bits("height level %d" % l, host.level(levels, size, l), m)
    pyr = host.pyramid(levels, size)
    every_sample = []
    for l, m in enumerate(mips):
        c = _corner_samples32(m)
        every_sample.append(c)
        four = np.stack([c[:-1, :-1], c[:-1, 1:], c[1:, :-1], c[1:, 1:]])
        lo, hi = four.min(0), four.max(0)
        got = host.level(pyr, size, l, per=2)
        if l == 0:
            util.assert_same_bits("level 0 min", got[..., 0], lo)
            util.assert_same_bits("level 0 max", got[..., 1], hi)
            continue
        child = host.level(pyr, size, l - 1, per=2)
        for dy in (0, 1):
            for dx in (0, 1):
                assert np.all(got[..., 0] <= child[dy::2, dx::2, 0]) and np.all(got[..., 1] >= child[dy::2, dx::2, 1]), l
        assert np.all(got[..., 0] <= lo) and np.all(got[..., 1] >= hi), l          # the "own level" term
        # ... and nothing looser than that: the entry IS the extreme of its children and its own samples
        cl = np.minimum(np.minimum(child[0::2, 0::2, 0], child[0::2, 1::2, 0]), np.minimum(child[1::2, 0::2, 0], child[1::2, 1::2, 0]))
        ch = np.maximum(np.maximum(child[0::2, 0::2, 1], child[0::2, 1::2, 1]), np.maximum(child[1::2, 0::2, 1], child[1::2, 1::2, 1]))
        util.assert_same_bits("level %d min" % l, got[..., 0], np.minimum(cl, lo))
        util.assert_same_bits("level %d max" % l, got[..., 1], np.maximum(ch, hi))
    top = host.level(pyr, size, len(mips) - 1, per=2)[0, 0]
    assert top[0] <= min(c.min() for c in every_sample) and top[1] >= max(c.max() for c in every_sample)


def _walk_triangles(rng):
    """Triangles in texture space on the 1 / 128 grid (every float32 operation of the classification is then exact, so the float64
    yardstick decides the same ties): small ones, ones across several wraps, flipped ones, ones larger than the map."""
    out = []
    while len(out) < 40:
        kind = len(out) % 4
        span = (24, 200, 700, 1500)[kind]
        c = rng.integers(-600, 600, 2)
        t = (c + rng.integers(-span, span + 1, (3, 2))).astype(np.float64) / 128.0
        area = (t[1, 0] - t[0, 0]) * (t[2, 1] - t[0, 1]) - (t[1, 1] - t[0, 1]) * (t[2, 0] - t[0, 0])
        if abs(area) < 1e-3:
            continue
        if (len(out) // 4) % 2 == (0 if area > 0 else 1):      # alternate the orientation
            t = t[[0, 2, 1]]
        out.append(t)
    return out


@pytest.mark.parametrize("target", [0, 2])
def test_walk_visits_exactly_the_overlapping_texels(host, target):
    rng = np.random.default_rng(11)
    size = 16
    heights = (rng.integers(0, 256, (size, size)).astype(np.float32) / np.float32(255)).astype(np.float32)
    levels = host.levels(heights)
    pyr = host.pyramid(levels, size)
    gp = api.tfdm_params(target_mip_level=target)
    p = host.params(gp, size)
    res = size >> target
    flipped = spans = larger = 0
    for tc in _walk_triangles(rng):
        v = np.zeros(3, api.VERTEX_DTYPE)
        v["position"] = [(0, 0, 0), (1, 0, 0), (0, 1, 0.25)]
        v["normal"] = (0, 0, 1)
        v["texCoord"] = tc
        rec = host.records(v, [[0, 1, 2]], gp, size)
        assert rec["numRoots"][0] >= 1
        util.assert_same_bits("stored texture coordinates", rec["tc"][0], tc.astype(np.float32).ravel())
        flipped += int(rec["flipped"][0])
        ext = tc.max(0) - tc.min(0)
        spans += int(np.any(np.floor(tc.max(0)) - np.floor(tc.min(0)) >= 2))
        larger += int(np.any(ext > 1))
        x0, y0, x1, y1 = T.texel_range(tc, res)
        xs, ys = np.meshgrid(np.arange(x0 - 1, x1 + 2), np.arange(y0 - 1, y1 + 2))
        hit = T.overlap_sat(tc, (xs + 0.5) / res, (ys + 0.5) / res, 0.5 / res)
        want = set(zip(xs[hit].tolist(), ys[hit].tolist()))
        assert want
        for sx in (0, 1):
            for sy in (0, 1):
                tex, _ = host.walk(rec[0], pyr, p, sx, sy, boxes=False)
                leaf = tex[tex[:, 2] == target]
                assert np.all(tex[:, 2] >= target)
                got = list(zip(leaf[:, 0].tolist(), leaf[:, 1].tolist()))
                assert len(got) == len(set(got)), "a texel was visited twice (signs %d %d)" % (sx, sy)
                assert set(got) == want, "signs %d %d: %d missed, %d extra" % (sx, sy, len(want - set(got)), len(set(got) - want))
    assert flipped >= 10 and spans >= 10 and larger >= 10      # the input set holds what it claims to hold


def _tc_samples(rect_lo, rect_hi, k=8):
    """k x k sample positions over rectangles [m, 2] x [m, 2], borders included: [m, k * k, 2] and the local coordinates."""
    g = np.linspace(0.0, 1.0, k)
    a, b = np.meshgrid(g, g)
    ab = np.stack([a.ravel(), b.ravel()], 1)
    return rect_lo[:, None, :] + ab[None] * (rect_hi - rect_lo)[:, None, :]


def _heights_at(corner, res, x, y, tc):
    """Bilinear height of the corner samples of texel (x, y) [m] of a grid with `res` texels per unit at positions tc [m, s, 2]."""
    n = corner.shape[0] - 1
    a = np.clip(tc[..., 0] * res - x[:, None], 0, 1)
    b = np.clip(tc[..., 1] * res - y[:, None], 0, 1)
    xm, ym = x % n, y % n
    tl, tr, bl, br = corner[ym, xm], corner[ym, xm + 1], corner[ym + 1, xm], corner[ym + 1, xm + 1]
    return (1 - a) * (1 - b) * tl[:, None] + a * (1 - b) * tr[:, None] + (1 - a) * b * bl[:, None] + a * b * br[:, None]


def _containment(host, vertices, triangles, heights, gp, tri_subset=None, unbounded_cap=0.0):
    """Samples of the surface inside every per-triangle box and every texel box of the descent; returns the smallest margin seen,
    relative to the box size (a negative margin is a sample outside).

    A texel box with an infinite bound is correct but worthless, so their share is capped.  The affine form gives up only where the
    interval of the interpolated normal's squared length reaches zero.  With one normal for the whole triangle it never does: the
    cap is 0.  With smooth normals it does where the vertex normals of a triangle are far enough apart that their extrapolation
    over the footprint's bounds can vanish, which takes about a right angle between them: the creases of a mesh, a few triangles in
    a hundred on the teapot (rim, lid, spout and handle joints).  The cap there is 5 %; a core that gave up as a rule would be near
    100 %."""
    st = host.state(vertices, triangles, heights, gp)
    size, target = st["size"], int(gp.targetMipLevel)
    mips = T.mips32(heights) if isinstance(heights, np.ndarray) else heights
    corner = T.corner_heights64(mips[target])
    res = size >> target
    X = T.transform64(gp)
    base, scale = T.height_terms64(gp)
    worst = np.inf
    tested = unbounded = 0
    todo = range(len(triangles)) if tri_subset is None else tri_subset
    for pi in todo:
        rec = st["records"][pi]
        if rec["numRoots"] == 0:
            continue
        bt = T.Base64(vertices, triangles[pi], X)
        tex, boxes = host.walk(rec, st["pyramid"], st["params"], 0, 0)
        leaf = tex[:, 2] == target
        lx, ly = tex[leaf, 0].astype(np.int64), tex[leaf, 1].astype(np.int64)
        lo = np.maximum(np.stack([lx, ly], 1) / res, bt.tc.min(0))
        hi = np.minimum(np.stack([lx + 1, ly + 1], 1) / res, bt.tc.max(0))
        tc = _tc_samples(lo, hi)                                           # [m, 64, 2]: 64 per target texel, over the clipped texel
        h = base + scale * _heights_at(corner, res, lx, ly, tc)
        S = bt.surface(tc, h)                                              # object space
        St = bt.to_tangent(S)                                              # tangent space
        # every texel box of the descent: the samples of the target texels underneath it
        for (x, y, lod), box in zip(tex, boxes.astype(np.float64)):
            under = ((lx >> (lod - target)) == x) & ((ly >> (lod - target)) == y)
            assert under.any()
            pts = St[under].reshape(-1, 3)
            if not np.all(np.isfinite(box)):                              # a bound the affine form gave up on: everything is inside
                assert np.all(box[:3][~np.isfinite(box[:3])] == -np.inf) and np.all(box[3:][~np.isfinite(box[3:])] == np.inf)
                unbounded += 1
                continue
            tested += 1
            ext = np.maximum(box[3:] - box[:3], 1e-30)
            worst = min(worst, ((pts - box[:3]) / ext).min(), ((box[3:] - pts) / ext).min())
        # the per-triangle box: the samples that lie on the base triangle, and a barycentric grid that reaches its edges and corners
        inside = np.all(bt.bary(tc) >= 0, -1)
        pts = [S[inside]]
        area_texels = abs(T._cross2(bt.tc[1] - bt.tc[0], bt.tc[2] - bt.tc[0])) * 0.5 * res * res
        k = int(np.ceil(np.sqrt(128 * max(area_texels, 1.0)))) + 1           # k (k + 1) / 2 >= 64 per texel of footprint
        i, j = np.meshgrid(np.arange(k + 1), np.arange(k + 1))
        keep = i + j <= k
        bc = np.stack([(k - i - j)[keep], i[keep], j[keep]], 1) / k
        gtc = bc @ bt.tc
        gx, gy = np.floor(gtc[:, 0] * res).astype(np.int64), np.floor(gtc[:, 1] * res).astype(np.int64)
        gh = base + scale * _heights_at(corner, res, gx, gy, gtc[:, None, :])[:, 0]
        pts.append(bt.surface(gtc, gh))
        pts = np.concatenate(pts)
        box = st["aabbs"][pi].astype(np.float64)
        assert np.all(np.isfinite(box)), "the box of triangle %d is not finite" % pi
        ext = np.maximum(box[3:] - box[:3], 1e-30)
        worst = min(worst, ((pts - box[:3]) / ext).min(), ((box[3:] - pts) / ext).min())
    print("%d texel boxes tested, %d more unbounded (conservative: such a texel is always entered)" % (tested, unbounded))
    assert tested > 0
    assert unbounded <= unbounded_cap * (tested + unbounded), "%d of %d texel boxes are unbounded, the cap is %g" % (unbounded, tested + unbounded, unbounded_cap)
    return worst


@pytest.mark.parametrize("case", ["quad_flat", "quad_rotated_scaled_level2", "teapot_smooth"])
def test_surface_lies_inside_every_box(host, case):
    heights = T.two_sine_map(64)
    if case == "quad_flat":
        v, t = T.quad_mesh()
        worst = _containment(host, v, t, heights, api.tfdm_params(h_scale=0.1))
    elif case == "quad_rotated_scaled_level2":
        v, t = T.quad_mesh()
        gp = api.tfdm_params(h_scale=0.1, h_offset=0.02, h_bias=0.5, tex_scale=(2.5, 1.5), tex_rotation=30.0, tex_offset=(0.3, -0.2), target_mip_level=2)
        worst = _containment(host, v, t, heights, gp)
    else:
        v, t = T.obj_mesh("teapot.obj")
        ext = float((v["position"].max(0) - v["position"].min(0)).max())
        worst = _containment(host, v, t, heights, api.tfdm_params(h_scale=0.01 * ext), unbounded_cap=0.05)
    print("smallest margin of a surface sample to a box face, relative to the box: %.3e" % worst)
    assert worst >= 0.0


# ---------------------------------------------------------------- hits
def _flag_and_cap(edge, near, what):
    flagged = edge | near
    share = flagged.mean()
    print("%s: edge rays %.2f %% + near-miss rays %.2f %% of %d" % (what, 100 * edge.mean(), 100 * (near & ~edge).mean(), len(edge)))
    assert share <= EDGE_CAP, "%s: %.2f %% of the rays are edge rays, the cap is 2 %%" % (what, 100 * share)
    return ~flagged


@pytest.fixture(scope="module")
def e_mesh(built_lib):
    """E_mesh of the module docstring, with the BVH8 trace of the CPU oracle on the tessellated quad."""
    heights = T.two_sine_map(64)
    v, t = T.quad_mesh()
    mm = T.MicroMesh(v, t, T.mips32(heights), api.tfdm_params(h_scale=0.1))
    mv, mt = mm.float32_mesh()
    assert len(mt) == 2 * 64 * 64
    s = api.HostScene()
    g = s.add_geom(mv, mt, s.add_material_traditional((0.5, 0.5, 0.5), (0, 0, 0), 0.3))
    s.add_instance(s.add_group([g]), api.make_transform())
    osc = util.feed_oracle(s)
    org, dirs = T.cap_rays(20000)
    hits = osc.trace(0, org, dirs)
    t64, _, edge, near = T.brute64(mm.A, mm.B, mm.C, org[:, :3], dirs[:, :3], org[:, 3].astype(np.float64), dirs[:, 3].astype(np.float64),
                                   clip=(mm.tA, mm.tB, mm.tC, mm.baseTc, mm.prim))
    keep = _flag_and_cap(edge, near, "tessellated quad")
    got_hit = hits["triIndex"] != api.GFX_INVALID_SLOT
    assert np.array_equal(got_hit[keep], np.isfinite(t64)[keep])
    both = keep & got_hit
    e = float((np.abs(hits["dist"][both].astype(np.float64) - t64[both]) / np.maximum(1.0, t64[both])).max())
    print("E_mesh = %.3e (BVH8 trace of the tessellated quad against float64)" % e)
    assert 0 < e < 1e-4
    return e


def _compare_two_triangle(host, e_mesh, v, t, heights, gp, org, dirs, what):
    mips = T.mips32(heights)
    mm = T.MicroMesh(v, t, mips, gp, level=int(gp.targetMipLevel))
    t64, k64, edge, near = T.brute64(mm.A, mm.B, mm.C, org[:, :3], dirs[:, :3], org[:, 3].astype(np.float64), dirs[:, 3].astype(np.float64),
                                     clip=(mm.tA, mm.tB, mm.tC, mm.baseTc, mm.prim))
    keep = _flag_and_cap(edge, near, what)
    st = host.state(v, t, heights, gp)
    hits = host.trace_state(st, api.TRACE_CLOSEST, org, dirs)
    got_hit = hits["primIndex"] != api.GFX_INVALID_SLOT
    want_hit = np.isfinite(t64)
    assert want_hit[keep].mean() > 0.3, "%s: the ray set barely hits the surface" % what
    bad = keep & (got_hit != want_hit)
    assert not bad.any(), "%s: hit / miss differs on %d rays, first %d" % (what, bad.sum(), np.nonzero(bad)[0][0])
    both = keep & want_hit
    bad = both & (hits["primIndex"] != np.where(k64 >= 0, mm.prim[np.maximum(k64, 0)], -1))
    assert not bad.any(), "%s: primIndex differs on %d rays, first %d" % (what, bad.sum(), np.nonzero(bad)[0][0])
    err = np.abs(hits["dist"][both].astype(np.float64) - t64[both]) / np.maximum(1.0, t64[both])
    print("%s: worst |t - t64| / max(1, t64) = %.3e = %.2f x E_mesh over %d rays" % (what, err.max(), err.max() / e_mesh, both.sum()))
    assert err.max() <= 8 * e_mesh, "%s: ray %d is off by %.3e, 8 x E_mesh = %.3e" % (what, np.nonzero(both)[0][err.argmax()], err.max(), 8 * e_mesh)
    # misses report tmax, the normal is a unit vector on the side the flag says
    assert np.all(hits["dist"][~got_hit] == dirs[~got_hit, 3])
    n = hits["normal"][got_hit].astype(np.float64)
    assert np.all(np.abs(np.linalg.norm(n, axis=1) - 1) < 1e-5)
    # any-hit: 1 exactly where the closest-hit query finds something
    occ = host.trace_state(st, api.TRACE_ANY, org, dirs)
    assert np.array_equal(occ == 1, got_hit)
    return hits, t64


def test_hits_quad_against_the_micro_mesh(host, e_mesh):
    v, t = T.quad_mesh()
    org, dirs = T.cap_rays(20000)
    hits, _ = _compare_two_triangle(host, e_mesh, v, t, T.two_sine_map(64), api.tfdm_params(h_scale=0.1), org, dirs, "quad, 20 000 rays")
    got = hits["primIndex"] != api.GFX_INVALID_SLOT
    # the flag is the side of the object-space normal the ray comes from
    side = (dirs[got, :3].astype(np.float64) * hits["normal"][got].astype(np.float64)).sum(1)
    sure = np.abs(side) > 1e-4
    assert np.array_equal(hits["frontFace"][got][sure] == 1, side[sure] < 0)
    # a ray that starts above the quad sees the top of the height field (one from beside it may enter under a crest at the open rim)
    above = got & np.all((org[:, :2] > 0) & (org[:, :2] < 1), 1)
    assert above.sum() > 4000 and np.all(hits["frontFace"][above] == 1) and np.all(hits["normal"][above][:, 2] > 0)


def test_hits_wrapped_and_rotated_transform(host, e_mesh):
    v, t = T.quad_mesh()
    gp = api.tfdm_params(h_scale=0.1, h_offset=0.01, h_bias=0.25, tex_scale=(2.5, 1.5), tex_rotation=30.0, tex_offset=(0.3, -0.2))
    org, dirs = T.cap_rays(4000)
    _compare_two_triangle(host, e_mesh, v, t, T.two_sine_map(64), gp, org, dirs, "quad, wrapped and rotated transform")


def test_hits_bunny_base_mesh(host, e_mesh):
    v, t = T.obj_mesh("stanford_bunny_309_faces.obj")
    ext = float((v["position"].max(0) - v["position"].min(0)).max())
    org, dirs = T.mesh_rays(v, 4000, 5)
    _compare_two_triangle(host, e_mesh, v, t, T.two_sine_map(64), api.tfdm_params(h_scale=0.02 * ext), org, dirs, "bunny")


def test_hits_box_mode_against_float64_boxes(host, e_mesh):
    """Box mode: the surface is the set of the target-level texel boxes.  The boxes are the core's (their containment is the test
    above); the ray transform, the slab test and the choice of the closest are float64 here.  Edge rule for boxes: the slab interval
    of the hit box, or of a nearer box the ray just misses, is shorter than 1e-3.  A texel that two base triangles share has the
    same box under both, give or take a rounding of their records: where the two distances agree within the tolerance the surface
    hit is the same one and either index is right."""
    v, t = T.quad_mesh()
    gp = api.tfdm_params(h_scale=0.1, local_intersection=api.TFDM_BOX)
    heights = T.two_sine_map(64)
    st = host.state(v, t, heights, gp)
    org, dirs = T.cap_rays(4000)
    X = T.transform64(gp)
    tmin, tmax = org[:, 3].astype(np.float64), dirs[:, 3].astype(np.float64)
    per_prim = []
    for pi in range(len(t)):
        bt = T.Base64(v, t[pi], X)
        tex, boxes = host.walk(st["records"][pi], st["pyramid"], st["params"], 0, 0)
        boxes = boxes[tex[:, 2] == 0].astype(np.float64)
        o = bt.to_tangent(org[:, :3].astype(np.float64))
        d = dirs[:, :3].astype(np.float64) @ bt.toTang[:3, :3].T
        per_prim.append(T.box_brute64(boxes, o, d, tmin, tmax))
    best = np.stack([tt.min(1) for tt, _, _ in per_prim], 1)                  # [R, prims]
    t64 = best.min(1)
    k64 = best.argmin(1)
    eps = 1e-3 / 64                                                           # 1e-3 of a texel, as a length along the ray
    edge, near = np.zeros(len(org), bool), np.zeros(len(org), bool)
    r = np.arange(len(org))
    for tt, margin, entry in per_prim:
        k = tt.argmin(1)
        edge |= np.isfinite(tt[r, k]) & (tt[r, k] <= t64) & (margin[r, k] < eps)
        with np.errstate(invalid="ignore"):
            near |= ((margin < 0) & (margin > -eps) & (entry < t64[:, None])).any(1)
    keep = _flag_and_cap(edge, near, "box mode")
    hits = host.trace_state(st, api.TRACE_CLOSEST, org, dirs)
    got_hit = hits["primIndex"] != api.GFX_INVALID_SLOT
    assert np.array_equal(got_hit[keep], np.isfinite(t64)[keep])
    both = keep & got_hit
    err = np.abs(hits["dist"][both].astype(np.float64) - t64[both]) / np.maximum(1.0, t64[both])
    print("box mode: worst error %.3e = %.2f x E_mesh over %d rays" % (err.max(), err.max() / e_mesh, both.sum()))
    assert err.max() <= 8 * e_mesh
    tol = 8 * e_mesh * np.maximum(1.0, t64)
    with np.errstate(invalid="ignore"):
        other = np.abs(best[:, 0] - best[:, 1]) <= tol
    assert np.all((hits["primIndex"][both] == k64[both]) | other[both])
    assert np.array_equal(host.trace_state(st, api.TRACE_ANY, org, dirs) == 1, got_hit)


def test_tmax_and_rays_from_inside(host):
    """tmax short of the surface is a miss that reports tmax; a ray that starts between the base plane and the surface leaves through
    the surface's back."""
    v, t = T.quad_mesh()
    heights = np.full((16, 16), 0.5, np.float32)
    st = host.state(v, t, heights, api.tfdm_params(h_scale=0.2))          # a flat sheet at z = 0.1
    org = np.array([[0.3, 0.4, 1.0], [0.3, 0.4, 1.0], [0.3, 0.4, 0.05], [0.3, 0.4, 0.05]], np.float64)
    d = np.array([[0, 0, -1], [0, 0, -1], [0, 0, 1], [0, 0, -1]], np.float64)
    o, dd = T.pack_rays(org, d)
    dd[1, 3] = 0.85
    hits = host.trace_state(st, api.TRACE_CLOSEST, o, dd)
    assert abs(hits["dist"][0] - 0.9) < 1e-6 and hits["frontFace"][0] == 1 and hits["normal"][0][2] > 0.999
    assert hits["primIndex"][1] == api.GFX_INVALID_SLOT and hits["dist"][1] == np.float32(0.85)
    assert abs(hits["dist"][2] - 0.05) < 1e-6 and hits["frontFace"][2] == 0
    assert hits["primIndex"][3] == api.GFX_INVALID_SLOT
