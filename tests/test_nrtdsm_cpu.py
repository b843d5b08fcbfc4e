"""CPU: the host compilation of csrc/nrtdsm/nrtdsm_core.hip.h (tests/nrtdsm_host.cpp) against the float64 model of the surface
(tests/nrtdsm_ref.py), which shares no line with it and models the surface, not the algorithm.

Cases: a 64 x 64 two-sine map on the quad (plain, and under a wrapped and rotated texture transform), on a curved patch (an 8 x 8-quad
spherical cap with shared radial normals, plus one base triangle with mirrored texture coordinates), on the 309-face bunny and on
the teapot.  Rays: the sets of tests/test_gpu_tfdm.py (20 000 plus the special rays) and six rays that are NaN, infinite or of zero
direction.

Edge rule (a condition on the rays under the model alone, asserted before anything is compared): a ray whose float64 closest hit has
a barycentric coordinate below 1e-3 -- of its micro-triangle (half texel) or of its base triangle -- or that passes within 1e-3
outside a nearer micro-triangle is left out of the closest / hit-or-miss comparison; at most EDGE_CAP of the rays.  One more kind of
ray falls under the rule, and under the same cap: a ray that crosses one of the model's flat facets while Newton's iteration finds no
root on any half texel near it.  It grazes a patch's bulge; the model has no hit to compare there.  "Hits lie on the surface" needs
no such rule and holds for every hit.  The teapot is compared on rays of its own (teapot_model_rays): under the common set it
exceeds the cap.

Distance tolerance, not a chosen number:  8 * E_mesh * max(1, t) + 2 * 1e-5 * s / |cos theta|.  E_mesh is measured in this run exactly
as tests/test_tfdm_cpu.py measures it (the existing BVH8 trace on the tessellated quad against float64).  The second term is the
solver's stopping width in the map value h (1e-5, kSolverEps) carried to a distance: a step of 1e-5 in h moves the surface by
s * 1e-5 * |N| along N (s = hScale / sqrt(texScale.x texScale.y), |N| <= 1 for unit vertex normals), which a ray meeting the surface
under the angle theta to its normal sees as s * 1e-5 / |cos theta|; twice, for the two ends of the stopping interval.

Normal: the model's normal on kept rays within the angle the distance tolerance implies: a hit displaced by `tol` lies on a patch whose
normal turns by less than one radian across a texel of object size w, so the normal is off by at most tol / w, plus 1e-5 rad for
the float32 evaluation of a cross product of two differences.

Measured (this file, on the host core): see DESIGN.md section 20."""
import numpy as np
import pytest

from gfxexp_amd import api
from tests import nrtdsm_host as NH
from tests import nrtdsm_ref as NR
from tests import tfdm_host as T
from tests import util
from tests.test_gpu_tfdm import _special_rays
from tests.test_tfdm_cpu import e_mesh      # noqa: F401 -- the fixture, measured exactly as there

EDGE_CAP = 0.02
N_RAYS = 20000

CASES = {
    "quad": dict(mesh="quad", gp=dict(h_scale=0.1)),
    "quad_wrapped_rotated": dict(mesh="quad", gp=dict(h_scale=0.1, h_offset=0.01, h_bias=0.25, tex_scale=(2.5, 1.5), tex_rotation=30.0, tex_offset=(0.3, -0.2))),
    "cap": dict(mesh="cap", gp=dict(h_scale=0.05)),
    "bunny": dict(mesh="stanford_bunny_309_faces.obj", gp=dict(h_scale=0.02), relative=True),
    "teapot": dict(mesh="teapot.obj", gp=dict(h_scale=0.01), relative=True),
}


def case_inputs(name):
    """(vertices, triangles, heights, params, rays): shared with tests/test_gpu_nrtdsm.py."""
    c = CASES[name]
    v, t = T.quad_mesh() if c["mesh"] == "quad" else NH.cap_mesh() if c["mesh"] == "cap" else T.obj_mesh(c["mesh"])
    gpk = dict(c["gp"])
    if c.get("relative"):
        gpk["h_scale"] *= float((v["position"].max(0) - v["position"].min(0)).max())
    rng = np.random.default_rng(23)
    o, d = T.cap_rays(N_RAYS) if c["mesh"] == "quad" else T.mesh_rays(v, N_RAYS, 5)
    so, sd = _special_rays(v, rng)
    bo, bd = T.pack_rays(np.full((6, 3), 0.5), np.tile([0.1, 0.2, -1.0], (6, 1)))
    bo[0, 0], bo[1, 1], bd[2, 2], bd[3, 0], bd[4, :3], bo[5, 3] = np.nan, np.inf, np.nan, -np.inf, 0.0, np.nan
    return v, t, T.two_sine_map(64), api.tfdm_params(**gpk), (np.concatenate([o, so, bo]), np.concatenate([d, sd, bd]))


N_BAD = 6
MODEL_CASES = sorted(CASES)
# The model finds its candidates on flat facets (k x k per half texel) on these; test_doubling_k... shows k = 1 enough.  On the teapot
# it does not use facets at all (below), so there is no k to double.
FACET_CASES = ["bunny", "cap", "quad", "quad_wrapped_rotated"]
N_TEAPOT_MODEL_RAYS = 1500


def teapot_model_rays(S, n=N_TEAPOT_MODEL_RAYS, seed=41, cone_deg=20.0):
    """The teapot's rays for the comparison with the model.  Its 15 704 base triangles cover about one texel each and are displaced by
    half their own size: under the rays of tests/test_gpu_tfdm.py 4 to 6 % are edge rays, above EDGE_CAP, so the case gets rays of its
    own, as the rule says: through points of the model's surface (base triangles drawn by area, uniform barycentrics), directions within
    `cone_deg` of the model's normal there, origins a quarter of the mesh's extent away.  Fewer of them, because here the model solves
    every half texel near a ray directly (Surface.trace(exact=True)): a flat facet can hide a nearer, strongly curved patch."""
    rng = np.random.default_rng(seed)
    area = np.linalg.norm(np.cross(S.p[:, 1] - S.p[:, 0], S.p[:, 2] - S.p[:, 0]), axis=1)
    prim = rng.choice(len(area), n, p=area / area.sum())
    r1, r2 = np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 1, n)
    a, b = r1 * (1 - r2), r1 * r2
    X, nm = S.point(prim, a, b), S.normal(prim, a, b)
    ang, phi = np.arccos(rng.uniform(np.cos(np.radians(cone_deg)), 1.0, n)), rng.uniform(0, 2 * np.pi, n)
    t1 = unit(np.cross(nm, np.where(np.abs(nm[:, :1]) < 0.9, [[1.0, 0, 0]], [[0, 1.0, 0]])))
    t2 = np.cross(nm, t1)
    d = -(np.cos(ang)[:, None] * nm + np.sin(ang)[:, None] * (np.cos(phi)[:, None] * t1 + np.sin(phi)[:, None] * t2))
    return T.pack_rays(X - 0.25 * S.extent * d, d * (0.5 * S.extent))


@pytest.fixture(scope="module")
def host(built_lib, tmp_path_factory):
    return NH.Host(tmp_path_factory.mktemp("nrtdsm_host"))


_SOLVED = {}


def solved(host, name, model=False):
    """Everything a case's tests share, computed once: the host core's answers and, with `model`, the model's closest hits (k = 1)."""
    if name not in _SOLVED:
        v, t, heights, gp, (org, dirs) = case_inputs(name)
        st = host.state(v, t, heights, gp)
        hits, cnt, it = host.trace(st, api.TRACE_CLOSEST, org, dirs, counters=True, iterations=True)
        S = NR.Surface(v, t, T.mips32(heights)[0], gp)
        _SOLVED[name] = dict(v=v, t=t, heights=heights, gp=gp, org=org, dirs=dirs, st=st, hits=hits, cnt=cnt, it=it, S=S)
    c = _SOLVED[name]
    if model and "m" not in c:
        # mo, md, mhits: the rays the model is compared on and the host core's answers to them
        if name == "teapot":
            c["mo"], c["md"] = teapot_model_rays(c["S"])
            c["mhits"] = host.trace(c["st"], api.TRACE_CLOSEST, c["mo"], c["md"])
        else:
            c["mo"], c["md"], c["mhits"] = c["org"], c["dirs"], c["hits"]
        c["m"] = c["S"].trace(c["mo"][:, :3], c["md"][:, :3], c["mo"][:, 3], c["md"][:, 3], k=1, exact=name == "teapot")
    return c


def kept(m, what):
    share = m["flagged"].mean()
    print("%s: edge rays %.2f %% of %d" % (what, 100 * share, len(m["flagged"])))
    assert share <= EDGE_CAP, "%s: %.2f %% of the rays are edge rays, the cap is 2 %%" % (what, 100 * share)
    return ~m["flagged"]


def tolerance(c, e_mesh, t, cos, dlen):
    """In units of the ray's parameter t (as E_mesh is); `dlen` = |d| carries the second term, an object-space distance, there."""
    s = c["S"].scale
    return 8 * e_mesh * np.maximum(1.0, t) + 2 * 1e-5 * abs(s) / (np.maximum(np.abs(cos), 1e-12) * dlen)


def unit(d):
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


@pytest.mark.parametrize("name", FACET_CASES)
def test_doubling_k_does_not_change_the_models_hits(host, name):
    """The set of hits of ALL the test rays: hit or miss, base triangle, distance."""
    c = solved(host, name, model=True)
    m2 = c["S"].trace(c["org"][:, :3], c["dirs"][:, :3], c["org"][:, 3], c["dirs"][:, 3], k=2, flags=False)
    h1, h2 = np.isfinite(c["m"]["t"]), np.isfinite(m2["t"])
    with np.errstate(invalid="ignore"):
        differ = (h1 != h2) | (h1 & h2 & ((c["m"]["prim"] != m2["prim"]) | (np.abs(c["m"]["t"] - m2["t"]) > 1e-9 * np.maximum(1, np.abs(m2["t"])))))
    print("%s: k = 1 -> 2 changes %d of %d rays" % (name, differ.sum(), len(differ)))
    assert not differ.any(), "rays %s" % np.nonzero(differ)[0][:10]


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_hit_lies_on_the_surface(host, e_mesh, name):
    """|o + t d - S_prim(bcB, bcC)| in float64 within the distance tolerance, for every hit of every ray: no edge rule."""
    c = solved(host, name)
    S, hits, org, dirs = c["S"], c["hits"], c["org"], c["dirs"]
    o64, d64 = org[:, :3].astype(np.float64), dirs[:, :3].astype(np.float64)
    got = hits["primIndex"] != api.GFX_INVALID_SLOT
    assert 0.2 < got[:N_RAYS].mean() < 0.98, "%s: %.1f %% of the rays hit" % (name, 100 * got.mean())
    g = np.nonzero(got)[0]
    prim, a, b, t = hits["primIndex"][g].astype(np.int64), hits["bcB"][g].astype(np.float64), hits["bcC"][g].astype(np.float64), hits["dist"][g].astype(np.float64)
    off = np.linalg.norm(o64[g] + t[:, None] * d64[g] - S.point(prim, a, b), axis=1)
    # theta: between the ray and the model's normal at the reported point
    nrm = S.normal(prim, a, b)
    dl = np.linalg.norm(d64[g], axis=1)
    tol = tolerance(c, e_mesh, t, (unit(d64[g]) * nrm).sum(1), dl) * dl
    ratio = off / tol
    print("%s: |o + t d - S(bcB, bcC)| worst %.3e, worst ratio to the tolerance %.3f over %d hits" % (name, off.max(), ratio.max(), len(g)))
    assert ratio.max() <= 1, "%s: ray %d is %.3e off the surface, tolerance %.3e" % (name, g[ratio.argmax()], off[ratio.argmax()], tol[ratio.argmax()])
    assert np.all(a >= -2e-5) and np.all(b >= -2e-5) and np.all(a + b <= 1 + 2e-5)
    assert np.all(t > org[g, 3]) and np.all(t < dirs[g, 3])
    assert np.all(np.abs(np.linalg.norm(hits["normal"][got].astype(np.float64), axis=1) - 1) < 1e-5)
    # misses report tmax (bit for bit, a NaN included); any-hit = 1 exactly where the closest-hit query finds something
    util.assert_same_bits(name + ": t of a miss", hits["dist"][~got], dirs[~got, 3])
    occ = host.trace(c["st"], api.TRACE_ANY, org, dirs)
    assert np.array_equal(occ == 1, got)
    special = hits[N_RAYS:-N_BAD]
    assert np.any(special["primIndex"] != api.GFX_INVALID_SLOT) and np.any(special["primIndex"] == api.GFX_INVALID_SLOT)


@pytest.mark.parametrize("name", MODEL_CASES)
def test_closest_hit_against_the_model(host, e_mesh, name):
    c = solved(host, name, model=True)
    S, m, hits, org, dirs = c["S"], c["m"], c["mhits"], c["mo"], c["md"]
    keep = kept(m, name)
    d64 = dirs[:, :3].astype(np.float64)
    got = hits["primIndex"] != api.GFX_INVALID_SLOT
    want = np.isfinite(m["t"])
    # closest and hit / miss on the rays the rule keeps
    bad = keep & (got != want)
    assert not bad.any(), "%s: hit / miss differs on %d kept rays, first %d: %s, model t %r" % (name, bad.sum(), np.nonzero(bad)[0][0], hits[bad][0], m["t"][bad][0])
    both = keep & want
    bad = both & (hits["primIndex"] != m["prim"])
    assert not bad.any(), "%s: primIndex differs on %d rays, first %d" % (name, bad.sum(), np.nonzero(bad)[0][0])
    nm = S.normal(m["prim"][both], m["alpha"][both], m["beta"][both])
    dlb = np.linalg.norm(d64[both], axis=1)
    cos = (unit(d64[both]) * nm).sum(1)
    tolb = tolerance(c, e_mesh, m["t"][both], cos, dlb)
    err = np.abs(hits["dist"][both].astype(np.float64) - m["t"][both])
    print("%s: |t - t64| worst %.3e, worst ratio to the tolerance %.3f over %d rays" % (name, err.max(), (err / tolb).max(), both.sum()))
    assert (err / tolb).max() <= 1, "%s: ray %d is off by %.3e, tolerance %.3e" % (name, np.nonzero(both)[0][(err / tolb).argmax()], err.max(), tolb[(err / tolb).argmax()])
    # the normal: unit, within the angle the distance tolerance implies, frontFace = the side the ray comes from
    n32 = hits["normal"][both].astype(np.float64)
    p, tc = S.p[m["prim"][both]], S.tc[m["prim"][both]]
    area_obj = np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    area_tex = np.abs(T._cross2(tc[:, 1] - tc[:, 0], tc[:, 2] - tc[:, 0])) * S.res ** 2
    w = np.sqrt(area_obj / area_tex)
    angle = np.arctan2(np.linalg.norm(np.cross(n32, nm), axis=1), (n32 * nm).sum(1))       # (arccos of a float32 dot product near 1 resolves 5e-4 rad)
    atol = tolb * dlb / w + 1e-5
    print("%s: normal off by at most %.3e rad, worst ratio to its tolerance %.3f" % (name, angle.max(), (angle / atol).max()))
    assert (angle / atol).max() <= 1
    sure = np.abs(cos) > 1e-4
    assert np.array_equal(hits["frontFace"][both][sure] == 1, cos[sure] < 0)
    if name == "cap":
        # the mirrored-uv triangle is exercised: hit, its normal on the side of +h like everyone's, without a negation for the mirroring
        last = len(c["t"]) - 1
        on_it = both & (m["prim"] == last)
        assert c["st"]["records"]["flipped"][last] == 1 and on_it.sum() >= 20
        print("cap: %d kept rays hit the mirrored-uv triangle, normal off by at most %.3e rad" % (on_it.sum(), angle[on_it[both]].max()))

@pytest.mark.parametrize("name", sorted(CASES))
def test_descent_terminates_below_its_ceiling(host, name):
    c = solved(host, name)
    # kMaxDescent = 2^22 iterations per base triangle and ray; a ray that is not finite enters nothing
    assert host.max_descent == 1 << 22
    print("%s: at most %d descent iterations on a base triangle (ceiling %d)" % (name, c["it"].max(), host.max_descent))
    assert c["it"].max() < host.max_descent
    bad = c["hits"][-N_BAD:]
    assert np.all(bad["primIndex"] == api.GFX_INVALID_SLOT) and np.all(c["it"][-N_BAD:] == 0)
    # a stricter statement for these maps: no more iterations than nodes below four roots of the 64 x 64 pyramid, visited and left
    assert c["it"].max() <= 2 * 4 * (4 ** 7 - 1) // 3


@pytest.mark.parametrize("name", sorted(CASES))
def test_surface_lies_inside_every_box_and_every_prism(host, name):
    c = solved(host, name)
    S, st = c["S"], c["st"]
    rec = st["records"]
    n = S.res
    rng = np.random.default_rng(11)
    prims = np.arange(len(rec)) if len(rec) <= 400 else rng.choice(len(rec), 400, replace=False)
    # the prism: minHeight <= base + scale h <= minHeight + amplitude over the footprint, densely sampled barycentrics
    g = np.linspace(0, 1, 41)
    a, b = np.meshgrid(g, g)
    inside = (a + b) <= 1
    a, b = a[inside], b[inside]
    w = np.stack([1 - a - b, a, b], 1)
    for pi in prims:
        assert rec["numRoots"][pi] > 0
        H = S.base + S.scale * S.height(w @ S.tc[pi])
        lo, hi = np.float64(rec["minHeight"][pi]), np.float64(rec["minHeight"][pi]) + np.float64(rec["amplitude"][pi])
        slack = 4 * 2.0 ** -24 * (abs(S.base) + abs(S.scale))
        assert H.min() >= lo - slack and H.max() <= hi + slack, "prism of triangle %d: heights [%g, %g] outside [%g, %g]" % (pi, H.min(), H.max(), lo, hi)
        # its box holds the six corners, hence (the shell is their convex hull) the surface
        corners = np.concatenate([S.p[pi] + lo * S.n[pi], S.p[pi] + hi * S.n[pi]])
        ext = np.abs(corners).max()
        assert np.all(corners >= st["aabbs"][pi, :3] - 4 * 2.0 ** -24 * ext) and np.all(corners <= st["aabbs"][pi, 3:] + 4 * 2.0 ** -24 * ext)
    # the descent's boxes: in (u, v, h) the surface IS h(u, v), affine per half texel, so its extremes over a texel of any level are
    # corner samples of level 0 inside the closed texel
    checked = 0
    for pi in prims[:60]:
        tex, mm = host.walk(st, int(pi))
        assert len(tex) > 0
        for (x, y, lod), (lo, hi) in zip(tex[:4000], mm[:4000]):
            span = 1 << min(int(lod), 6)
            xs = (np.arange(x * span, x * span + span + 1) if lod <= 6 else np.arange(n + 1)) % n
            ys = (np.arange(y * span, y * span + span + 1) if lod <= 6 else np.arange(n + 1)) % n
            h = S.corner[np.ix_(ys, xs)]          # (corner rows / columns n and 0 are the same samples under the repeat wrap)
            assert h.min() >= lo - 1e-7 and h.max() <= hi + 1e-7, "texel %s of triangle %d: heights [%g, %g] outside [%g, %g]" % ((x, y, lod), pi, h.min(), h.max(), lo, hi)
            checked += 1
    print("%s: %d prisms and %d descent boxes hold the model's surface" % (name, len(prims), checked))


def test_quad_agrees_with_the_micro_mesh_of_the_tfdm_tests(host, e_mesh):
    """On the quad every vertex normal is the same unit vector, so S is the flat micro-mesh: MicroMesh of tests/tfdm_host.py (same
    diagonal, same corner heights) traced by brute64 ties the model's yardstick to the one the project already trusts."""
    c = solved(host, "quad", model=True)
    org, dirs, hits = c["org"][:N_RAYS], c["dirs"][:N_RAYS], c["hits"][:N_RAYS]
    mm = T.MicroMesh(c["v"], c["t"], T.mips32(c["heights"]), c["gp"])
    t64, k64, edge, near = T.brute64(mm.A, mm.B, mm.C, org[:, :3], dirs[:, :3], org[:, 3].astype(np.float64), dirs[:, 3].astype(np.float64),
                                     clip=(mm.tA, mm.tB, mm.tC, mm.baseTc, mm.prim))
    flagged = edge | near
    assert flagged.mean() <= EDGE_CAP
    keep = ~flagged
    got, want = hits["primIndex"] != api.GFX_INVALID_SLOT, np.isfinite(t64)
    assert np.array_equal(got[keep], want[keep])
    both = keep & want
    assert np.array_equal(hits["primIndex"][both], mm.prim[k64[both]])
    d64 = dirs[both, :3].astype(np.float64)
    A, B, Cc = mm.A[k64[both]], mm.B[k64[both]], mm.C[k64[both]]
    nrm = unit(np.cross(B - A, Cc - A))
    dl = np.linalg.norm(d64, axis=1)
    tol = tolerance(c, e_mesh, t64[both], (unit(d64) * nrm).sum(1), dl)
    err = np.abs(hits["dist"][both].astype(np.float64) - t64[both])
    print("quad against MicroMesh: worst |t - t64| %.3e, worst ratio %.3f; the model against MicroMesh: %.3e"
          % (err.max(), (err / tol).max(), np.abs(c["m"]["t"][:N_RAYS][both] - t64[both]).max()))
    assert (err / tol).max() <= 1
    # ... and the model itself is that mesh
    assert np.abs(c["m"]["t"][:N_RAYS][both] - t64[both]).max() < 1e-12


def test_refused_parameters_have_a_text(host):
    assert host.refuse(api.tfdm_params(h_scale=0.1)) is None
    assert "targetMipLevel" in host.refuse(api.tfdm_params(target_mip_level=1))
    for mode in (api.TFDM_BOX, api.TFDM_BILINEAR, 2):
        assert "localIntersection" in host.refuse(api.tfdm_params(local_intersection=mode))
    assert "finite" in host.refuse(api.tfdm_params(h_scale=float("nan")))
    assert "finite" in host.refuse(api.tfdm_params(tex_offset=(float("inf"), 0.0)))
    assert "positive" in host.refuse(api.tfdm_params(tex_scale=(0.0, 1.0)))
    assert "positive" in host.refuse(api.tfdm_params(tex_scale=(1.0, -2.0)))


def test_cubic_solver_against_numpy(host):
    """solve_cubic on cubics with one, two and three roots in the range, against numpy.roots in float64 (1e-5 stopping width)."""
    rng = np.random.default_rng(5)
    worst, n = 0.0, 0
    for _ in range(2000):
        r = np.sort(rng.uniform(-0.5, 1.5, 3))
        k = rng.uniform(0.2, 3.0) * rng.choice([-1.0, 1.0])
        c = (k * np.poly(r))[::-1].astype(np.float32)                 # c0..c3
        exact = np.roots(c[::-1].astype(np.float64))
        exact = np.sort(exact[np.abs(exact.imag) < 1e-9].real)
        inside = exact[(exact > 0.02) & (exact < 0.98)]
        gaps = np.diff(exact)
        if len(exact) == 3 and gaps.min() < 0.05:
            continue                                                   # near-double roots: ill-conditioned in float32
        got = np.sort(host.cubic(c, 0.0, 1.0).astype(np.float64))
        got_in = got[(got > 0.02) & (got < 0.98)]
        assert len(got_in) == len(inside), "coefficients %s: %s, numpy %s" % (c, got, exact)
        if len(inside):
            worst = max(worst, np.abs(got_in - inside).max())
            n += len(inside)
    print("cubic: %d roots, worst error %.3e" % (n, worst))
    assert n > 1000 and worst <= 2e-5
