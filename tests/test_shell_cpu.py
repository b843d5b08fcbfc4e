"""CPU: the host compilation of csrc/nrtdsm/shell_core.hip.h and shell_build.h (tests/shell_host.cpp) against the float64 model
of the shell-mapped surface (tests/shell_ref.py), which shares no line with it and models the surface, not the algorithm.

Cases (tests/shell_host.py CASES): the "One Box" shell on the quad at 4 x 4 tiles, the same under a wrapped and rotated texture
transform (negative tile indices), on a 4 x 4-quad spherical cap with its mirrored-uv triangle at about 6 tiles per base edge and
with the whole cap inside one tile, the 309-face bunny on the quad at 3 x 3 tiles, and the box plus a second geometry on the cap.
3000 rays each and six rays that are NaN, infinite or of zero direction.

Edge rule (a condition on the rays under the model alone, asserted before anything is compared): a ray whose float64 closest hit lies
within 1e-4 in barycentrics of an edge of its base triangle or of its shell triangle, or within 1e-4 of a tile border in u or v, or
that crosses one of the model's flat facets while Newton's iteration finds no root anywhere (it grazes), is left out of the
comparison; at most EDGE_CAP (tests/test_nrtdsm_cpu.py) of the rays.

Distance tolerance: 8 * E_mesh * max(1, t) + 2 * 1e-5 * s / |cos theta|, DESIGN.md section 20's: kSolverEps in h on both sides.
Normal: within NORMAL_TOL of the model's dS/da x dS/db oriented by the winding; the worst measured angle is in DESIGN.md section 21
and NORMAL_TOL is one order above it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gfxexp_amd import api
from tests import shell_host as SH
from tests import shell_ref as SR
from tests import tfdm_host as T
from tests import util
from tests.test_nrtdsm_cpu import EDGE_CAP
from tests.test_tfdm_cpu import e_mesh      # noqa: F401 -- the fixture, measured exactly as there

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORMAL_TOL = 8.2e-5        # rad: one order over the worst measured angle, 8.144e-6 on quad_bunny
FACET_K = {"quad_box": 1, "quad_box_wrapped_rotated": 1, "quad_bunny": 1}     # affine on the quad: flat facets are exact; else 3


@pytest.fixture(scope="module")
def host(built_lib, tmp_path_factory):
    return SH.Host(tmp_path_factory.mktemp("shell_host"))


_SOLVED = {}


def solved(host, name):
    if name not in _SOLVED:
        v, t, geoms, gp, (org, dirs) = SH.case_inputs(name)
        st = host.state(v, t, geoms, gp)
        hits, cnt, it = host.trace(st, api.TRACE_CLOSEST, org, dirs, counters=True, iterations=True)
        S = SR.Surface(v, t, geoms, gp)
        m = S.trace(org[:, :3], dirs[:, :3], org[:, 3], dirs[:, 3], k=FACET_K.get(name, 3))
        _SOLVED[name] = dict(v=v, t=t, geoms=geoms, gp=gp, org=org, dirs=dirs, st=st, hits=hits, cnt=cnt, it=it, S=S, m=m)
    return _SOLVED[name]


def unit(d):
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def tolerance(S, e_mesh, t, cos, dlen):
    return 8 * e_mesh * np.maximum(1.0, t) + 2 * 1e-5 * abs(S.scale) / (np.maximum(np.abs(cos), 1e-12) * dlen)


@pytest.mark.parametrize("name", sorted(SH.CASES))
def test_the_model_alone_stays_within_the_edge_cap(host, name):
    m = solved(host, name)["m"]
    share = m["flagged"].mean()
    hit = np.isfinite(m["t"][:SH.N_RAYS]).mean()
    print("%s: edge rays %.2f %% of %d; %.1f %% of the rays hit" % (name, 100 * share, len(m["flagged"]), 100 * hit))
    assert share <= EDGE_CAP
    assert 0.1 < hit < 0.98


@pytest.mark.parametrize("name", sorted(SH.CASES))
def test_closest_hit_against_the_model(host, e_mesh, name):
    c = solved(host, name)
    S, m, hits, org, dirs = c["S"], c["m"], c["hits"], c["org"], c["dirs"]
    keep = ~m["flagged"]
    assert (~keep).mean() <= EDGE_CAP
    d64 = dirs[:, :3].astype(np.float64)
    got, want = hits["primIndex"] != api.GFX_INVALID_SLOT, np.isfinite(m["t"])
    bad = keep & (got != want)
    assert not bad.any(), "%s: hit / miss differs on %d kept rays, first %d: %s, model t %r" % (name, bad.sum(), np.nonzero(bad)[0][0], hits[bad][0], m["t"][bad][0])
    both = keep & want
    for field, ref in (("primIndex", m["prim"]), ("shellTriangle", m["tri"]), ("shellGeom", S.geom[m["tri"]])):
        bad = both & (hits[field] != ref)
        assert not bad.any(), "%s: %s differs on %d rays, first %d" % (name, field, bad.sum(), np.nonzero(bad)[0][0])
    bad = both & np.any(hits["tile"] != m["tile"], axis=1)
    assert not bad.any(), "%s: tile differs on %d rays" % (name, bad.sum())
    tile = m["tile"][both].astype(np.float64)
    nm = S.normal(m["prim"][both], tile, m["tri"][both], m["a"][both], m["b"][both])
    dl = np.linalg.norm(d64[both], axis=1)
    cos = (unit(d64[both]) * nm).sum(1)
    tol = tolerance(S, e_mesh, m["t"][both], cos, dl)
    err = np.abs(hits["dist"][both].astype(np.float64) - m["t"][both])
    print("%s: |t - t64| worst %.3e, worst ratio to the tolerance %.3f over %d rays" % (name, err.max(), (err / tol).max(), both.sum()))
    assert (err / tol).max() <= 1
    # the hit point lies on the model's surface: S of the reported base barycentrics at the model's height there
    o64 = org[both, :3].astype(np.float64)
    hp = o64 + hits["dist"][both].astype(np.float64)[:, None] * d64[both]
    off = np.linalg.norm(hp - S.point(m["prim"][both], tile, m["tri"][both], m["a"][both], m["b"][both]), axis=1)
    print("%s: |o + t d - S| worst %.3e, worst ratio %.3f" % (name, off.max(), (off / (tol * dl)).max()))
    assert (off / (tol * dl)).max() <= 1
    bc = np.abs(hits["bcB"][both] - m["alpha"][both]) + np.abs(hits["bcC"][both] - m["beta"][both])
    assert bc.max() < 1e-3
    # the normal: unit, on the winding's side, frontFace the side the ray comes from
    n32 = hits["normal"][both].astype(np.float64)
    assert np.all(np.abs(np.linalg.norm(n32, axis=1) - 1) < 1e-5)
    angle = np.arctan2(np.linalg.norm(np.cross(n32, nm), axis=1), (n32 * nm).sum(1))
    print("%s: normal off by at most %.3e rad" % (name, angle.max()))
    assert angle.max() <= NORMAL_TOL
    sure = np.abs(cos) > 1e-4
    assert np.array_equal(hits["frontFace"][both][sure] == 1, cos[sure] < 0)
    if name.startswith("cap"):
        last = len(c["t"]) - 1
        on_it = both & (m["prim"] == last)
        assert c["st"]["records"]["flipped"][last] == 1 and on_it.sum() >= 5, on_it.sum()
        print("%s: %d kept rays hit the mirrored-uv triangle, normal off by at most %.3e rad" % (name, on_it.sum(), angle[on_it[both]].max()))
    if name == "cap_two_geoms":
        assert set(np.unique(hits["shellGeom"][both])) == {0, 1} and hits["shellTriangle"][both].max() >= 12
    if name == "quad_box_wrapped_rotated":
        assert hits["tile"][both].min() < 0
    # misses report tmax bit for bit and zero new fields; any-hit = 1 exactly where the closest-hit query finds something
    util.assert_same_bits(name + ": t of a miss", hits["dist"][~got], dirs[~got, 3])
    assert not hits["shellTriangle"][~got].any() and not hits["shellGeom"][~got].any() and not hits["tile"][~got].any()
    occ = host.trace(c["st"], api.TRACE_ANY, org, dirs)
    assert np.array_equal(occ == 1, got)
    assert c["cnt"][2] == len(org) and c["cnt"][0] > 0 and c["cnt"][1] > 0 and c["cnt"][3] > 0


@pytest.mark.parametrize("name", sorted(SH.CASES))
def test_iterations_stay_below_the_static_bound(host, name):
    c = solved(host, name)
    assert host.max_descent == 1 << 22
    print("%s: at most %d iterations on a base triangle (ceiling %d)" % (name, c["it"].max(), host.max_descent))
    assert c["it"].max() < host.max_descent
    bad = c["hits"][-SH.N_BAD:]
    assert np.all(bad["primIndex"] == api.GFX_INVALID_SLOT) and np.all(c["it"][-SH.N_BAD:] == 0)


def _leaves_under(nodes, k):
    out, todo = [], [k]
    while todo:
        n = nodes[todo.pop()]
        if n["count"]:
            out.append(int(n["first"]))
        else:
            todo += [int(n["first"]), int(n["first"]) + 1]
    return out


@pytest.mark.parametrize("name", sorted(SH.CASES))
def test_every_box_and_every_prism_holds_the_surface(host, name):
    c = solved(host, name)
    S, st = c["S"], c["st"]
    rec, nodes = st["records"], st["shell_nodes"]
    prims = np.arange(len(rec))
    under = {}
    g = np.linspace(0, 1, 13)
    a, b = np.meshgrid(g, g)
    ins = (a + b) <= 1
    a, b = a[ins], b[ins]
    boxes = 0
    for pi in prims:
        cand = S.candidates(pi)
        lo, hi = np.float64(rec["minHeight"][pi]), np.float64(rec["minHeight"][pi]) + np.float64(rec["amplitude"][pi])
        if not cand:
            continue
        assert rec["numRoots"][pi] > 0
        # the prism: every point of the shell mesh over the footprint has its height inside [minHeight, minHeight + amplitude]
        for tile, tris in cand:
            x = S.uvh(np.array(tile, np.float64)[None, None], tris[:, None], a[None], b[None])
            w = S.at(pi, x)[2]
            inside = w.min(-1) >= 0
            if inside.any():
                H = S.base + S.scale * x[..., 2][inside]
                slack = 4 * 2.0 ** -24 * (abs(S.base) + abs(S.scale) * max(abs(S.hlo), abs(S.hhi)))
                assert H.min() >= min(lo, hi) - slack and H.max() <= max(lo, hi) + slack, "prism of triangle %d" % pi
        corners = np.concatenate([S.p[pi] + lo * S.n[pi], S.p[pi] + hi * S.n[pi]])
        ext = np.abs(corners).max()
        assert np.all(corners >= st["aabbs"][pi, :3] - 4 * 2.0 ** -24 * ext) and np.all(corners <= st["aabbs"][pi, 3:] + 4 * 2.0 ** -24 * ext)
        if pi % 7:
            continue
        # the boxes the traversal enters: in (u, v, h) the surface IS the shell mesh
        ids, bx = host.walk(st, int(pi))
        assert len(ids) > 0
        for (tx, ty, lod, node), bb in zip(ids[:3000], bx[:3000]):
            if node < 0:
                assert bb[2] <= S.hlo and bb[5] >= S.hhi and bb[3] - bb[0] == 2.0 ** lod
                continue
            if node not in under:
                under[node] = S.m[_leaves_under(nodes, node)].reshape(-1, 3)
            pts = under[node] + np.array([tx, ty, 0.0])
            eps = 2.0 ** -22 * max(1.0, abs(tx), abs(ty))
            assert np.all(pts >= bb[:3] - eps) and np.all(pts <= bb[3:] + eps), "node %d in tile (%d, %d)" % (node, tx, ty)
            boxes += 1
    print("%s: %d prisms and %d shell-node boxes hold the model's surface" % (name, len(prims), boxes))
    assert boxes > 0


def test_one_whole_tile_inside_a_triangle_gives_the_roots_range(host):
    """The height range of a base triangle that holds a whole tile is the shell BVH root's; the one-tile cap climbs to level 0 roots."""
    c = solved(host, "quad_box")
    rec, S = c["st"]["records"], c["S"]
    assert np.allclose(rec["minHeight"], S.base + S.scale * S.hlo) and np.allclose(rec["amplitude"], S.scale * (S.hhi - S.hlo))
    assert np.all(rec["rootLod"] == 2) and np.all(rec["numRoots"] == 4)      # [0, 4]^2: floor(4 / 4) = 1, two squares per axis
    one = solved(host, "cap_box_one_tile")["st"]["records"]
    assert np.all(one["rootLod"] == 0) and np.all(one["numRoots"][one["numRoots"] > 0] == 1)


def test_refusals_have_a_text(host):
    assert host.refuse(api.shell_params(h_scale=0.1)) is None
    assert "targetMipLevel" in host.refuse(api.tfdm_params(target_mip_level=1, local_intersection=0))
    for mode in (api.TFDM_TWO_TRIANGLE, api.TFDM_BILINEAR, 2):
        assert "localIntersection" in host.refuse(api.tfdm_params(local_intersection=mode))
    assert "finite" in host.refuse(api.shell_params(h_scale=float("nan")))
    assert "positive" in host.refuse(api.shell_params(tex_scale=(0.0, 1.0)))
    pos, tri = api.shell_box()
    with pytest.raises(SH.Refused, match="no shell geometry"):
        host.build([])
    with pytest.raises(SH.Refused, match="no triangles"):
        host.build([(pos, np.zeros((0, 3), np.uint32))])
    with pytest.raises(SH.Refused, match="more than 8"):
        host.build([(pos, tri)] * 9)
    bad = pos.copy()
    bad[3, 2] = np.nan
    with pytest.raises(SH.Refused, match="not finite"):
        host.build([(bad, tri)])
    bad = pos.copy()
    bad[3, 0] = 1.25
    with pytest.raises(SH.Refused, match=r"outside \[0, 1\]"):
        host.build([(bad, tri)])
    with pytest.raises(SH.Refused, match="does not exist"):
        host.build([(pos, tri + 1)])
    big = np.zeros(((1 << 20) + 1, 3), np.uint32)
    with pytest.raises(SH.Refused, match="2\\^20"):
        host.build([(pos, big)])
    v, t = T.quad_mesh()
    with pytest.raises(SH.Refused, match="2\\^22"):
        host.state(v, t, [(pos, tri)], api.shell_params(tex_offset=(5.0e6, 0.0)))
    # eight geometries are fine, and so is a flat decal at h = 0: it is hit from above
    host.build([(pos, tri)] * 8)
    flat = pos.copy()
    flat[:, 2] = 0.0
    st = host.state(v, t, [(flat[:4], np.array([[0, 1, 3], [0, 3, 2]], np.uint32))], api.shell_params(tex_scale=(2.0, 2.0)))
    o, d = T.pack_rays(np.array([[0.25, 0.25, 1.0], [0.02, 0.02, 1.0]]), np.array([[0.0, 0.0, -1.0], [0.0, 0.0, -1.0]]))
    h = host.trace(st, api.TRACE_CLOSEST, o, d)
    assert h["primIndex"][0] != api.GFX_INVALID_SLOT and abs(h["dist"][0] - 1.0) < 1e-6 and h["normal"][0, 2] > 0.999 and h["frontFace"][0] == 1
    assert h["primIndex"][1] == api.GFX_INVALID_SLOT


def test_fit_and_box_against_numbers_written_here(built_lib):
    pos, tri = api.shell_box()
    assert pos.min(0).tolist() == [np.float32(0.2), np.float32(0.2), 0.0] and pos.max(0).tolist() == [np.float32(0.8), np.float32(0.8), np.float32(0.08)]
    assert tri.shape == (12, 3) and sorted(np.unique(tri)) == list(range(8))
    # closed and outward: every edge once in each direction, every normal away from the centre
    edges = [(int(t[k]), int(t[(k + 1) % 3])) for t in tri for k in range(3)]
    assert len(set(edges)) == 36 and all((b, a) in set(edges) for a, b in edges)
    p = pos[tri].astype(np.float64)
    nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert np.all((nrm * (p.mean(1) - np.array([0.5, 0.5, 0.04]))).sum(1) > 0)
    pts = np.array([[1.0, 2.0, 3.0], [5.0, 4.0, 3.5], [3.0, 2.5, 7.0]], np.float32)
    np.testing.assert_allclose(api.shell_fit(pts), [[0.0, 0.25, 0.0], [1.0, 0.75, 0.125], [0.5, 0.375, 1.0]], atol=1e-7)
    # Y-up: (x, y, z) -> (x, -z, y) first; then dx = 4, dy = 4: scale 1/4, the lowest y (2.0) to height 0
    np.testing.assert_allclose(api.shell_fit(pts, y_up=True), [[0.0, 1.0, 0.0], [1.0, 0.875, 0.5], [0.5, 0.0, 0.125]], atol=1e-7)
    with pytest.raises(api.GfxError):
        api.shell_fit(np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.0]], np.float32))


def test_symbols_are_declared_exported_and_mirrored(built_lib):
    header = open(os.path.join(ROOT, "include", "gfxexp.h")).read()
    for name in ("gfx_shell_create", "gfx_shell_set_params", "gfx_shell_set_geometry", "gfx_shell_destroy", "gfx_shell_trace", "gfx_shell_read", "gfx_shell_size"):
        assert re.search(r"\b%s\s*\(" % name, header) and hasattr(built_lib, name) and name in api.C_ABI_SYMBOLS
    for name in ("gfxh_shell_fit", "gfxh_shell_box"):
        assert hasattr(built_lib, name) and name in api.HOST_ABI_SYMBOLS
    layout = api.abi_layout()
    assert layout["gfx_shell_hit"]["size"] == 48 == api.SHELL_HIT_DTYPE.itemsize == C.sizeof(api.GfxShellHit)
    dt = api.SHELL_HIT_DTYPE
    assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names] == layout["gfx_shell_hit"]["fields"]
    assert api.abi_mirrors()["gfx_shell_hit"] is api.GfxShellHit and api.abi_mirrors()["gfx_shell_geom"] is api.GfxShellGeom
    for m in ("set_params", "set_geometry", "trace", "read_shell_nodes", "read_shell_triangles", "device_bytes"):
        assert hasattr(api.Shell, m)
    assert built_lib.gfx_shell_destroy(None) == 1
