"""Adversarial cases for the BVH8 build and traversal: scenes generated in code, ray sets at the geometric edges of the slab test,
and a float64 brute-force reference (tests/test_oracle_trace_edges.py on the CPU, tests/test_gpu_trace_edges.py on the GPU).

A case is a HostScene together with its world-space triangles in float64 (computed here from the scene's own vertex arrays and
instance transforms, in the flattened order: instance slot ascending, group list order, primitive index), their
(instSlot, geomInstSlot, primIndex), and the same triangles rounded the way the product's and the oracle's flatten round them
(((m0 x + m1 y) + m2 z) + m3 in fp32).  The float64 reference decides, per ray, whether the answer is ROBUST -- far enough from
every rounding decision of the fp32 triangle test that any correct traversal must return it.  The reference runs on the
flattened triangles (the fp32 ones, exactly, in float64): what the flatten's rounding does to a scene 1e6 from the origin is
pinned on its own, against the float64 triangles.  Robust means:
  * a robust hit: the nearest candidate has every barycentric above max(1e-4, its fp32 error bound), lies inside (tmin, tmax) by
    max(1e-5 relative, its fp32 distance error bound), and every other candidate is farther by as much;
  * a robust miss: no triangle comes within those margins.
The fp32 error bounds of the triangle test (first order, times a safety factor) only matter where the plain 1e-4 / 1e-5 margins
are too thin for fp32 -- far origins, grazing rays, triangles a few ulps wide; elsewhere the plain margins decide."""
import os

import numpy as np

from gfxexp_amd import api
from tests import util

ASSETS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "assets")
BUNNY = os.path.join(ASSETS, "stanford_bunny_309_faces.obj")
FLT_MAX = np.float32(3.4028234663852886e+38)
U32 = 2.0 ** -24                 # unit roundoff of fp32
ERR_K = 16.0                     # safety factor on the first-order fp32 error bounds
BC_MARGIN, T_MARGIN = 1e-4, 1e-5
PAIR_CHUNK = 1 << 19             # rays x triangles the float64 reference evaluates at once


# ---------------------------------------------------------------------------------------------------------------- scenes
def world_triangles(hs, transforms=None):
    """(float64 world triangles (n, 3, 3), fp32 world triangles (n, 3, 3), ids (n,) TRI_IDS_DTYPE) of a HostScene, in flattened
    order.  `transforms`: {instSlot: xfm12} overriding the scene's own (an animated update)."""
    geoms = [(v["position"].astype(np.float32), t.astype(np.int64)) for v, t, _ in hs.geoms()]
    groups = hs.groups()
    w64, w32, ids = [], [], []
    for inst, (g, x) in enumerate(hs.instances()):
        if transforms and inst in transforms:
            x = np.asarray(transforms[inst], np.float32)
        m = x.reshape(3, 4).astype(np.float32)
        m64 = m.astype(np.float64)
        for gs in groups[g]:
            pos, tri = geoms[int(gs)]
            v = pos[tri]                                                 # (k, 3 vertices, 3) float32
            w64.append(v.astype(np.float64) @ m64[:, :3].T + m64[:, 3])
            r = np.empty_like(v)
            for row in range(3):                                         # xfmPoint of the flatten, operation by operation
                r[..., row] = ((m[row, 0] * v[..., 0] + m[row, 1] * v[..., 1]) + m[row, 2] * v[..., 2]) + m[row, 3] * np.float32(1.0)
            w32.append(r)
            rec = np.zeros(len(tri), api.TRI_IDS_DTYPE)
            rec["instSlot"], rec["geomInstSlot"], rec["primIndex"] = inst, int(gs), np.arange(len(tri))
            ids.append(rec)
    return np.concatenate(w64), np.concatenate(w32), np.concatenate(ids)


class Case:
    """A scene of the adversarial set.  `dynamic`: instance slots declared animated; `moves`: {slot: xfm12} of the transform
    update that follows the first build (animated cases); `max_leaf`: gfx_accel_set_max_leaf of the GPU build (None = default)."""

    def __init__(self, name, hs, dynamic=(), moves=None, max_leaf=None):
        self.name, self.hs, self.dynamic, self.moves, self.max_leaf = name, hs, tuple(dynamic), moves, max_leaf
        self.set_state(final=False)

    def set_state(self, final):
        """Select the triangles before (final=False) or after (final=True) the animated update."""
        self.tris64, self.tris32, self.ids = world_triangles(self.hs, self.moves if final else None)
        pts = self.tris64.reshape(-1, 3)
        self.lo, self.hi = pts.min(0), pts.max(0)
        self.centre = 0.5 * (self.lo + self.hi)
        self.extent = float(np.linalg.norm(self.hi - self.lo))
        return self

    def flat_index(self, ids):
        """(instSlot, geomInstSlot, primIndex) records -> position in the flattened triangle list (-1: no triangle of the case)."""
        def key(r):
            return (r["instSlot"].astype(np.int64) << 42) | (r["geomInstSlot"].astype(np.int64) << 21) | r["primIndex"].astype(np.int64)
        mine = key(self.ids)
        order = np.argsort(mine)
        want = key(ids)
        pos = np.clip(np.searchsorted(mine[order], want), 0, len(mine) - 1)
        return np.where(mine[order][pos] == want, order[pos], -1)


def _vertices(p):
    p = np.asarray(p, np.float32).reshape(-1, 3)
    v = np.zeros(len(p), api.VERTEX_DTYPE)
    v["position"] = p
    v["normal"] = (0, 0, 1)
    v["texCoord0Dir"] = (1, 0, 0)
    return v


def _soup(hs, mat, tris):
    """One geometry of independent triangles (m, 3, 3) -> geom slot."""
    tris = np.asarray(tris, np.float32).reshape(-1, 3, 3)
    return hs.add_geom(_vertices(tris.reshape(-1, 3)), np.arange(3 * len(tris)).reshape(-1, 3), mat)


def _new_scene():
    hs = api.HostScene()
    return hs, hs.add_material_traditional((0.6, 0.6, 0.6), (0.04, 0.04, 0.04), 0.2)


def _box_tris(lo, hi):
    """12 triangles of an axis-aligned box (zero extents allowed: faces coincide or collapse to zero area)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c = np.array([[hi[0] if i & 1 else lo[0], hi[1] if i & 2 else lo[1], hi[2] if i & 4 else lo[2]] for i in range(8)])
    out = []
    for a, b, cc, d in [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]:
        out += [(c[a], c[b], c[cc]), (c[a], c[cc], c[d])]
    return np.array(out)


def _quad(origin, u, v):
    o, u, v = (np.asarray(x, np.float64) for x in (origin, u, v))
    return np.array([(o, o + u, o + u + v), (o, o + u + v, o + v)])


def offset_case(offset, scale=0.1, name=None):
    """The bunny (309 triangles, at the benchmark's scale 0.1) moved by `offset` along (1, 0.5, -0.75), or scaled by `scale`.
    At 1e6 the fp32 spacing is 0.0625: the flattened vertices land on a coarse grid and many triangles collapse."""
    hs = api.HostScene()
    hs.add_instance(hs.load_obj(BUNNY), api.make_transform(scale=scale, pos=tuple(float(offset) * np.array([1.0, 0.5, -0.75]))))
    return Case(name or f"bunny_offset_{offset:g}", hs)


def mixed_scale_case():
    """A box room 10^4 across ([-2e3, 8e3]^3, walls facing in) holding clusters of 40 triangles about 1e-3 in size: by three walls,
    in the middle, and at the corner far from the origin (coordinates near 8e3, fp32 spacing 2^-11: triangles two ulps wide)."""
    hs, mat = _new_scene()
    room = _box_tris((-2e3, -2e3, -2e3), (8e3, 8e3, 8e3))[:, ::-1]
    hs.add_instance(hs.add_group([_soup(hs, mat, room)]), api.make_transform())
    rng = np.random.default_rng(5)
    centres = [(3e3, 3e3, -2e3 + 0.5), (8e3 - 0.5, 3e3, 3e3), (3e3, -2e3 + 0.02, 3e3), (3e3, 3e3, 3e3),
               (8e3 - 1.0, 8e3 - 1.0, 8e3 - 1.0), (8e3 - 0.01, 8e3 - 0.3, 8e3 - 0.2)]
    tris = [np.asarray(c) + rng.uniform(-0.02, 0.02, (40, 1, 3)) + rng.uniform(-1e-3, 1e-3, (40, 3, 3)) for c in centres]
    hs.add_instance(hs.add_group([_soup(hs, mat, np.concatenate(tris))]), api.make_transform())
    return Case("mixed_scale_room", hs)


def axis_aligned_case():
    """Quads in the x, y and z planes, boxes with one extent zero (their two big faces coincide, their side faces have no area),
    closed unit cubes, and a coplanar stack of quads 0, 1, 2 and 4 ulps apart.  Identity transforms: the fp32 triangles are exact."""
    hs, mat = _new_scene()
    tris = []
    for k, (u, v, n) in enumerate([((1, 0, 0), (0, 1, 0), 2), ((0, 1, 0), (0, 0, 1), 0), ((0, 0, 1), (1, 0, 0), 1)]):
        for j in range(3):
            o = np.zeros(3)
            o[n], o[(n + 1) % 3] = 1.0 + 0.5 * j, -1.0 + 0.75 * k
            tris.append(_quad(o, np.asarray(u) * 1.5, np.asarray(v) * 1.25))
    tris += [_box_tris((2, 0, 0), (3, 1, 0)), _box_tris((2, 2, 0), (2, 3, 1)), _box_tris((0, 3, 2), (1, 3, 3)),
             _box_tris((-2, -2, -2), (-1, -1, -1)), _box_tris((4, 0, 0), (5, 1, 1))]
    z = np.float32(2.5)
    for ulps in (0, 1, 2, 4):
        zz = z
        for _ in range(ulps):
            zz = np.nextafter(zz, np.float32(np.inf))
        tris.append(_quad((-3.0, 2.0, float(zz)), (1, 0, 0), (0, 1, 0)))
    hs.add_instance(hs.add_group([_soup(hs, mat, np.concatenate(tris))]), api.make_transform())
    return Case("axis_aligned", hs)


def degenerate_case():
    """Zero-area triangles (collinear vertices, repeated vertices) between ordinary ones; exact duplicates, inside one geometry
    and in a second instance at the same transform (the closest-hit tie rule on the flattened index); and
    triangles that all have the same bounding-box centre (Morton ties)."""
    hs, mat = _new_scene()
    rng = np.random.default_rng(11)
    base = rng.uniform(-1, 1, (40, 1, 3)) + rng.uniform(-0.3, 0.3, (40, 3, 3))
    coll = rng.uniform(-1, 1, (20, 1, 3)) + rng.uniform(-0.3, 0.3, (20, 1, 3)) * np.array([0.0, 0.5, 1.0])[None, :, None]
    rep = rng.uniform(-1, 1, (20, 3, 3))
    rep[:, 2] = rep[:, 1]
    dup = np.repeat(base[:8], 3, axis=0)
    c, r = np.array([0.25, 0.5, -0.25]), 0.3
    corners = np.array([[c[0] + (r if i & 1 else -r), c[1] + (r if i & 2 else -r), c[2] + (r if i & 4 else -r)] for i in range(8)])
    same_centre = np.array([(corners[a], corners[b], corners[7 - a]) for a in range(8) for b in range(8) if b not in (a, 7 - a)][:24])
    hs.add_instance(hs.add_group([_soup(hs, mat, np.concatenate([base, coll, rep, dup, same_centre]))]), api.make_transform())
    hs.add_instance(hs.add_group([_soup(hs, mat, base[:12])]), api.make_transform())
    return Case("degenerate", hs)


SIZES = (1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65, 4097)


def sizes_case(n, max_leaf=None):
    """n random triangles in a box about 2 across: the one-node subtree (n <= 8), the general builder just above it, and around
    the 64- and 4096-triangle marks."""
    hs, mat = _new_scene()
    rng = np.random.default_rng(1000 + n)
    size = 0.6 / max(1.0, n ** (1 / 3))
    hs.add_instance(hs.add_group([_soup(hs, mat, rng.uniform(-1, 1, (n, 1, 3)) + rng.uniform(-size, size, (n, 3, 3)))]),
                    api.make_transform())
    return Case(f"sizes_{n}" + (f"_leaf{max_leaf}" if max_leaf else ""), hs, max_leaf=max_leaf)


DEEP_LEVELS = 18


def _nest_level_tris(s):
    """One level of the nest in the cube [0, s]^3: a triangle spanning each of the octants 1..7 (its box is the octant), and in
    octant 7 a cluster of three small triangles beside it, so that octant is an internal child.  A ray through the corner meets
    both the next level (octant 0) and octant 7, and descending into the first pushes the second."""
    h = 0.5 * s
    out = []
    for k in range(1, 8):
        lo = np.array([h if k & 1 else 0.0, h if k & 2 else 0.0, h if k & 4 else 0.0])
        out.append((lo + (0, 0, h), lo + (h, 0, 0), lo + (0, h, 0)))
    for j in range(3):
        c = np.array([0.9, 0.88 - 0.05 * j, 0.6 + 0.1 * j]) * s
        out.append((c, c + (s / 32, 0, 0), c + (0, s / 32, s / 64)))
    return np.array(out)


def _emitter(hs):
    return hs.add_material_traditional((0.01, 0.01, 0.01), (0, 0, 0), 0.3, (20.0, 18.0, 15.0))


def deep_case(levels=DEEP_LEVELS):
    """A self-similar nest in [0, 1]^3 that halves per level down to 2^-levels (8 Morton cells at 21 bits per axis): every wide
    node should be seven octants plus the next level.  The level-0 octant triangles are emitters (a light for the path tracer
    that does not change the root box)."""
    hs, mat = _new_scene()
    top = _nest_level_tris(1.0)
    geoms = [_soup(hs, _emitter(hs), top[:7]), _soup(hs, mat, top[7:])]
    geoms += [_soup(hs, mat, _nest_level_tris(2.0 ** -lvl)) for lvl in range(1, levels)]
    s = 2.0 ** -levels
    geoms.append(_soup(hs, mat, [((0, 0, s), (s, 0, 0), (0, s, 0))]))        # the innermost octant 0
    hs.add_instance(hs.add_group(geoms), api.make_transform())
    return Case("deep_nest", hs)


def animated_deep_case(levels=DEEP_LEVELS):
    """The nest of deep_case as one declared-animated instance per level (the unit-cube level scaled by 2^-level), built lined up
    side by side along +x -- a shallow animated subtree -- and then moved into the nest by a transform update: the in-place
    rebuild of the animated subtree gets deeper.  A static emissive quad above the nest."""
    hs, mat = _new_scene()
    hs.add_instance(hs.add_group([_soup(hs, _emitter(hs), _quad((0.0, 1.5, 0.0), (0, 0, 1), (1, 0, 0)))]), api.make_transform())
    unit = hs.add_group([_soup(hs, mat, _nest_level_tris(1.0))])
    last = hs.add_group([_soup(hs, mat, [((0, 0, 1), (1, 0, 0), (0, 1, 0))])])
    slots, moves = [], {}
    for lvl in range(levels + 1):
        sc = 2.0 ** -lvl
        slot = hs.add_instance(unit if lvl < levels else last, api.make_transform(scale=sc, pos=(2.0 + 1.5 * lvl, 0.0, 0.0)))
        slots.append(slot)
        moves[slot] = api.make_transform(scale=sc)
    return Case("animated_nest", hs, dynamic=slots, moves=moves)


# every scene but the size sweep, by name (built on demand: a HostScene needs the product's library)
SCENES = {
    "bunny_offset_1e3": lambda: offset_case(1e3),
    "bunny_offset_1e5": lambda: offset_case(1e5),
    "bunny_offset_1e6": lambda: offset_case(1e6),
    "bunny_tiny": lambda: offset_case(0.0, scale=1e-4, name="bunny_tiny"),
    "mixed_scale_room": mixed_scale_case,
    "axis_aligned": axis_aligned_case,
    "degenerate": degenerate_case,
    "deep_nest": deep_case,
    "animated_nest": animated_deep_case,
}
STATES = [(name, False) for name in SCENES] + [("animated_nest", True)]      # (scene, after its animated update)


def oracle_for(case, final=False, max_leaf=None):
    """The oracle's scene for `case` (after its animated update when final), SAH builder with max_leaf triangles per leaf."""
    config = None if max_leaf is None else [0.3, 1.2, 1.0, 1, max_leaf]
    osc = util.feed_oracle(case.hs, config=config)
    if final:
        for slot, xfm in case.moves.items():
            osc.set_instance_transform(slot, xfm)
        osc.commit(config=config)
    return osc


def all_rays(case, osc, seed=0):
    """Every ray set of a case, the interval edges at the oracle's brute-force distances included."""
    sets = ray_sets(case, seed)
    sets["interval_edges"] = edge_rays(case, osc)
    return sets


def flat_hits(hits):
    """The oracle's triIndex is the flattened triangle index; -1 for a miss."""
    return np.where(hits["triIndex"] != api.GFX_INVALID_SLOT, hits["triIndex"].astype(np.int64), -1)


# ---------------------------------------------------------------------------------------------------------------- rays
def _rays(o, d, tmin=0.0, tmax=FLT_MAX):
    o = np.asarray(o, np.float32).reshape(-1, 3)
    d = np.asarray(d, np.float32).reshape(-1, 3)
    n = max(len(o), len(d))
    org = np.zeros((n, 4), np.float32)
    org[:, :3], org[:, 3] = o, tmin
    dirs = np.zeros((n, 4), np.float32)
    dirs[:, :3], dirs[:, 3] = d, tmax
    return org, dirs


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _budget(case, want):
    """Rays of a set: `want`, fewer for big scenes (rays x triangles of a set stays near 2^21)."""
    return int(max(64, min(want, (1 << 21) // max(1, len(case.tris64)))))


def pinhole(case, n=None, cam=None, look=None):
    res = max(4, int(np.sqrt(n or _budget(case, 2304))))
    cam = case.centre + np.array([0.35, 0.3, 0.9]) * case.extent if cam is None else np.asarray(cam)
    return util.pinhole_rays(res, res, cam, case.centre if look is None else look)


def segments(case, rng, n=None):
    """Random segments between two points of the scene box grown by 20 %; unit directions, tmax = 0.9999 of the length."""
    n = n or _budget(case, 2000)
    grow = 0.2 * (case.hi - case.lo) + 1e-3
    p0 = rng.uniform(case.lo - grow, case.hi + grow, (n, 3)).astype(np.float32).astype(np.float64)
    p1 = rng.uniform(case.lo - grow, case.hi + grow, (n, 3))
    length = np.linalg.norm(p1 - p0, axis=1)
    return _rays(p0, (p1 - p0) / length[:, None], 0.0, (length * 0.9999).astype(np.float32))


SPECIAL_COMPONENTS = np.array([0.0, -0.0, 1e-40, -1e-40, 1e-21, -1e-21, 1e-45], np.float32)   # +-0, denormals, below the clamp


def axis_parallel(case, rng, n=None):
    """Directions with one or two components exactly +0 / -0 / denormal / about 1e-21 and the others of ordinary size, from a point
    of the grown scene box toward a triangle; half of the origin coordinates are vertex coordinates of the scene (rays in the planes
    of axis-aligned geometry).  The GPU traversal's box tests treat a component below 1e-20 as 1e-20 (bvh8.hip.h Traversal::begin),
    which is like an axis-parallel ray only while another component is of ordinary size: a direction whose every component is tiny
    (length 1e-21, hits at t ~ 1e21) has its boxes culled by the clamp, and is outside what these sets ask of the traversal."""
    n = n or _budget(case, 1500)
    grow = 0.1 * (case.hi - case.lo) + 1e-3
    o = rng.uniform(case.lo - grow, case.hi + grow, (n, 3)).astype(np.float32)
    verts = case.tris32.reshape(-1, 3)
    from_verts = verts[rng.integers(0, len(verts), (n, 3)), np.arange(3)[None, :]]
    o = np.where(rng.random((n, 3)) < 0.5, from_verts, o).astype(np.float32)
    target = case.tris64[rng.integers(0, len(case.tris64), n)].mean(axis=1)
    d = _unit(target - o.astype(np.float64) + 1e-30).astype(np.float32)
    for i in range(n):
        axes = rng.choice(3, size=1 + (i % 2), replace=False)
        d[i, axes] = SPECIAL_COMPONENTS[rng.integers(0, len(SPECIAL_COMPONENTS), len(axes))]
        rest = [k for k in range(3) if k not in axes]
        if np.max(np.abs(d[i, rest])) < 0.1:        # the other components carry the ray
            d[i, rest[0]] = 1.0 if rng.random() < 0.5 else -1.0
    return _rays(o, d)


def non_unit(case, rng, n=None):
    """Directions toward random scene points with lengths from 1e-3 to 1e3 (tmax FLT_MAX)."""
    n = n or _budget(case, 1500)
    cam = case.centre + np.array([-0.4, 0.7, 0.8]) * case.extent
    target = case.tris64[rng.integers(0, len(case.tris64), n)].mean(axis=1) + rng.normal(0, 0.05 * case.extent, (n, 3))
    return _rays(np.broadcast_to(cam, (n, 3)), _unit(target - cam) * (10.0 ** rng.uniform(-3, 3, (n, 1))))


def on_planes(case, rng, n=None):
    """Origins exactly on geometry: a triangle's vertex, a face plane of a triangle's box or of the scene box, or inside a
    triangle's box; half of the directions graze along the plane (normal component exactly 0)."""
    n = n or _budget(case, 1500)
    t32 = case.tris32.astype(np.float64)
    k = rng.integers(0, len(t32), n)
    blo, bhi = t32[k].min(axis=1), t32[k].max(axis=1)
    o = rng.uniform(blo, bhi)
    kind, axis = rng.integers(0, 4, n), rng.integers(0, 3, n)
    rows = np.arange(n)
    side = rng.random(n) < 0.5
    vert = kind == 0
    o[vert] = t32[k[vert], rng.integers(0, 3, np.count_nonzero(vert))]
    face = np.where(side[:, None], blo, bhi)[rows, axis]
    o[kind == 1, axis[kind == 1]] = face[kind == 1]
    slo, shi = case.tris32.reshape(-1, 3).min(0).astype(np.float64), case.tris32.reshape(-1, 3).max(0).astype(np.float64)
    o[kind == 2, axis[kind == 2]] = np.where(side, slo[axis], shi[axis])[kind == 2]
    d = rng.normal(size=(n, 3))
    graze = (rng.random(n) < 0.5) & (kind >= 1)
    d[graze, axis[graze]] = 0.0
    return _rays(o.astype(np.float32), _unit(d))


def far_origins(case, rng, n=None):
    """Origins 1e6 to 1e7 away from the scene, aimed back at random points of its triangles."""
    n = n or _budget(case, 1500)
    target = case.tris64[rng.integers(0, len(case.tris64), n)].mean(axis=1)
    o = (case.centre + _unit(rng.normal(size=(n, 3))) * (10.0 ** rng.uniform(6, 7, (n, 1)))).astype(np.float32)
    return _rays(o, _unit(target - o.astype(np.float64)))


def ray_sets(case, seed=0):
    """{name: (org_tmin (n, 4) f32, dir_tmax (n, 4) f32)} of every set that needs no hit distance first."""
    rng = np.random.default_rng(seed)
    return {"pinhole": pinhole(case), "segments": segments(case, rng), "axis_parallel": axis_parallel(case, rng),
            "non_unit": non_unit(case, rng), "on_planes": on_planes(case, rng), "far_origins": far_origins(case, rng)}


def interval_edges(org, dirs, dist):
    """Rays whose brute-force hit distance is `dist` (f32, finite): the same ray with tmax in {d, next(d), FLT_MAX, +inf} (tmin 0),
    tmin in {d, prev(d), 0, -1} (tmax FLT_MAX), and tmin == tmax in {d, 0}."""
    d = np.asarray(dist, np.float32)
    up, down = np.nextafter(d, np.float32(np.inf)), np.nextafter(d, np.float32(-np.inf))
    z, big = np.zeros_like(d), np.full_like(d, FLT_MAX)
    variants = [(z, d), (z, up), (z, big), (z, np.full_like(d, np.inf)), (d, big), (down, big), (np.full_like(d, -1.0), big),
                (d, d), (z, z)]
    o_all, d_all = [], []
    for tmin, tmax in variants:
        o, dd = org.copy(), dirs.copy()
        o[:, 3], dd[:, 3] = tmin, tmax
        o_all.append(o)
        d_all.append(dd)
    return np.concatenate(o_all), np.concatenate(d_all)


def edge_rays(case, osc):
    """interval_edges of up to 400 pinhole rays that hit, at the oracle's brute-force distance."""
    org, dirs = pinhole(case)
    brute = osc.trace(2, org, dirs)
    hit = np.nonzero(brute["triIndex"] != api.GFX_INVALID_SLOT)[0][:400]
    return interval_edges(org[hit], dirs[hit], brute["dist"][hit])


def decidable(case, org, dirs, flat, dist):
    """Rays whose brute-force answer every conservative traversal returns: the misses, and the hits whose point org + dist dir lies in
    the box of the triangle hit, grown per axis by 2^-24 (|org_k| + max |box_k|) -- an eighth of the GPU traversal's widening, a
    sixteenth of the oracle's.  Elsewhere the fp32 triangle test is so ill-conditioned (a zero-area triangle, a ray from 1e7 away
    that grazes a tiny one) that it reports a "hit" outside the triangle and outside every box that holds it: a brute force takes
    it, a traversal that culls by box cannot, and which of two traversals does depends on its tree."""
    hit = flat >= 0
    ok = ~hit
    t = case.tris32[flat[hit]].astype(np.float64)
    lo, hi = t.min(axis=1), t.max(axis=1)
    o = org[hit, :3].astype(np.float64)
    p = o + dist[hit].astype(np.float64)[:, None] * dirs[hit, :3].astype(np.float64)
    grow = U32 * (np.abs(o) + np.maximum(np.abs(lo), np.abs(hi)))
    ok[hit] = np.all((p >= lo - grow) & (p <= hi + grow), axis=1)
    return ok


# ---------------------------------------------------------------------------------------------------------------- float64 reference
NOT_ROBUST, ROBUST_HIT, ROBUST_MISS = 0, 1, 2


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


class Reference:
    """Plain float64 ray-triangle brute force over all triangles, chunked; "robust" as in the module docstring."""

    def __init__(self, case):
        t = case.tris32.astype(np.float64)
        self.pA, self.eAB, self.eCA = t[:, 0], t[:, 1] - t[:, 0], t[:, 0] - t[:, 2]
        self.n = _cross(self.eCA, self.eAB)
        self.nlen = np.linalg.norm(self.n, axis=1)
        self.emax = np.linalg.norm(np.stack([self.eAB, self.eCA, t[:, 2] - t[:, 1]]), axis=2).max(axis=0)
        # dot(n, dir) as the fp32 test computes it: where it is exactly zero that test never reports a hit (t is NaN or inf)
        p = case.tris32
        e_ab, e_ca = p[:, 1] - p[:, 0], p[:, 0] - p[:, 2]
        self.n32 = np.stack([e_ca[:, 1] * e_ab[:, 2] - e_ca[:, 2] * e_ab[:, 1], e_ca[:, 2] * e_ab[:, 0] - e_ca[:, 0] * e_ab[:, 2],
                             e_ca[:, 0] * e_ab[:, 1] - e_ca[:, 1] * e_ab[:, 0]], axis=1).astype(np.float32)

    def classify(self, org, dirs):
        """-> (kind (n,) int8, tri (n,) flat index of the robust hit or -1, t (n,) float64, tol (n,) distance tolerance)"""
        n = len(org)
        out = (np.zeros(n, np.int8), np.full(n, -1, np.int64), np.full(n, np.nan), np.zeros(n))
        step = max(1, PAIR_CHUNK // max(1, len(self.pA)))
        for s in range(0, n, step):
            for dst, src in zip(out, self._chunk(org[s:s + step], dirs[s:s + step])):
                dst[s:s + step] = src
        return out

    def _chunk(self, org, dirs):
        o = org[:, None, :3].astype(np.float64)
        d = dirs[:, :3].astype(np.float64)
        tmin, tmax = org[:, 3:4].astype(np.float64), dirs[:, 3:4].astype(np.float64)
        d32 = dirs[:, :3]
        den32 = (self.n32[None, :, 0] * d32[:, None, 0] + self.n32[None, :, 1] * d32[:, None, 1]) + self.n32[None, :, 2] * d32[:, None, 2]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            w = self.pA[None] - o                                         # (rays, tris, 3)
            den = d @ self.n.T
            q = _cross(np.broadcast_to(d[:, None, :], w.shape), w)
            b = np.einsum("rmk,mk->rm", q, self.eCA) / den
            c = np.einsum("rmk,mk->rm", q, self.eAB) / den
            a = 1.0 - b - c
            t = np.einsum("rmk,mk->rm", w, self.n) / den
            # first-order fp32 error of the triangle test: the positions carry |pA - org| u (its first subtraction)
            pos_err = U32 * np.linalg.norm(w, axis=2)
            e_bc = ERR_K * (pos_err * self.emax[None] * np.linalg.norm(d, axis=1)[:, None] / np.abs(den) + U32)
            e_t = ERR_K * (pos_err * self.nlen[None] / np.abs(den) + U32 * np.abs(t))
            m_bc = np.maximum(BC_MARGIN, e_bc)
            m_t = np.maximum(T_MARGIN * np.abs(t), e_t)
            finite = np.isfinite(t) & np.isfinite(m_t) & np.isfinite(m_bc)
            cand = finite & (a > -m_bc) & (b > -m_bc) & (c > -m_bc) & (t > tmin - m_t) & (t < tmax + m_t) & (den32 != 0)
            uncertain = ~finite & (den32 != 0)          # parallel in float64, not in fp32: anything may come out
            rows = np.arange(len(org))
            tc = np.where(cand, t, np.inf)
            best = np.argmin(tc, axis=1)
            tb = tc[rows, best]
            found = np.isfinite(tb)
            mt_b = np.where(found, m_t[rows, best], 0.0)
            inside = (np.minimum(np.minimum(a, b), c)[rows, best] > m_bc[rows, best]) & (tb > tmin[:, 0] + mt_b) & (tb < tmax[:, 0] - mt_b)
            others = np.where(cand, t - np.maximum(m_t, mt_b[:, None]), np.inf)
            others[rows, best] = np.inf
            separated = others.min(axis=1) > tb
        clean = ~uncertain.any(axis=1)
        kind = np.where(clean & ~found, ROBUST_MISS, np.where(clean & found & inside & separated, ROBUST_HIT, NOT_ROBUST)).astype(np.int8)
        return kind, np.where(kind == ROBUST_HIT, best, -1), np.where(kind == ROBUST_HIT, tb, np.nan), mt_b


def check_against_reference(ref, flat_hit, dist, what):
    """flat_hit: flat triangle index of each ray's answer (-1 = miss); dist: its distance.  Every robust ray must agree with the
    float64 reference.  Returns (robust hits, robust misses) checked."""
    kind, tri, t, tol = ref
    h = kind == ROBUST_HIT
    wrong = h & (flat_hit != tri)
    assert not wrong.any(), (f"{what}: {np.count_nonzero(wrong)} of {np.count_nonzero(h)} robust hits return another triangle; "
                             f"first: ray {np.nonzero(wrong)[0][0]}, triangle {flat_hit[wrong][0]} instead of {tri[wrong][0]}")
    far = h & ~(np.abs(dist.astype(np.float64) - t) <= tol)
    assert not far.any(), f"{what}: {np.count_nonzero(far)} robust hits at the wrong distance; first {dist[far][0]!r} vs {t[far][0]!r}"
    miss = kind == ROBUST_MISS
    bad = miss & (flat_hit >= 0)
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} of {np.count_nonzero(miss)} robust misses report a hit; first ray {np.nonzero(bad)[0][0]}"
    return int(np.count_nonzero(h)), int(np.count_nonzero(miss))
