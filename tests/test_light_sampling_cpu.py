"""CPU: the oracle's emitter distributions and light sampler (oracle/orc_scene.h, the twin of gfxexp_amd/csrc/lights.hip and the
sampling half of shading.hip.h) against the definition stated independently in float64 (tests/light_ref.py), on the scenes of
tests/light_scenes.py.  Two steps: (a) the tables against the definition, (b) the selection against the tables, then (c) the
sample against the record it was drawn on.  tests/test_gpu_light_sampling.py puts the kernels bit for bit on the oracle, which
places them under the same definition.

Tolerances that are not derived are measured: the oracle's worst error against light_ref over the scenes of this file, as printed
by the tests (run with -s), times four (the fp32 cross / length / luminance chain takes about ten roundings; four leaves room
for another scene's values).  Measured on an x86-64 host with the parity build of the oracle (-O2 -ffp-contract=off):

    weights, all three levels, relative          MEASURED_WEIGHT_REL  = 5.1e-7   (worst: pathological 5.03e-7; level3 2.4e-7, transforms 2.1e-7,
                                                 small_street 2.0e-7, textured 1.6e-7, instance-count scenes 5.9e-8, bunny 2.8e-8)
    density * area against the table product     MEASURED_DENSITY_REL per scene, below (the world-space area of a small emitter far
                                                 from the origin, or of a sliver, loses digits to cancellation: level3, the street
                                                 and the pathological scene are orders of magnitude above the others, so one
                                                 number for all would test the others with their slack)
"""
import numpy as np
import pytest

from tests import light_scenes as LS, util

F = np.float32
EPS = 2.0 ** -24

MEASURED_WEIGHT_REL = 5.1e-7
MEASURED_DENSITY_REL = {"level3": 2.0e-5, "transforms": 5.9e-7, "textured": 1.3e-6, "bunny": 4.8e-7, "small_street": 6.3e-6, "pathological": 2.5e-5}
MEASURED_DENSITY_REL.update({f"count_{n}": 5.6e-8 for n in LS.INSTANCE_COUNTS})      # worst of the eight (count_4096)
TOL_FACTOR = 4.0


case = LS.case
ALL = list(LS.SCENES)


# ---------------------------------------------------------------- (a) tables against the definition
def _check_distribution(what, t, want64, worst):
    w, cdf, integral = t
    n = len(w)
    assert n == len(want64), what
    zero = want64 == 0
    assert np.all(w[zero] == 0), f"{what}: a zero-weight entry is not exactly 0"
    if np.any(~zero):
        worst[0] = max(worst[0], float(np.max(np.abs(w[~zero].astype(np.float64) - want64[~zero]) / want64[~zero])))
    # the serial float32 prefix sum, first entry 0
    serial = np.concatenate([[F(0)], np.cumsum(w, dtype=F)[:-1]]).astype(F)
    util.assert_same_bits(what + " cdf", cdf, serial)
    assert F(integral) == F(cdf[n - 1] + w[n - 1]), what
    # against the exact sums of the same float32 weights: every one of the at most n additions rounds the running sum once, by at
    # most half an ulp of a value that never exceeds the total, i.e. by at most 2^-24 * total
    exact = np.concatenate([[0.0], np.cumsum(w.astype(np.float64))])
    assert np.all(np.abs(cdf.astype(np.float64) - exact[:-1]) <= n * EPS * exact[-1]), what
    assert abs(np.float64(F(integral)) - exact[-1]) <= n * EPS * exact[-1], what


@pytest.mark.parametrize("name", ALL)
def test_tables_follow_the_definition(oracle_lib, name):
    c = case(name)
    worst = [0.0]
    for g, t in c.l2.items():
        _check_distribution(f"{name} geometry {g}", t, c.ref.tri_w[g], worst)
    assert set(c.l1) == set(c.ref.inst_geom_w)
    for g, t in c.l1_by_group.items():
        ii = int(c.layout.emitter_insts[np.nonzero(c.layout.inst_group[c.layout.emitter_insts] == g)[0][0]])
        _check_distribution(f"{name} instance {ii}", t, c.ref.inst_geom_w[ii], worst)
    _check_distribution(f"{name} instances", c.l0, c.ref.inst_w, worst)
    print(f"\n[measured] {name}: worst relative weight error against the float64 definition {worst[0]:.3e}")
    assert worst[0] <= TOL_FACTOR * MEASURED_WEIGHT_REL


# ---------------------------------------------------------------- (b) selection against the tables
@pytest.mark.parametrize("name", ALL)
def test_selection_follows_the_tables(oracle_lib, name):
    """The share of the stratified sweep that picks record e against P_e = the product of the three table shares.  A stratum is
    misassigned only if its ul lies within delta of an end of e's interval, so the share is off by at most 2 / N (the two strata
    the ends cut) + 2 * delta.  delta in units of ul, each rounding being at most 2^-24 relative:
      level 1  ul * I1: one rounding of a value <= I1, i.e. <= 2^-24 of the ul range                                   1
      remap    u' = (u - lo) / (hi - lo): three roundings, each relative to u' <= 1, which spans p1 of the ul range    3 p1
               (u - 0 and I - 0 are exact in a one-entry level: then only the division rounds                          1 p1)
      level 2  u' * I2                                                                                                  1 p1
      remap and level 3 likewise, spanning p1 p2                                                                (3 or 1 + 1) p1 p2
    so c = 2 * (1 + (r1 + 1) p1 + (r2 + 1) p1 p2), r = 1 for a one-entry level, else 3: at most 18, and below 16 unless one instance
    holds most of the scene's power in a level of several entries -- which none of these scenes has (asserted)."""
    c = case(name)
    lay = c.layout
    early = c.rec == LS.NONE
    assert int(c.counts.sum()) + int(np.count_nonzero(early)) == c.n
    assert np.all(c.sweep_pd[early] == 0)
    s0, s1, s2 = c.share
    p_e = s0 * s1 * s2
    r1 = np.where(c.entries[0] == 1, 1.0, 3.0)
    r2 = np.where(c.entries[1] == 1, 1.0, 3.0)
    cc = 2.0 * (1.0 + (r1 + 1.0) * s0 + (r2 + 1.0) * s0 * s1)
    assert cc.max() < 16.0
    diff = np.abs(c.counts / c.n - p_e)
    bound = 2.0 / c.n + cc * EPS
    worst = int(np.argmax(diff - bound))
    print(f"\n[measured] {name}: worst share difference {diff.max():.3e} (bound there {bound[np.argmax(diff)]:.3e}), early outs {np.count_nonzero(early)}")
    assert np.all(diff <= bound), f"record {worst} {c.ids[worst]}: share {c.counts[worst] / c.n} against {p_e[worst]}"
    # exactly on an entry of the instance-level CDF the search takes the entry that begins there (<=, not <)
    ul, expect = LS.tie_ul(c.l0)
    if len(ul):
        tie = np.full((len(ul), 3), 0.5, F)
        tie[:, 0] = ul
        _, tie_pd, tie_ids = c.osc.sample_light_ids((0, 0, 0), tie)
        lit = c.l0[0][expect] > 0
        assert np.array_equal(tie_ids[lit, 0], expect[lit].astype(np.uint32)), name
        assert np.all(tie_ids[~lit] == LS.NONE) and np.all(tie_pd[~lit] == 0), name
        print(f"[measured] {name}: {len(ul)} selection numbers exactly on an instance boundary")
    # behind a zero-probability instance or geometry instance: never
    behind = (c.prob[0] == 0) | (c.prob[1] == 0)
    assert np.all(c.counts[behind] == 0)
    assert np.all(c.sweep_pd[~early] > 0)


# ---------------------------------------------------------------- (c) the sample on the record
def _low_distortion_map(u0, u1):
    """Heitz, A Low-Distortion Map Between Triangle and Square, in float64: barycentric coordinates of (A, B, C)."""
    a, b = 0.5 * u0, 0.5 * u1
    off = b - a
    b = np.where(off > 0, b + off, b)
    a = np.where(off > 0, a, a - off)
    return np.stack([a, b, 1.0 - a - b], -1)


def _barycentrics(tri, p):
    """float64 barycentric coordinates of p (n, m, 3) in tri (n, 3, 3) and the distance from the plane."""
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    nrm = np.cross(e1, e2)
    nn = np.einsum("ij,ij->i", nrm, nrm)
    d = p - tri[:, None, 0]
    b = np.einsum("nmj,nj->nm", np.cross(d, e2[:, None]), nrm) / nn[:, None]
    cc = np.einsum("nmj,nj->nm", np.cross(e1[:, None], d), nrm) / nn[:, None]
    dist = np.einsum("nmj,nj->nm", d, nrm) / np.sqrt(nn)[:, None]
    return np.stack([1 - b - cc, b, cc], -1), dist


def _subset(c):
    extra = (LS.MIRRORED_INSTANCE,) if c.name == "transforms" else ()
    return LS.choose_records(c.layout, c.rec, c.counts, seed=31, extra=extra)


@pytest.mark.parametrize("name", ALL)
def test_samples_lie_on_their_records(oracle_lib, name):
    c = case(name)
    want, ul = _subset(c)
    ids, tris, nrm, nmat, area = c.ref.records()
    assert np.array_equal(ids, c.ids)                                     # the definition enumerates the records in the layout's order
    # zero-area records have no density to speak of: never picked, left out, counted
    zero = np.nonzero(area == 0)[0][:4]
    assert np.all(c.counts[zero] == 0)
    left_out = len(zero)
    total = len(want) + left_out
    assert left_out <= 0.02 * total or total < 50, (left_out, total)
    g = LS.grid_u01()
    u = np.concatenate([np.repeat(ul, 64)[:, None], np.tile(g, (len(want), 1))], 1).astype(F)
    ls, pd, pick = c.osc.sample_light_ids((0, 0, 0), u)
    assert np.array_equal(c.layout.record_of(pick).reshape(-1, 64), np.repeat(want[:, None], 64, 1))
    tri, pos = tris[want], ls[:, 3:6].astype(np.float64).reshape(-1, 64, 3)
    extent = np.max(np.linalg.norm(tri - np.roll(tri, 1, axis=1), axis=2), axis=1)
    # fp32: three rounded products and two sums per world vertex, the same again for the blend -- 16 half-ulps of the largest coordinate
    tol = 16 * EPS * np.maximum(np.abs(tri).max(axis=(1, 2)), extent)
    bc, dist = _barycentrics(tri, pos)
    assert np.all(bc >= -(tol / extent)[:, None, None]), name
    assert np.all(np.abs(dist) <= tol[:, None]), name
    assert np.all(np.linalg.norm(pos.mean(axis=1) - tri.mean(axis=1), axis=1) <= extent / 8), name
    # normal: unit, and the normal matrix times the interpolated vertex normal
    nr = ls[:, 6:9].astype(np.float64).reshape(-1, 64, 3)
    assert np.all(np.abs(np.linalg.norm(nr, axis=2) - 1) <= 8 * EPS)
    w = _low_distortion_map(g[:, 0].astype(np.float64), g[:, 1].astype(np.float64))          # (64, 3)
    interp = np.einsum("mk,nkj->nmj", w, nrm[want])
    side = np.einsum("nij,nmj->nmi", nmat[want], interp)
    side /= np.linalg.norm(side, axis=2, keepdims=True)
    assert np.all(np.einsum("nmj,nmj->nm", nr, side) >= 1 - 1e-5), name
    assert np.all(ls[:, 9] == 0)
    # density * area = the table probability
    p0, p1, p2 = c.prob
    table = (p0 * p1 * p2)[want]
    got = pd.astype(np.float64).reshape(-1, 64) * area[want][:, None]
    rel = np.abs(got - table[:, None]) / table[:, None]
    print(f"\n[measured] {name}: worst relative error of density * area against the table product {rel.max():.3e} ({len(want)} records, {left_out} zero-area left out)")
    assert rel.max() <= TOL_FACTOR * MEASURED_DENSITY_REL[name]
    # emittance: the material's constant, or within the texture's range
    assert np.all(np.isfinite(ls)) and np.all(ls[:, :3] >= 0)


SOLID_ANGLE_SCENES = ["transforms", "textured", "level3", "count_2"]


@pytest.mark.parametrize("name", SOLID_ANGLE_SCENES)
def test_solid_angle_samples(oracle_lib, name):
    """sampleLight<true> from a point close to an emitter, one far from it and one in its plane."""
    c = case(name)
    want, ul = _subset(c)
    _, tris, _, _, area = c.ref.records()
    pick = int(np.argmax(area[want]))
    rec, tri = int(want[pick]), tris[want[pick]]
    e1, e2 = tri[1] - tri[0], tri[2] - tri[0]
    gn = np.cross(e1, e2)
    gn /= np.linalg.norm(gn)
    extent = max(np.linalg.norm(e1), np.linalg.norm(e2), np.linalg.norm(tri[2] - tri[1]))
    centre = tri.mean(axis=0)
    g = LS.grid_u01()
    u = np.concatenate([np.full((64, 1), ul[pick], F), g], 1)
    for what, sp in (("close", centre + 0.05 * extent * gn), ("far", centre + 20.0 * extent * gn)):
        sp = sp.astype(F)
        ls, pd, ids = c.osc.sample_light_ids(sp, u, solid_angle=True)
        assert np.all(c.layout.record_of(ids) == rec)
        assert np.all(np.isfinite(ls)) and np.all(np.isfinite(pd)) and np.all(pd > 0), (name, what)
        d = ls[:, 3:6].astype(np.float64) - sp.astype(np.float64)
        far = np.linalg.norm(d, axis=1, keepdims=True)
        d /= far
        corners = tri - sp.astype(np.float64)
        corners /= np.linalg.norm(corners, axis=1, keepdims=True)
        edges = np.stack([np.cross(corners[k], corners[(k + 1) % 3]) for k in range(3)])
        edges *= np.sign(np.dot(corners[2], edges[0]))
        # the sine of the angle between the direction and each edge's plane, allowed to be short by the angle the position's own
        # rounding subtends (16 half-ulps of the largest coordinate, as above) plus 4e-7 for the fp32 unit vectors
        # ... and by what the fp32 excess alpha + beta + gamma - pi does to a small spherical triangle: three arc cosines of up to
        # pi, each good to about two ulps, against an area that shrinks with the square of the distance (Van Oosterom-Strackee in
        # float64) -- a relative error of the area moves a sample by that share of the triangle's angular size
        solid = 2 * abs(np.arctan2(np.dot(corners[0], np.cross(corners[1], corners[2])),
                                   1 + corners[0] @ corners[1] + corners[1] @ corners[2] + corners[2] @ corners[0]))
        angle = 16 * EPS * max(np.abs(tri).max(), np.abs(sp).max()) / far + 4e-7 + (8 * EPS * np.pi / solid) * np.linalg.norm(edges, axis=1).max()
        sines = (d @ edges.T) / np.linalg.norm(edges, axis=1)
        print(f"\n[measured] {name} {what}: least sine of a direction against an edge plane {sines.min():.3e}, allowed {-angle.max():.3e}")
        assert np.all(sines >= -angle), (name, what)
        bc, dist = _barycentrics(tri[None], ls[None, :, 3:6].astype(np.float64))
        assert np.all(bc >= -1e-3) and np.all(np.abs(dist) <= 1e-4 * max(extent, np.abs(tri).max()))
    if name == "count_2":
        # in the emitter's plane, all coordinates exact: the spherical triangle has no area, the density is 0 and nothing is NaN
        sp = np.array([tri[:, 0].max() + 2.0, tri[0, 1], tri[:, 2].max() + 1.0], F)
        assert F(tri[0, 1]) == tri[0, 1] == tri[1, 1] == tri[2, 1]
        ls, pd, ids = c.osc.sample_light_ids(sp, u, solid_angle=True)
        assert np.all(pd == 0)
        assert not np.any(np.isnan(ls)), ls[:4]


def test_a_scene_of_zero_weight_emitters_yields_density_zero(oracle_lib):
    hs = LS.zero_weight_scene()
    osc = util.feed_oracle(hs)
    assert osc.lights_read(0)[2] == 0
    u = np.full((64, 3), 0.5, F)
    u[:, 0] = LS.sweep_ul(64)
    for solid in (False, True):
        ls, pd, ids = osc.sample_light_ids((0.3, 1.0, 0.3), u, solid_angle=solid)
        assert np.all(pd == 0) and np.all(ids == LS.NONE) and np.all(ls == 0)


def test_sample_light_and_its_sibling_agree(oracle_lib):
    c = case("textured")
    u = np.random.default_rng(3).random((500, 3)).astype(F)
    ls, pd = c.osc.sample_light((0, 0, 0), u)
    ls2, pd2, _ = c.osc.sample_light_ids((0, 0, 0), u)
    util.assert_same_bits("sample", ls, ls2)
    util.assert_same_bits("density", pd, pd2)

