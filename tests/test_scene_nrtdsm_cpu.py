"""CPU: NRTDSM objects as instances of a scene beside TFDM ones, on the host -- the host compilation of
csrc/nrtdsm/nrtdsm_instance.hip.h (tests/scene_nrtdsm_host.cpp) around the host cores (tests/nrtdsm_host.cpp, tests/tfdm_host.cpp).

  * geometry, independent of the core: one NRTDSM instance (the curved cap; the quad under a 32 x 32 procedural map) under transforms
    whose linear part is exact in float (a signed axis permutation times power-of-two scales: uniform, non-uniform, mirrored), against
    the float64 model of the surface (tests/nrtdsm_ref.py), asked in OBJECT space: the float world rays go there through the exact
    float64 inverse, t stays what it is (the direction is not renormalised), the model's normal comes back through the float64 normal
    matrix;
  * the merge rule across kinds: TFDM quad, NRTDSM cap, TFDM quad rotated, the same NRTDSM cap again -- the walk equals the chain of
    single-instance host traces in index order with tmax = the best so far, bit for bit, and the surface both caps share reports the
    lower index;
  * the world-box cull changes nothing, on those rays and on 500 rays per NRTDSM instance along its unpadded world box.

Distance tolerance: that of tests/test_nrtdsm_cpu.py, 8 * E_mesh * max(1, t) + 2 * 1e-5 * s / |cos theta|, with E_mesh
measured in this run as there, theta and |d| taken in object space, where the solver works (t is the same number in both spaces).
The keep rule and its 2 % cap are those of that file, asserted on the model alone before anything is compared.

Normal tolerance: in object space the angle that file derives, tol |d| / w + 1e-5 rad (w: the object size of a texel).  The normal
matrix inv(L)^T of an instance is linear, and a linear map turns the angle between two nearby directions by at most its condition
number kappa (largest over smallest scale of L: 1 for the uniform transform, 8 for the other two), so the world-space angle is held
to kappa times that; plus 1e-6 rad for normal_to_world's own float arithmetic (three products, two sums, one normalisation).

Measured (printed by the tests, recorded in DESIGN.md section 22)."""
import numpy as np
import pytest

from gfxexp_amd import api
from tests import nrtdsm_host as NH
from tests import nrtdsm_ref as NR
from tests import scene_nrtdsm_host as M
from tests import scene_trace_host as S
from tests import tfdm_host as T
from tests import util
from tests.test_nrtdsm_cpu import kept, tolerance, unit
from tests.test_scene_trace_cpu import EXACT
from tests.test_tfdm_cpu import e_mesh      # noqa: F401 -- the fixture, measured exactly as there

INVALID = api.GFX_INVALID_SLOT
N_RAYS = 4000


@pytest.fixture(scope="module")
def nhost(built_lib, tmp_path_factory):
    return NH.Host(tmp_path_factory.mktemp("nrtdsm_host"))


@pytest.fixture(scope="module")
def mhost(built_lib, tmp_path_factory):
    return M.MixedHost(tmp_path_factory.mktemp("scene_nrtdsm_host"))


OBJECTS = {
    "cap": lambda: NH.cap_mesh() + (T.two_sine_map(64), api.tfdm_params(h_scale=0.05)),
    "quad": lambda: T.quad_mesh() + (M.small_map(32), api.tfdm_params(h_scale=0.1)),
}
_MODEL = {}


def model_of(nhost, obj):
    """Per object, computed once: the host state, the model, the object-space rays and the model's closest hits on them."""
    if obj not in _MODEL:
        v, t, heights, gp = OBJECTS[obj]()
        o, d = T.mesh_rays(v, N_RAYS, 5) if obj == "cap" else T.cap_rays(N_RAYS)
        _MODEL[obj] = dict(v=v, t=t, st=nhost.state(v, t, heights, gp), S=NR.Surface(v, t, T.mips32(heights)[0], gp), o=o, d=d)
    return _MODEL[obj]


# ---------------------------------------------------------------- geometry, independent of the core
@pytest.mark.parametrize("name", sorted(EXACT))
@pytest.mark.parametrize("obj", sorted(OBJECTS))
def test_nrtdsm_instance_under_exact_transforms(nhost, mhost, e_mesh, obj, name):
    c = model_of(nhost, obj)
    Sf = c["S"]
    L, tr = EXACT[name]
    L, tr = np.asarray(L, np.float64), np.asarray(tr, np.float64)
    m = S.affine(L, tr)
    assert np.array_equal(m.astype(np.float64)[:, :3], L) and abs(np.linalg.det(L)) > 0
    if name == "mirrored":
        assert np.linalg.det(L) < 0
    # float world rays: the images of the object-space rays, rounded to float once; the model's rays: those floats through the
    # exact float64 inverse (a signed permutation times powers of two, and a dyadic translation: exact in float64)
    org, dirs = T.pack_rays(c["o"][:, :3].astype(np.float64) @ L.T + tr, c["d"][:, :3].astype(np.float64) @ L.T)
    Li = np.linalg.inv(L)
    assert np.array_equal(Li @ L, np.eye(3))
    o64, d64 = (org[:, :3].astype(np.float64) - tr) @ Li.T, dirs[:, :3].astype(np.float64) @ Li.T
    mo = Sf.trace(o64, d64, org[:, 3], dirs[:, 3], k=1)
    keep = kept(mo, "%s / %s" % (obj, name))
    want = np.isfinite(mo["t"])
    assert 0.2 < want[keep].mean() < 0.98
    # the scene query on the host: no plain geometry, one NRTDSM instance
    rec = mhost.instance_of_state(M.NRTDSM, c["st"], m)
    assert rec["pad0"][0] == M.NRTDSM
    hits = mhost.trace(rec, None, api.TRACE_CLOSEST, org, dirs)
    got = hits["where"] != INVALID
    bad = keep & (got != want)
    assert not bad.any(), "%s / %s: hit / miss differs on %d kept rays, first %d" % (obj, name, bad.sum(), np.nonzero(bad)[0][0])
    both = keep & want
    bad = both & (hits["index"] != mo["prim"])
    assert not bad.any(), "%s / %s: the primitive differs on %d rays, first %d" % (obj, name, bad.sum(), np.nonzero(bad)[0][0])
    nm = Sf.normal(mo["prim"][both], mo["alpha"][both], mo["beta"][both])
    dlb = np.linalg.norm(d64[both], axis=1)
    cos = (unit(d64[both]) * nm).sum(1)
    tolb = tolerance(c, e_mesh, mo["t"][both], cos, dlb)
    err = np.abs(hits["dist"][both].astype(np.float64) - mo["t"][both])
    print("%s / %s: |t - t64| worst %.3e, worst ratio to the bound %.3f over %d rays" % (obj, name, err.max(), (err / tolb).max(), both.sum()))
    assert (err / tolb).max() <= 1, "%s / %s: ray %d is off by %.3e, bound %.3e" % (obj, name, np.nonzero(both)[0][(err / tolb).argmax()], err[(err / tolb).argmax()],
                                                                                    tolb[(err / tolb).argmax()])
    assert np.all(hits["where"][got] >> 1 == 0) and np.all(hits["dist"][~got] == dirs[~got, 3]) and np.all(hits["index"][~got] == INVALID)
    # the normal: unit, within the angle the bound implies of the model's normal brought to world space by the float64 normal matrix
    n32 = hits["normal"][both].astype(np.float64)
    assert np.all(np.abs(np.linalg.norm(n32, axis=1) - 1) < 1e-5)
    nw = unit(nm @ Li)                                             # rows: inv(L)^T nm
    p, tc = Sf.p[mo["prim"][both]], Sf.tc[mo["prim"][both]]
    w = np.sqrt(np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1) / (np.abs(T._cross2(tc[:, 1] - tc[:, 0], tc[:, 2] - tc[:, 0])) * Sf.res ** 2))
    sv = np.linalg.svd(L, compute_uv=False)
    kappa = sv.max() / sv.min()
    angle = np.arctan2(np.linalg.norm(np.cross(n32, nw), axis=1), (n32 * nw).sum(1))
    atol = kappa * (tolb * dlb / w + 1e-5) + 1e-6
    print("%s / %s: normal off by at most %.3e rad, worst ratio to its bound %.3f (kappa = %g)" % (obj, name, angle.max(), (angle / atol).max(), kappa))
    assert (angle / atol).max() <= 1
    # frontFace is the side of the WORLD normal the world ray comes from, the mirrored instance too
    side = (unit(dirs[both, :3].astype(np.float64)) * nw).sum(1)
    sure = np.abs(side) > 1e-4
    assert sure.mean() > 0.99 and np.array_equal((hits["where"][both][sure] & 1) == 1, side[sure] < 0)
    # any-hit: 1 exactly where the closest-hit query finds something
    assert np.array_equal(mhost.trace(rec, None, api.TRACE_ANY, org, dirs) == 1, got)


# ---------------------------------------------------------------- the merge rule across kinds
@pytest.fixture(scope="module")
def merge_scene(built_lib, nhost, mhost):
    """TFDM quad (0), NRTDSM cap (1), TFDM quad rotated (2), the NRTDSM cap of member 1 again under the same transform (3)."""
    qv, qt = T.quad_mesh()
    quad = nhost.T.state(qv, qt, T.two_sine_map(64), api.tfdm_params(h_scale=0.1))
    cv, ct = NH.cap_mesh()
    cap = nhost.state(cv, ct, T.two_sine_map(64), api.tfdm_params(h_scale=0.05))
    cap_m = S.affine(S.rotation((1.0, 0.3, 0.0), 25.0) @ np.diag([0.8, 0.8, 0.5]), (0.5, 0.6, -0.42))
    members = [(M.TFDM, quad, S.affine(np.eye(3), (0, 0, 0))), (M.NRTDSM, cap, cap_m),
               (M.TFDM, quad, S.affine(S.rotation((0.2, 1.0, 0.1), 30.0), (0.1, 0.1, 0.3))), (M.NRTDSM, cap, cap_m)]
    table = np.concatenate([mhost.instance_of_state(k, st, m, 100 + i) for i, (k, st, m) in enumerate(members)])
    unpadded = [S.image_of_box(m, st["nodes"][0]["lo"], st["nodes"][0]["hi"]) for _, st, m in members]
    org, dirs = S.chain_rays(unpadded)
    # a synthetic plain phase: a plain triangle hit on a third of the rays, somewhere along the scene's depth
    rng = np.random.default_rng(77)
    plain = np.zeros(len(org), api.HIT_DTYPE)
    plain["triIndex"] = INVALID
    plain["dist"] = dirs[:, 3]
    some = rng.uniform(size=len(org)) < 0.33
    plain["dist"][some], plain["bcB"][some], plain["bcC"][some] = rng.uniform(2.0, 3.5, some.sum()), 0.25, 0.5
    plain["triIndex"][some] = rng.integers(0, 1000, some.sum())
    return members, table, unpadded, org, dirs, plain


def test_merge_rule_across_kinds(nhost, mhost, merge_scene):
    members, table, _, org, dirs, plain = merge_scene
    assert list(table["pad0"]) == [0, 1, 0, 1]
    shost_rec = [table[k:k + 1] for k in range(len(table))]
    # the walk ...
    walk, cw = mhost.trace(table, plain, api.TRACE_CLOSEST, org, dirs, counters=True)
    # ... and the chain of single-instance host traces in index order, tmax = the best so far, the plain hit first
    best = mhost.trace(table[:0], plain, api.TRACE_CLOSEST, org, dirs)
    for k, rec in enumerate(shost_rec):
        d = dirs.copy()
        d[:, 3] = best["dist"]
        one = mhost.trace(rec, None, api.TRACE_CLOSEST, org, d)
        win = one["where"] != INVALID
        assert np.all(one["where"][win] >> 1 == 0)
        for f in ("dist", "bcB", "bcC", "index", "normal"):
            best[f][win] = one[f][win]
        best["where"][win] = (np.uint32(k) << np.uint32(1)) | (one["where"][win] & np.uint32(1))
    for f in api.SCENE_HIT_DTYPE.names:
        util.assert_same_bits("the walk against the chain of single-instance traces, field %s" % f, walk[f], best[f])
    where = walk["where"]
    disp = (where != INVALID) & (where != api.SCENE_PLAIN)
    shares = [np.mean(where == api.SCENE_PLAIN)] + [np.mean(disp & (where >> 1 == k)) for k in range(4)]
    print("closest hits: plain %.1f %%, members %s %%, miss %.1f %%" % (100 * shares[0], ["%.1f" % (100 * s) for s in shares[1:]], 100 * np.mean(where == INVALID)))
    # every hit on the surface members 1 and 3 share reports index 1; the others are all seen
    assert shares[4] == 0 and all(s > 0.02 for s in shares[:4]), shares
    # ... and it is the same answer a table without the second copy gives
    three = mhost.trace(table[:3], plain, api.TRACE_CLOSEST, org, dirs)
    for f in api.SCENE_HIT_DTYPE.names:
        util.assert_same_bits("with and without the second copy, field %s" % f, walk[f], three[f])
    # a plain hit at exactly an NRTDSM distance stays
    alone = mhost.trace(table[1:2], None, api.TRACE_CLOSEST, org, dirs)
    hit = alone["where"] != INVALID
    tie = np.zeros(len(org), api.HIT_DTYPE)
    tie["dist"], tie["bcB"], tie["bcC"], tie["triIndex"] = alone["dist"], 0.25, 0.5, np.where(hit, 7, INVALID)
    tied = mhost.trace(table[1:2], tie, api.TRACE_CLOSEST, org, dirs)
    assert hit.mean() > 0.05 and np.all(tied["where"][hit] == api.SCENE_PLAIN) and np.all(tied["index"][hit] == 7) and np.all(tied["where"][~hit] == INVALID)
    # any-hit: occluded exactly where the plain phase said so or a member is hit inside the ray's interval
    occ_plain = (plain["triIndex"] != INVALID).astype(np.uint32)
    occ = mhost.trace(table, occ_plain, api.TRACE_ANY, org, dirs)
    none = mhost.trace(table, None, api.TRACE_CLOSEST, org, dirs)
    assert np.array_equal(occ == 1, (occ_plain == 1) | (none["where"] != INVALID))
    assert cw[2] == len(org) and 0 < cw[5] <= cw[4] <= 4 * len(org) and cw[3] >= cw[5]


def test_world_box_cull_changes_nothing(mhost, merge_scene):
    members, table, unpadded, org, dirs, plain = merge_scene
    extra = [S.box_rays(lo, hi, 500, seed=60 + k) for k, (lo, hi) in enumerate(unpadded) if members[k][0] == M.NRTDSM]
    assert len(extra) == 2
    org = np.concatenate([org] + [e[0] for e in extra])
    dirs = np.concatenate([dirs] + [e[1] for e in extra])
    pl = np.concatenate([plain, np.full(1000, plain[plain["triIndex"] == INVALID][0])])
    pl["dist"][-1000:] = dirs[-1000:, 3]
    for mode in (api.TRACE_CLOSEST, api.TRACE_ANY):
        p = pl if mode == api.TRACE_CLOSEST else (pl["triIndex"] != INVALID).astype(np.uint32)
        culled, c1 = mhost.trace(table, p, mode, org, dirs, cull=True, counters=True)
        full, c0 = mhost.trace(table, p, mode, org, dirs, cull=False, counters=True)
        if mode == api.TRACE_CLOSEST:
            for f in api.SCENE_HIT_DTYPE.names:
                util.assert_same_bits("closest, field %s, with and without the world-box cull" % f, culled[f], full[f])
        else:
            assert np.array_equal(culled, full)
        print("mode %d: %d world-box tests, %d traversals with the cull, %d without" % (mode, c1[4], c1[5], c0[5]))
        assert c1[4] == c0[4] and c1[5] < c0[5] and c0[5] == c0[4] and c1[2] == len(org)
