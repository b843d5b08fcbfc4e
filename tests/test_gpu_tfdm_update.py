"""-m gpu: gfx_tfdm_update_heights / gfx_nrtdsm_update_heights, a height map changed in place with a tree refit on the device.

After an update the object is compared with a fresh object created with the whole new map and the same parameters: every level
of heights and pyramid, the per-triangle boxes and the records are the same bits; the tree keeps its shape, every leaf is its
primitive's box and every inner box the exact union of its children's; closest hits and any-hit words equal the fresh object's in
every field, and equal the host core's on the nodes read back from the device with the host-made levels and pyramid of the new
map.  Nothing here has a tolerance.

The rays are those of tests/test_gpu_tfdm.py (20 000 + the special ones) and, per rectangle, up to 300 more that are aimed at it:
down the interpolated normal onto points of the base mesh whose texture coordinate lies inside the rectangle (_targeted_rays, float64,
from the mesh alone).  "The hit distances changed" is asserted wherever at least MIN_AIMED such rays exist.  Where no base triangle's footprint
reaches the rectangle grown by a texel (exact overlap test; the teapot's texture coordinates leave the map's first texel free), an
update changes no point of the surface: there the test asserts the opposite, that no hit changed in any bit.  In between (the bunny
and the teapot touch the corner texels with slivers that no ray finds) neither holds by reasoning, and what guards against a
no-op is that the heights read back changed and equal the fresh object's.

The comparison of the closest hits with a fresh object's is a comparison between two trees over the same boxes: it holds because the
walk of tfdm_core.hip.h counts a hit only from its leaf's box entry (less a per-ray slack) on.  Before that rule one of the 21 371 rays
of teapot-0x0x64x64 found primitive 8480 at t = 1.340186 through the refitted tree and primitive 8477 at t = 1.3380991 through the fresh
one, both hits in front of their primitives' boxes."""
import functools

import numpy as np
import pytest

from gfxexp_amd import api
from tests import nrtdsm_host as NH
from tests import tfdm_host as T
from tests import tfdm_update_host as U
from tests import util
from tests.test_gpu_tfdm import CASES as TFDM_CASES, _rays, gpu_tfdm_trace

pytestmark = pytest.mark.gpu
SIZE = 64
MIN_AIMED = 20        # aimed rays a "the hits changed" assertion rests on; fewer (a sliver of a footprint in the rectangle) prove nothing either way
RECTS = [(0, 0, 1, 1), (63, 63, 1, 1), (5, 9, 17, 3), (0, 20, 64, 1), (0, 0, 63, 64), (0, 0, 64, 64)]
CASES = {k: dict(TFDM_CASES[k], kind="tfdm") for k in ("quad", "quad_box", "quad_level2", "quad_wrapped_rotated", "bunny", "teapot")}
CASES["quad_bilinear"] = dict(mesh="quad", gp=dict(h_scale=0.1, local_intersection=api.TFDM_BILINEAR), kind="tfdm")
CASES["nrtdsm_quad"] = dict(mesh="quad", gp=dict(h_scale=0.1), kind="nrtdsm")
CASES["nrtdsm_teapot"] = dict(mesh="teapot.obj", gp=dict(h_scale=0.01), relative=True, kind="nrtdsm")


@pytest.fixture(scope="module")
def hosts(built_lib, tmp_path_factory):
    d = tmp_path_factory.mktemp("tfdm_update_gpu")
    nh = NH.Host(d)
    return {"tfdm": nh.T, "nrtdsm": nh}


@functools.lru_cache(maxsize=None)
def _data(name):
    c = CASES[name]
    v, t = T.quad_mesh() if c["mesh"] == "quad" else T.obj_mesh(c["mesh"])
    gpk = dict(c["gp"])
    if c.get("relative"):
        gpk["h_scale"] *= float((v["position"].max(0) - v["position"].min(0)).max())
    org, dirs = _rays(name if name in TFDM_CASES else ("quad" if c["mesh"] == "quad" else "teapot"), v)
    return v, t, T.two_sine_map(SIZE), api.tfdm_params(**gpk), org, dirs


def _targeted_rays(v, t, gp, rect, size, n=300, seed=41):
    """A changed texel moves the corner heights around it, so the surface moves over the rectangle grown by one texel on every side
    (repeat wrap).  Returns (rays, reached): rays down the interpolated normal onto base-mesh points whose transformed texture
    coordinate lies in that region, or None where the sampling found fewer than MIN_AIMED; reached: does any base triangle's footprint overlap the
    region at all (separating axes, float64)."""
    x0, y0, w, h = rect
    rng = np.random.default_rng(seed)
    pts = np.stack([(x0 - 1 + rng.uniform(0, 1, n) * (w + 2)) / size, (y0 - 1 + rng.uniform(0, 1, n) * (h + 2)) / size], 1)
    t = np.asarray(t).reshape(-1, 3)
    X = T.transform64(gp)
    uv = v["texCoord"][t].astype(np.float64)
    tc = uv @ X[:2, :2].T + X[:2, 2]                                          # [tris, 3, 2]
    lo, hi = np.floor(tc.min((0, 1))).astype(int) - 1, np.floor(tc.max((0, 1))).astype(int) + 1
    a, e1, e2 = tc[:, 0], tc[:, 1] - tc[:, 0], tc[:, 2] - tc[:, 0]
    det = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    ok = det != 0
    org, dirs = [np.zeros((0, 3))], [np.zeros((0, 3))]
    ext = float(np.linalg.norm(v["position"].max(0).astype(np.float64) - v["position"].min(0)))
    cx, cy = np.meshgrid((np.arange(x0 - 1, x0 + w + 1) + 0.5) / size, (np.arange(y0 - 1, y0 + h + 1) + 0.5) / size)
    rlo, rhi = np.array([x0 - 1, y0 - 1]) / size, np.array([x0 + w + 1, y0 + h + 1]) / size
    shifts = [(sx, sy) for sx in range(lo[0], hi[0] + 1) for sy in range(lo[1], hi[1] + 1)]
    near = {sh: np.nonzero(ok & np.all(tc.max(1) > rlo + sh, 1) & np.all(tc.min(1) < rhi + sh, 1))[0] for sh in shifts}      # bounding boxes
    for sh, k in near.items():
        if len(k) == 0:
            continue
        d = (pts + sh)[:, None, :] - a[None, k]                               # [pts, near triangles, 2]
        bb = (d[..., 0] * e2[None, k, 1] - d[..., 1] * e2[None, k, 0]) / det[None, k]
        bc = (e1[None, k, 0] * d[..., 1] - e1[None, k, 1] * d[..., 0]) / det[None, k]
        pi, ti = np.nonzero((bb > 1e-3) & (bc > 1e-3) & (bb + bc < 1 - 1e-3))
        b = np.stack([1 - bb[pi, ti] - bc[pi, ti], bb[pi, ti], bc[pi, ti]], 1)
        P = np.einsum("kv,kvc->kc", b, v["position"][t[k[ti]]].astype(np.float64))
        N = np.einsum("kv,kvc->kc", b, v["normal"][t[k[ti]]].astype(np.float64))
        with np.errstate(all="ignore"):
            N /= np.linalg.norm(N, axis=1, keepdims=True)
        keep = np.isfinite(N).all(1)
        org.append((P + 0.6 * ext * N)[keep]); dirs.append(-N[keep])
    org, dirs = np.concatenate(org), np.concatenate(dirs)
    if len(org) >= MIN_AIMED:
        pick = np.random.default_rng(seed + 1).permutation(len(org))[:n]
        return T.pack_rays(org[pick], dirs[pick]), True
    return None, any(T.overlap_sat(tc[i], cx + sh[0], cy + sh[1], 0.5 / size).any() for sh, k in near.items() for i in k)


def _make(kind, ctx, v, t, heights, gp):
    return (api.Nrtdsm if kind == "nrtdsm" else api.Tfdm)(ctx, v, t, heights, gp)


def _host_state(hosts, kind, v, t, heights, gp):
    return hosts[kind].state(v, t, heights, gp)


def _host_trace(hosts, kind, st, mode, org, dirs):
    return hosts["nrtdsm"].trace(st, mode, org, dirs) if kind == "nrtdsm" else hosts["tfdm"].trace_state(st, mode, org, dirs)


def _update(obj, new, rect, pitched=False):
    """pitched: the source is the whole new map on the device, addressed at the rectangle's first texel with the map's pitch."""
    import torch
    x0, y0, w, h = rect
    size = new.shape[0]
    if pitched:
        d = torch.from_numpy(np.ascontiguousarray(new, np.float32)).cuda()
        obj.update_heights(d.data_ptr() + 4 * (y0 * size + x0), x0, y0, w, h, pitch=size, stream=torch.cuda.current_stream().cuda_stream)
    else:
        d = torch.from_numpy(np.ascontiguousarray(new[y0:y0 + h, x0:x0 + w], np.float32)).cuda()
        obj.update_heights(d.data_ptr(), x0, y0, w, h, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def _read_all(obj):
    levels = int(np.log2(obj.size)) + 1
    return {"heights": [obj.read_heights(k) for k in range(levels)], "pyramid": [obj.read_pyramid(k) for k in range(levels)],
            "aabbs": obj.read_aabbs(), "records": obj.read_records(), "nodes": obj.read_nodes()}


def _assert_same_object(what, got, want, nodes=False):
    for k, (a, b) in enumerate(zip(got["heights"], want["heights"])):
        util.assert_same_bits("%s: height level %d" % (what, k), a, b)
    for k, (a, b) in enumerate(zip(got["pyramid"], want["pyramid"])):
        util.assert_same_bits("%s: pyramid level %d" % (what, k), a, b)
    util.assert_same_bits(what + ": per-triangle boxes", got["aabbs"], want["aabbs"])
    util.assert_same_bits(what + ": records", got["records"], want["records"])
    if nodes:
        util.assert_same_bits(what + ": tree", got["nodes"], want["nodes"])


def _assert_same_hits(what, got, want):
    for f in api.TFDM_HIT_DTYPE.names:
        util.assert_same_bits("%s: closest hit, %s" % (what, f), got[f], want[f])


def _check_update(hosts, kind, what, v, t, heights, new, gp, rect, org, dirs, pitched=False, expect_change=True, ctx=None, obj=None):
    """One update of `obj` (made here from `heights` unless given) to `new`, and every comparison of the module docstring."""
    aimed, reached = _targeted_rays(v, t, gp, rect, new.shape[0])
    if aimed is not None:
        org, dirs = np.concatenate([org, aimed[0]]), np.concatenate([dirs, aimed[1]])
    ctx = ctx or api.Context(0)
    obj = obj or _make(kind, ctx, v, t, heights, gp)
    fresh = _make(kind, ctx, v, t, new, gp)
    heights_before = obj.read_heights(0)
    nodes_before = obj.read_nodes()
    hits_before = gpu_tfdm_trace(obj, api.TRACE_CLOSEST, org, dirs)
    _update(obj, new, rect, pitched)
    got, want = _read_all(obj), _read_all(fresh)
    _assert_same_object(what, got, want)
    U.assert_refitted(what, got["nodes"], nodes_before, got["aabbs"])
    hits = gpu_tfdm_trace(obj, api.TRACE_CLOSEST, org, dirs)
    occ = gpu_tfdm_trace(obj, api.TRACE_ANY, org, dirs)
    st = dict(_host_state(hosts, kind, v, t, new, gp))
    st["nodes"] = got["nodes"]
    _assert_same_hits(what + ", against the host core on the device's nodes", hits, _host_trace(hosts, kind, st, api.TRACE_CLOSEST, org, dirs))
    util.assert_same_bits(what + ": any hit against the host core", occ, _host_trace(hosts, kind, st, api.TRACE_ANY, org, dirs))
    fresh_hits = gpu_tfdm_trace(fresh, api.TRACE_CLOSEST, org, dirs)
    print("%s: %d of %d closest hits differ from the fresh object's" % (what, int((hits.view(np.uint8).reshape(len(hits), -1) != fresh_hits.view(np.uint8).reshape(len(hits), -1)).any(1).sum()), len(hits)))
    util.assert_same_bits(what + ": any hit against the fresh object", occ, gpu_tfdm_trace(fresh, api.TRACE_ANY, org, dirs))
    _assert_same_hits(what + ", against the fresh object", hits, fresh_hits)
    changed = int((hits["dist"].view(np.uint32) != hits_before["dist"].view(np.uint32)).sum())
    print("%s: %d of %d hit distances changed" % (what, changed, len(hits)))
    assert not np.array_equal(got["heights"][0], heights_before), what + ": the heights did not change"
    if expect_change and aimed is not None:
        assert changed > 0, what + ": no hit distance changed, the update may have done nothing"
    elif expect_change and not reached:  # no base triangle reaches the rectangle: nothing of the surface may have moved
        _assert_same_hits(what + ", a rectangle no footprint reaches", hits, hits_before)
    fresh.close()
    return ctx, obj


@pytest.mark.parametrize("rect", RECTS, ids=lambda r: "x".join(str(v) for v in r))
@pytest.mark.parametrize("name", sorted(CASES))
def test_update_equals_a_fresh_object(built_lib, hosts, name, rect):
    v, t, heights, gp, org, dirs = _data(name)
    new = U.bumped_map(heights, rect, 1 + RECTS.index(rect))
    _, obj = _check_update(hosts, CASES[name]["kind"], "%s %s" % (name, rect), v, t, heights, new, gp, rect, org, dirs, pitched=RECTS.index(rect) % 2 == 1)
    obj.close()


@pytest.mark.parametrize("kind", ["tfdm", "nrtdsm"])
def test_overlapping_updates_and_the_restored_map(built_lib, hosts, kind):
    v, t, heights, gp, org, dirs = _data("quad" if kind == "tfdm" else "nrtdsm_quad")
    ctx = api.Context(0)
    obj, twin = _make(kind, ctx, v, t, heights, gp), _make(kind, ctx, v, t, heights, gp)
    first, second = (10, 12, 30, 20), (25, 5, 30, 40)
    m1 = U.bumped_map(heights, first, 11)
    m2 = U.bumped_map(m1, second, 12)
    _update(obj, m1, first)
    _update(obj, m2, second, pitched=True)
    fresh = _make(kind, ctx, v, t, m2, gp)
    _assert_same_object(kind + ": after two overlapping updates", _read_all(obj), _read_all(fresh))
    _assert_same_hits(kind + ": after two overlapping updates", gpu_tfdm_trace(obj, api.TRACE_CLOSEST, org, dirs), gpu_tfdm_trace(fresh, api.TRACE_CLOSEST, org, dirs))
    _update(obj, heights, (10, 5, 45, 40), pitched=True)              # the union of the two: the original map again
    _assert_same_object(kind + ": restored", _read_all(obj), _read_all(twin), nodes=True)
    _assert_same_hits(kind + ": restored", gpu_tfdm_trace(obj, api.TRACE_CLOSEST, org, dirs), gpu_tfdm_trace(twin, api.TRACE_CLOSEST, org, dirs))
    for o in (obj, twin, fresh):
        o.close()


def _one_triangle():
    v, t = T.quad_mesh()
    return v, t[:1]


def _zero_area_triangle():
    v, t = T.quad_mesh()
    v = v.copy()
    v["texCoord"] = (0.25, 0.25)          # every vertex at one texture coordinate: no roots, a box that is empty by the record
    return v, t[:1]


@pytest.mark.parametrize("edge", ["one_triangle", "size_1", "size_2", "zero_texture_area"])
@pytest.mark.parametrize("kind", ["tfdm", "nrtdsm"])
def test_edge_objects(built_lib, hosts, kind, edge):
    _, _, _, _, org, dirs = _data("quad")
    gp = api.tfdm_params(h_scale=0.1)
    v, t = T.quad_mesh()
    heights, rect = T.two_sine_map(SIZE), (5, 9, 17, 30)
    if edge == "one_triangle":
        v, t = _one_triangle()
    elif edge == "zero_texture_area":
        v, t = _zero_area_triangle()
    elif edge == "size_1":
        heights, rect = np.full((1, 1), 0.25, np.float32), (0, 0, 1, 1)
    elif edge == "size_2":
        heights, rect = np.array([[0.1, 0.9], [0.4, 0.6]], np.float32), (1, 0, 1, 2)
    new = U.bumped_map(heights, rect, 5)
    ctx = api.Context(0)
    obj = _make(kind, ctx, v, t, heights, gp)
    nodes = obj.read_nodes()
    if edge in ("one_triangle", "zero_texture_area"):
        assert len(nodes) == 1 and nodes["count"][0] == 1
    if edge == "zero_texture_area":
        assert U.box_empty(obj.read_aabbs()).all() and not nodes["lo"].any() and not nodes["hi"].any()
    _check_update(hosts, kind, "%s %s" % (kind, edge), v, t, heights, new, gp, rect, org, dirs, expect_change=edge != "zero_texture_area", ctx=ctx, obj=obj)
    if edge == "zero_texture_area":
        util.assert_same_bits("the nothing-to-hit tree keeps its zero box", obj.read_nodes(), nodes)
    obj.close()


@pytest.mark.parametrize("kind", ["tfdm", "nrtdsm"])
def test_update_after_set_params(built_lib, hosts, kind):
    """set_params makes a new tree, so the level table of the refit must be made again."""
    v, t, heights, _, org, dirs = _data("bunny")
    ext = float((v["position"].max(0) - v["position"].min(0)).max())
    gp0, gp1 = api.tfdm_params(h_scale=0.02 * ext), api.tfdm_params(h_scale=0.05 * ext, tex_scale=(2.0, 3.0), tex_offset=(0.1, 0.2))
    ctx = api.Context(0)
    obj = _make(kind, ctx, v, t, heights, gp0)
    rect = (0, 0, 40, 64)
    _update(obj, U.bumped_map(heights, rect, 8), rect)                # the table of the first tree is made here
    obj.set_params(gp1)
    mid = U.bumped_map(heights, rect, 8)
    rect2 = (20, 3, 44, 50)
    _check_update(hosts, kind, kind + " after set_params", v, t, mid, U.bumped_map(mid, rect2, 9), gp1, rect2, org, dirs, ctx=ctx, obj=obj)
    obj.close()


@pytest.mark.parametrize("kind", ["tfdm", "nrtdsm"])
def test_device_bytes_grow_only_at_the_first_update(built_lib, kind):
    v, t, heights, gp, _, _ = _data("quad")
    ctx = api.Context(0)
    obj, twin = _make(kind, ctx, v, t, heights, gp), _make(kind, ctx, v, t, heights, gp)
    levels = sum((SIZE >> k) ** 2 for k in range(7))
    rec = 144 if kind == "nrtdsm" else 192
    assert obj.device_bytes() == twin.device_bytes() == levels * 12 + 2 * (rec + 24) + 3 * 32      # what an object owned before updates existed
    rect = (3, 3, 5, 5)
    _update(obj, U.bumped_map(heights, rect, 2), rect)
    grown = obj.device_bytes()
    assert grown > twin.device_bytes()
    _update(obj, U.bumped_map(heights, rect, 3), rect)
    assert obj.device_bytes() == grown
    obj.close(), twin.close()


@pytest.mark.parametrize("kind", ["tfdm", "nrtdsm"])
def test_refusals_are_errors_with_a_text_and_change_nothing(built_lib, kind):
    import torch
    v, t, heights, gp, org, dirs = _data("quad")
    ctx = api.Context(0)
    obj = _make(kind, ctx, v, t, heights, gp)
    before_hits, before = gpu_tfdm_trace(obj, api.TRACE_CLOSEST, org, dirs), _read_all(obj)
    src = torch.full((16, 16), 0.5, dtype=torch.float32, device="cuda")
    p = src.data_ptr()
    name = "gfx_%s_update_heights" % kind

    def refused(text, ptr, x0, y0, w, h, pitch=None):
        with pytest.raises(api.GfxError, match=text) as e:
            obj.update_heights(ptr, x0, y0, w, h, pitch=pitch)
        assert name in str(e.value)

    refused("null or not 4-byte aligned", 0, 0, 0, 4, 4)
    refused("null or not 4-byte aligned", p + 2, 0, 0, 4, 4)
    refused("rectangle is empty", p, 0, 0, 0, 4)
    refused("rectangle is empty", p, 0, 0, 4, 0)
    refused("srcPitch is smaller", p, 0, 0, 8, 4, pitch=7)
    refused("leaves the map", p, 60, 0, 5, 4)
    refused("leaves the map", p, 0, 61, 4, 4)
    refused("leaves the map", p, 0xFFFFFFFF, 0, 2, 1, pitch=16)
    bad = src.clone()
    bad[3, 5] = float("nan")
    refused("not finite", bad.data_ptr(), 8, 8, 16, 16)
    bad[3, 5] = float("inf")
    refused("not finite", bad.data_ptr(), 8, 8, 16, 16)
    bad[3, 5] = 1.5
    if kind == "nrtdsm":
        refused(r"outside \[0, 1\]", bad.data_ptr(), 8, 8, 16, 16)
        bad[3, 5] = -0.25
        refused(r"outside \[0, 1\]", bad.data_ptr(), 8, 8, 16, 16)
    torch.cuda.synchronize()
    _assert_same_object(kind + ": after the refusals", _read_all(obj), before, nodes=True)
    _assert_same_hits(kind + ": after the refusals", gpu_tfdm_trace(obj, api.TRACE_CLOSEST, org, dirs), before_hits)
    if kind == "tfdm":                      # TFDM takes any finite height
        obj.update_heights(bad.data_ptr(), 8, 8, 16, 16)
        assert obj.read_heights(0)[8 + 3, 8 + 5] == np.float32(1.5)
    obj.close()


def test_an_object_with_supplied_mips_is_refused(built_lib):
    import torch
    heights = T.two_sine_map(SIZE)
    v, t = T.quad_mesh()
    ctx = api.Context(0)
    for cls in (api.Tfdm, api.Nrtdsm):
        obj = cls(ctx, v, t, T.mips32(heights), api.tfdm_params(h_scale=0.1))
        before = _read_all(obj)
        src = torch.full((4, 4), 0.5, dtype=torch.float32, device="cuda")
        with pytest.raises(api.GfxError, match="update_heights: the object was created with its own mip levels"):
            obj.update_heights(src.data_ptr(), 0, 0, 4, 4)
        _assert_same_object("supplied mips", _read_all(obj), before, nodes=True)
        obj.close()


def test_an_update_that_empties_boxes_rebuilds_the_tree(built_lib):
    """NRTDSM leaves a box empty where hOffset + s h overflows, which depends on the heights: with such parameters an update goes
    through the records and the tree of a fresh build instead of the refit, in both directions."""
    v, t = T.quad_mesh()
    gp = api.tfdm_params(h_offset=3.0e38, h_scale=3.0e38)
    zeros, ones = np.zeros((SIZE, SIZE), np.float32), np.ones((SIZE, SIZE), np.float32)
    ctx = api.Context(0)
    obj = api.Nrtdsm(ctx, v, t, zeros, gp)
    assert not U.box_empty(obj.read_aabbs()).any()
    _update(obj, ones, (0, 0, SIZE, SIZE))
    assert U.box_empty(obj.read_aabbs()).all()
    _assert_same_object("emptied", _read_all(obj), _read_all(api.Nrtdsm(ctx, v, t, ones, gp)), nodes=True)
    _update(obj, zeros, (0, 0, SIZE, SIZE))
    _assert_same_object("filled again", _read_all(obj), _read_all(api.Nrtdsm(ctx, v, t, zeros, gp)), nodes=True)
    obj.close()
