"""-m gpu: tessellation-free displacement mapping through the C ABI (gfx_tfdm_*).

Bit for bit against the host compilation of the same core (tests/tfdm_host.cpp): every pyramid level, the per-triangle boxes, the
records, the tree, and every field of every closest hit.  Independent of the core: the displaced quad tessellated in float64 on the
host, uploaded as ordinary triangles and traced by the existing gfx_trace, agrees with gfx_tfdm_trace; and with no displacement the
query returns the base mesh.

Tolerance (tests/test_tfdm_cpu.py has the reasoning): E_mesh is measured here, in the same run, as the largest
|t - t64| / max(1, t64) of gfx_trace on the tessellated 64 x 64 quad against the float64 brute force over the rays the edge rule
keeps; gfx_tfdm_trace is allowed 8 x E_mesh.

Measured on an MI355X: E_mesh = 2.876e-06; gfx_tfdm_trace against gfx_trace on the tessellated 256 x 256 quad over 1920 x 1080
primary rays: 21 rays differ, all of them edge rays, worst error among the others 1.121e-05 = 3.90 x E_mesh."""
import ctypes as C

import numpy as np
import pytest

from gfxexp_amd import api
from tests import tfdm_host as T
from tests import util

pytestmark = pytest.mark.gpu
EDGE_CAP = 0.02


@pytest.fixture(scope="module")
def host(built_lib, tmp_path_factory):
    return T.Host(tmp_path_factory.mktemp("tfdm_host"))


def gpu_tfdm_trace(tf, mode, org, dirs, counters=False):
    import torch
    n = len(org)
    d_org = torch.from_numpy(np.ascontiguousarray(org, np.float32)).cuda()
    d_dir = torch.from_numpy(np.ascontiguousarray(dirs, np.float32)).cuda()
    d_out = torch.zeros(n if mode == api.TRACE_ANY else n * 8, dtype=torch.int32, device="cuda")
    d_cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    tf.trace(mode, d_org.data_ptr(), d_dir.data_ptr(), n, d_out.data_ptr(), d_cnt.data_ptr() if counters else 0, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    res = out.view(np.uint32) if mode == api.TRACE_ANY else out.view(api.TFDM_HIT_DTYPE).reshape(n)
    return (res, d_cnt.cpu().numpy().astype(np.uint64)) if counters else res


def _special_rays(v, rng, n=600):
    """Rays from inside the shell between the base mesh and the surface's highest point, axis-parallel rays, and rays whose tmax ends
    short of the surface."""
    lo, hi = v["position"].min(0).astype(np.float64), v["position"].max(0).astype(np.float64)
    ext = hi - lo
    pts = lo + rng.uniform(0, 1, (n, 3)) * ext
    d = rng.normal(size=(n, 3))
    axis = np.eye(3)[rng.integers(0, 3, n)] * rng.choice([-1.0, 1.0], n)[:, None]
    d[: n // 3] = axis[: n // 3]                                                 # axis-parallel, from inside the bounds
    o, dd = T.pack_rays(pts, d)
    far_o, far_d = T.mesh_rays(v, n, 17)
    far_d[: n // 2, :3] /= np.linalg.norm(far_d[: n // 2, :3], axis=1, keepdims=True)
    far_d[: n // 2, 3] = (0.6 * np.linalg.norm(ext)).astype(np.float32)          # ends before the mesh is reached (origins lie a diagonal away)
    far_d[n // 2:, 3] = rng.uniform(0.5, 1.5, n - n // 2).astype(np.float32)     # ... or somewhere inside it (unnormalised directions toward the bounds)
    return np.concatenate([o, far_o]), np.concatenate([dd, far_d])


CASES = {
    "quad": dict(mesh="quad", gp=dict(h_scale=0.1)),
    "quad_box": dict(mesh="quad", gp=dict(h_scale=0.1, local_intersection=api.TFDM_BOX)),
    "quad_level2": dict(mesh="quad", gp=dict(h_scale=0.1, target_mip_level=2)),
    "quad_box_level2": dict(mesh="quad", gp=dict(h_scale=0.1, target_mip_level=2, local_intersection=api.TFDM_BOX)),
    "quad_wrapped_rotated": dict(mesh="quad", gp=dict(h_scale=0.1, h_offset=0.01, h_bias=0.25, tex_scale=(2.5, 1.5), tex_rotation=30.0, tex_offset=(0.3, -0.2))),
    "quad_supplied_mips": dict(mesh="quad", gp=dict(h_scale=0.1, target_mip_level=2), own_mips=True),
    "bunny": dict(mesh="stanford_bunny_309_faces.obj", gp=dict(h_scale=0.02), relative=True),
    "bunny_box": dict(mesh="stanford_bunny_309_faces.obj", gp=dict(h_scale=0.02, local_intersection=api.TFDM_BOX, tex_scale=(3.0, 3.0), tex_rotation=-20.0), relative=True),
    "teapot": dict(mesh="teapot.obj", gp=dict(h_scale=0.01), relative=True),
    "teapot_level2": dict(mesh="teapot.obj", gp=dict(h_scale=0.01, target_mip_level=2), relative=True),
}


def _case(name):
    c = CASES[name]
    v, t = T.quad_mesh() if c["mesh"] == "quad" else T.obj_mesh(c["mesh"])
    gpk = dict(c["gp"])
    if c.get("relative"):
        gpk["h_scale"] *= float((v["position"].max(0) - v["position"].min(0)).max())
    heights = T.two_sine_map(64)
    if c.get("own_mips"):
        rng = np.random.default_rng(2)
        m = T.mips32(heights)
        heights = [m[0]] + [np.clip(x + rng.uniform(-0.1, 0.1, x.shape), 0, 1).astype(np.float32) for x in m[1:]]
    return v, t, heights, api.tfdm_params(**gpk)


def _rays(name, v):
    rng = np.random.default_rng(23)
    n = 20000
    o, d = T.cap_rays(n) if CASES[name]["mesh"] == "quad" else T.mesh_rays(v, n, 5)
    so, sd = _special_rays(v, rng)
    return np.concatenate([o, so]), np.concatenate([d, sd])


@pytest.mark.parametrize("name", sorted(CASES))
def test_everything_equals_the_host_core_bit_for_bit(built_lib, host, name):
    v, t, heights, gp = _case(name)
    ctx = api.Context(0)
    tf = api.Tfdm(ctx, v, t, heights, gp)
    st = host.state(v, t, heights, gp)
    size = st["size"]
    for level in range(int(np.log2(size)) + 1):
        util.assert_same_bits("%s: height level %d" % (name, level), tf.read_heights(level), host.level(st["levels"], size, level))
        util.assert_same_bits("%s: pyramid level %d" % (name, level), tf.read_pyramid(level), host.level(st["pyramid"], size, level, per=2))
    util.assert_same_bits(name + ": records", tf.read_records(), st["records"])
    util.assert_same_bits(name + ": per-triangle boxes", tf.read_aabbs(), st["aabbs"])
    util.assert_same_bits(name + ": tree", tf.read_nodes(), st["nodes"])
    org, dirs = _rays(name, v)
    got, cnt = gpu_tfdm_trace(tf, api.TRACE_CLOSEST, org, dirs, counters=True)
    want, wcnt = host.trace_state(st, api.TRACE_CLOSEST, org, dirs, counters=True)
    hit = want["primIndex"] != api.GFX_INVALID_SLOT
    assert 0.2 < hit.mean() < 0.98, "%s: %.1f %% of the rays hit" % (name, 100 * hit.mean())
    for f in api.TFDM_HIT_DTYPE.names:
        util.assert_same_bits("%s: closest hit, %s" % (name, f), got[f], want[f])
    assert np.array_equal(cnt, wcnt), "%s: counters %s on the device, %s on the host" % (name, cnt, wcnt)
    occ = gpu_tfdm_trace(tf, api.TRACE_ANY, org, dirs)
    assert np.array_equal(occ == 1, hit) and np.all(occ <= 1)
    # the special rays did what they were made for: some start inside a per-triangle box and hit, some end short
    special = got[20000:]
    assert np.any(special["primIndex"] != api.GFX_INVALID_SLOT) and np.any(special["primIndex"] == api.GFX_INVALID_SLOT)
    assert np.all(got["dist"][~hit] == dirs[~hit, 3])
    tf.close()


def _upload_mesh(mv, mt):
    s = api.HostScene()
    g = s.add_geom(mv, mt, s.add_material_traditional((0.5, 0.5, 0.5), (0, 0, 0), 0.3))
    s.add_instance(s.add_group([g]), api.make_transform())
    ctx = api.Context(0)
    s.upload(ctx)
    return ctx, ctx.accel_build()


def _clip(mm):
    return (mm.tA, mm.tB, mm.tC, mm.baseTc, mm.prim)


@pytest.fixture(scope="module")
def e_mesh(built_lib):
    heights = T.two_sine_map(64)
    v, t = T.quad_mesh()
    mm = T.MicroMesh(v, t, T.mips32(heights), api.tfdm_params(h_scale=0.1))
    mv, mt = mm.float32_mesh()
    ctx, accel = _upload_mesh(mv, mt)
    org, dirs = T.cap_rays(20000)
    hits = util.gpu_trace(ctx, accel, api.TRACE_CLOSEST, org, dirs)
    t64, _, edge, near = T.brute64(mm.A, mm.B, mm.C, org[:, :3], dirs[:, :3], org[:, 3].astype(np.float64), dirs[:, 3].astype(np.float64), clip=_clip(mm))
    flagged = edge | near
    assert flagged.mean() <= EDGE_CAP
    keep = ~flagged
    got_hit = hits["triIndex"] != api.GFX_INVALID_SLOT
    assert np.array_equal(got_hit[keep], np.isfinite(t64)[keep])
    both = keep & got_hit
    e = float((np.abs(hits["dist"][both].astype(np.float64) - t64[both]) / np.maximum(1.0, t64[both])).max())
    print("E_mesh = %.3e (gfx_trace on the tessellated 64 x 64 quad against float64, %d rays)" % (e, both.sum()))
    assert 0 < e < 1e-4
    return e


def test_against_gfx_trace_on_the_tessellated_quad(built_lib, e_mesh):
    """Independent of the core: 256 x 256 map, 1920 x 1080 primary rays of a gfx_camera.  The quad is split along the TL-BR diagonal
    with axis-aligned texture coordinates, so no micro-triangle straddles the base edge and the tessellation IS the surface.

    The edge rule is a property of a ray under the float64 mesh.  Brute force over all 2 M rays x 131 072 triangles is out of reach,
    so: the rays on which the two queries disagree are all put through the float64 brute force and every one of them must carry a
    flag; and the share of flagged rays is asserted on a seeded sample of 1500 rays (and the disagreeing rays themselves must stay
    under the cap)."""
    w, h = 1920, 1080
    heights = (T.two_sine_map(256) * np.float32(0.5) + np.random.default_rng(4).integers(0, 128, (256, 256)).astype(np.float32) / np.float32(255) * np.float32(0.25)).astype(np.float32)
    v, t = T.quad_mesh()
    gp = api.tfdm_params(h_scale=0.05)
    mm = T.MicroMesh(v, t, T.mips32(heights), gp)
    mv, mt = mm.float32_mesh()
    assert len(mt) == 2 * 256 * 256
    ctx, accel = _upload_mesh(mv, mt)
    # the unit quad fills about two thirds of this frame (its plane alone: 0.66 of the pixel centres)
    cam = T.look_at_camera(w, h, (0.5, -0.35, 0.6), (0.5, 0.42, 0.0), fov_y_deg=42.0)
    org, dirs = api.camera_rays(cam, w, h)
    ref = util.gpu_trace(ctx, accel, api.TRACE_CLOSEST, org, dirs)
    tf = api.Tfdm(ctx, v, t, heights, gp)
    got = gpu_tfdm_trace(tf, api.TRACE_CLOSEST, org, dirs)
    ref_hit, got_hit = ref["triIndex"] != api.GFX_INVALID_SLOT, got["primIndex"] != api.GFX_INVALID_SLOT
    assert 0.3 < ref_hit.mean() < 0.99
    both = ref_hit & got_hit
    tol = 8 * e_mesh
    err = np.zeros(len(org))
    err[both] = np.abs(got["dist"][both].astype(np.float64) - ref["dist"][both].astype(np.float64)) / np.maximum(1.0, ref["dist"][both].astype(np.float64))
    differ = (ref_hit != got_hit) | (err > tol)
    print("hit share %.3f; rays on which the queries differ: %d of %d (%d in hit / miss); worst error among the others %.3e = %.2f x E_mesh"
          % (ref_hit.mean(), differ.sum(), len(org), (ref_hit != got_hit).sum(), err[~differ].max(), err[~differ].max() / e_mesh))
    assert differ.mean() <= EDGE_CAP

    def flags(idx):
        _, _, edge, near = T.brute64(mm.A, mm.B, mm.C, org[idx, :3], dirs[idx, :3], org[idx, 3].astype(np.float64), dirs[idx, 3].astype(np.float64), clip=_clip(mm))
        return edge | near
    sample = np.random.default_rng(9).choice(len(org), 1500, replace=False)
    share = flags(sample).mean()
    print("edge rays in the sample of 1500: %.2f %%" % (100 * share))
    assert share <= EDGE_CAP
    idx = np.nonzero(differ)[0]
    assert len(idx) <= 6000
    if len(idx):
        f = flags(idx)
        assert f.all(), "%d rays differ without being edge rays, first: ray %d, gfx_trace %s, gfx_tfdm_trace %s" % ((~f).sum(), idx[~f][0], ref[idx[~f][0]], got[idx[~f][0]])
    # the hit is reported on the right base triangle: TL-TR-BR holds the points with u >= v
    p = org[both, :3].astype(np.float64) + got["dist"][both, None].astype(np.float64) * dirs[both, :3].astype(np.float64)
    clear = np.abs(p[:, 0] - p[:, 1]) > 1e-3
    assert np.array_equal(got["primIndex"][both][clear] == 0, (p[:, 0] > p[:, 1])[clear])
    tf.close()


@pytest.mark.parametrize("mesh", ["quad", "stanford_bunny_309_faces.obj"])
def test_no_displacement_returns_the_base_mesh(built_lib, e_mesh, mesh):
    v, t = T.quad_mesh() if mesh == "quad" else T.obj_mesh(mesh)
    ctx, accel = _upload_mesh(v, t)
    tf = api.Tfdm(ctx, v, t, T.two_sine_map(64), api.tfdm_params(h_scale=0.0, h_offset=0.0))
    org, dirs = T.cap_rays(20000) if mesh == "quad" else T.mesh_rays(v, 20000, 5)
    ref = util.gpu_trace(ctx, accel, api.TRACE_CLOSEST, org, dirs)
    got = gpu_tfdm_trace(tf, api.TRACE_CLOSEST, org, dirs)
    ref_hit, got_hit = ref["triIndex"] != api.GFX_INVALID_SLOT, got["primIndex"] != api.GFX_INVALID_SLOT
    assert 0.2 < ref_hit.mean() < 0.99
    bad = ref_hit != got_hit
    assert not bad.any(), "hit / miss differs on %d rays, first %d: %s vs %s" % (bad.sum(), np.nonzero(bad)[0][0], ref[bad][0], got[bad][0])
    err = np.abs(got["dist"][ref_hit].astype(np.float64) - ref["dist"][ref_hit].astype(np.float64)) / np.maximum(1.0, ref["dist"][ref_hit].astype(np.float64))
    print("%s: worst error against gfx_trace on the base triangles %.3e = %.2f x E_mesh" % (mesh, err.max(), err.max() / e_mesh))
    assert err.max() <= 8 * e_mesh
    tf.close()


def test_set_params_equals_a_fresh_object(built_lib):
    v, t = T.obj_mesh("stanford_bunny_309_faces.obj")
    ext = float((v["position"].max(0) - v["position"].min(0)).max())
    heights = T.two_sine_map(64)
    a = api.tfdm_params(h_scale=0.02 * ext)
    b = api.tfdm_params(h_scale=0.03 * ext, h_bias=0.5, tex_scale=(2.0, 3.0), tex_rotation=15.0, tex_offset=(0.1, 0.2), target_mip_level=1, local_intersection=api.TFDM_BOX)
    ctx = api.Context(0)
    changed, fresh = api.Tfdm(ctx, v, t, heights, a), api.Tfdm(ctx, v, t, heights, b)
    org, dirs = T.mesh_rays(v, 20000, 6)
    before = gpu_tfdm_trace(changed, api.TRACE_CLOSEST, org, dirs)
    changed.set_params(b)
    util.assert_same_bits("records", changed.read_records(), fresh.read_records())
    util.assert_same_bits("boxes", changed.read_aabbs(), fresh.read_aabbs())
    util.assert_same_bits("tree", changed.read_nodes(), fresh.read_nodes())
    util.assert_same_bits("pyramid kept", changed.read_pyramid(0), fresh.read_pyramid(0))
    after, want = gpu_tfdm_trace(changed, api.TRACE_CLOSEST, org, dirs), gpu_tfdm_trace(fresh, api.TRACE_CLOSEST, org, dirs)
    util.assert_same_bits("hits after set_params", after, want)
    assert not np.array_equal(before["dist"], after["dist"])
    # a refused change leaves the object as it was
    with pytest.raises(api.GfxError, match="targetMipLevel"):
        changed.set_params(api.tfdm_params(target_mip_level=9))
    util.assert_same_bits("hits after a refused set_params", gpu_tfdm_trace(changed, api.TRACE_CLOSEST, org, dirs), want)


def test_refusals_are_errors_with_a_text(built_lib):
    L = built_lib
    ctx = api.Context(0)
    v, t = T.quad_mesh()
    good = T.two_sine_map(64)

    def create(heights, size, tris=t, levels=1, gp=None):
        ptrs = (C.POINTER(C.c_float) * levels)(*[heights.ctypes.data_as(C.POINTER(C.c_float))] * levels)
        h = C.c_void_p()
        rc = L.gfx_tfdm_create(ctx.h, None, v.ctypes.data_as(C.c_void_p), C.c_uint32(v.itemsize), C.c_uint32(len(v)), tris.ctypes.data_as(C.c_void_p),
                               C.c_uint32(len(tris)), ptrs, C.c_uint32(levels), C.c_uint32(size), C.byref(gp) if gp is not None else None, C.byref(h))
        return rc, h.value, L.gfx_last_error(ctx.h).decode()

    rc, h, msg = create(np.zeros((48, 48), np.float32), 48)
    assert rc != 0 and not h and "power of two" in msg
    rc, h, msg = create(good, 64, levels=3)            # a level count no square power-of-two map has
    assert rc != 0 and not h and "numLevels" in msg
    rc, h, msg = create(good, 64, tris=np.zeros((0, 3), np.uint32))
    assert rc != 0 and not h and "no triangles" in msg
    rc, h, msg = create(good, 64, gp=api.tfdm_params(target_mip_level=7))
    assert rc != 0 and not h and "targetMipLevel" in msg
    rc, h, msg = create(good, 64, gp=api.tfdm_params(local_intersection=2))
    assert rc != 0 and not h and "localIntersection" in msg
    rc, h, msg = create(good, 64, tris=np.array([[0, 1, 9]], np.uint32))
    assert rc != 0 and not h and "vertex" in msg
    with pytest.raises(api.GfxError, match="square"):   # the wrapper has one size to give: a map that is not square never reaches the library
        api.Tfdm(ctx, v, t, np.zeros((32, 64), np.float32))
    # the context is alive and well afterwards
    tf = api.Tfdm(ctx, v, t, good, api.tfdm_params(h_scale=0.1))
    org, dirs = T.cap_rays(1000)
    assert (gpu_tfdm_trace(tf, api.TRACE_CLOSEST, org, dirs)["primIndex"] != api.GFX_INVALID_SLOT).mean() > 0.5
    with pytest.raises(api.GfxError, match="mode"):
        tf.trace(5, 1, 1, 1, 1)
    with pytest.raises(api.GfxError, match="level"):
        tf.read_pyramid(9)
    # texture coordinates whose texel indices a float no longer holds exactly (and, further out, an int32 not at all): refused at
    # creation and at a change of parameters, and the object answers as before
    rc, h, msg = create(good, 64, gp=api.tfdm_params(tex_offset=(3.0e5, 0.0)))
    assert rc != 0 and not h and "2^24" in msg
    rc, h, msg = create(good, 64, gp=api.tfdm_params(tex_scale=(1.0e6, 1.0e6)))
    assert rc != 0 and not h and "2^24" in msg
    want = gpu_tfdm_trace(tf, api.TRACE_CLOSEST, org, dirs)
    with pytest.raises(api.GfxError, match="2\\^24"):
        tf.set_params(api.tfdm_params(h_scale=0.1, tex_offset=(0.0, -3.0e9)))
    util.assert_same_bits("hits after a refused texOffset", gpu_tfdm_trace(tf, api.TRACE_CLOSEST, org, dirs), want)
    tf.set_params(api.tfdm_params(h_scale=0.1, tex_offset=(1000.25, -2000.5)))      # far out, and fine: 2.6e5 x 64 stays below 2^24
    assert (gpu_tfdm_trace(tf, api.TRACE_CLOSEST, org, dirs)["primIndex"] != api.GFX_INVALID_SLOT).mean() > 0.5
    # misaligned buffers are refused before anything is launched
    for args in [(api.TRACE_CLOSEST, 256 + 4, 256, 1, 256), (api.TRACE_CLOSEST, 256, 256 + 8, 1, 256), (api.TRACE_CLOSEST, 256, 256, 1, 256 + 4),
                 (api.TRACE_ANY, 256, 256, 1, 256 + 2)]:
        with pytest.raises(api.GfxError, match="aligned"):
            tf.trace(*args)
    with pytest.raises(api.GfxError, match="8-byte"):
        tf.trace(api.TRACE_ANY, 256, 256, 1, 256 + 4, d_counters=256 + 4)
    tf.close()
