"""-m gpu: shell mapping through the C ABI (gfx_shell_*).

Bit for bit against the host compilation of the same core (tests/shell_host.cpp) on the six cases of tests/shell_host.py: the records,
the per-triangle boxes, the base tree, the shell BVH's nodes and triangles, every field of every closest hit, the counters and the
any-hit word.  The host core has completed every ray set before the device sees it.

Independent of the core: on the quad the map is affine, so the shell-mapped scene IS a triangle mesh.  Box and bunny are
instantiated over the tiles in float64, uploaded as ordinary triangles and traced by the existing gfx_trace; gfx_shell_trace agrees
on hit / miss on the rays the model's edge rule keeps and on the distance within the tolerance of tests/test_shell_cpu.py, with E_mesh
measured on the device in the same run (the fixture of tests/test_gpu_tfdm.py).

Consistency with the displacement half: the two-triangles-per-texel height field of a 4 x 4 map as a shell mesh at texScale 1 against
gfx_nrtdsm_trace on the same map, over the cap.

Measured on an MI355X: DESIGN.md section 21."""
import ctypes as C

import numpy as np
import pytest

from gfxexp_amd import api
from tests import nrtdsm_host as NH
from tests import nrtdsm_ref as NR
from tests import shell_host as SH
from tests import shell_ref as SR
from tests import tfdm_host as T
from tests import util
from tests.test_gpu_tfdm import _upload_mesh, e_mesh, gpu_tfdm_trace      # noqa: F401 -- e_mesh: the fixture, measured on the device
from tests.test_nrtdsm_cpu import EDGE_CAP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host(built_lib, tmp_path_factory):
    return SH.Host(tmp_path_factory.mktemp("shell_host"))


def gpu_shell_trace(sh, mode, org, dirs, counters=False):
    import torch
    n = len(org)
    d_org = torch.from_numpy(np.ascontiguousarray(org, np.float32)).cuda()
    d_dir = torch.from_numpy(np.ascontiguousarray(dirs, np.float32)).cuda()
    d_out = torch.zeros(n if mode == api.TRACE_ANY else n * 12, dtype=torch.int32, device="cuda")
    d_cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    sh.trace(mode, d_org.data_ptr(), d_dir.data_ptr(), n, d_out.data_ptr(), d_cnt.data_ptr() if counters else 0, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    res = out.view(np.uint32) if mode == api.TRACE_ANY else out.view(api.SHELL_HIT_DTYPE).reshape(n)
    return (res, d_cnt.cpu().numpy().astype(np.uint64)) if counters else res


def unit(d):
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


@pytest.mark.parametrize("name", sorted(SH.CASES))
def test_everything_equals_the_host_core_bit_for_bit(built_lib, host, name):
    v, t, geoms, gp, (org, dirs) = SH.case_inputs(name)
    st = host.state(v, t, geoms, gp)
    want, wcnt, it = host.trace(st, api.TRACE_CLOSEST, org, dirs, counters=True, iterations=True)       # the CPU first
    wocc = host.trace(st, api.TRACE_ANY, org, dirs)
    assert it.max() < host.max_descent
    ctx = api.Context(0)
    sh = api.Shell(ctx, v, t, geoms, gp)
    util.assert_same_bits(name + ": shell nodes", sh.read_shell_nodes(), st["shell_nodes"])
    util.assert_same_bits(name + ": shell triangles", sh.read_shell_triangles(), st["shell_tris"])
    util.assert_same_bits(name + ": records", sh.read_records(), st["records"])
    util.assert_same_bits(name + ": per-triangle boxes", sh.read_aabbs(), st["aabbs"])
    util.assert_same_bits(name + ": tree", sh.read_nodes(), st["nodes"])
    assert sh.device_bytes() >= st["records"].nbytes + st["shell_nodes"].nbytes + st["shell_tris"].nbytes
    got, cnt = gpu_shell_trace(sh, api.TRACE_CLOSEST, org, dirs, counters=True)
    hit = want["primIndex"] != api.GFX_INVALID_SLOT
    assert 0.1 < hit.mean() < 0.98, "%s: %.1f %% of the rays hit" % (name, 100 * hit.mean())
    for f in api.SHELL_HIT_DTYPE.names:
        util.assert_same_bits("%s: closest hit, %s" % (name, f), got[f], want[f])
    assert np.array_equal(cnt, wcnt), "%s: counters %s on the device, %s on the host" % (name, cnt, wcnt)
    occ = gpu_shell_trace(sh, api.TRACE_ANY, org, dirs)
    assert np.array_equal(occ, wocc) and np.array_equal(occ == 1, hit) and np.all(occ <= 1)
    assert np.all(got["primIndex"][-SH.N_BAD:] == api.GFX_INVALID_SLOT)
    sh.close()


def instantiate(S, tiles):
    """The shell mesh of model S copied into every tile of `tiles` ([(i, j)]) through base triangle 0's affine map, in float64, as
    a VERTEX_DTYPE mesh of ordinary triangles."""
    tl = np.array(tiles, np.float64)
    x = S.m[None] + np.concatenate([tl, np.zeros((len(tl), 1))], 1)[:, None, None, :]       # [tiles, M, 3, 3]
    pts = S.at(0, x.reshape(-1, 3, 3))[0]
    v = np.zeros(3 * len(pts), api.VERTEX_DTYPE)
    v["position"] = pts.reshape(-1, 3)
    v["normal"] = (0, 0, 1)
    v["texCoord0Dir"] = (1, 0, 0)
    return v, np.arange(3 * len(pts), dtype=np.uint32).reshape(-1, 3)


@pytest.mark.parametrize("name", ["quad_box", "quad_bunny"])
def test_against_gfx_trace_on_the_instantiated_quad(built_lib, host, e_mesh, name):
    v, t, geoms, gp, (org, dirs) = SH.case_inputs(name)
    org, dirs = org[:SH.N_RAYS], dirs[:SH.N_RAYS]
    host.trace(host.state(v, t, geoms, gp), api.TRACE_CLOSEST, org, dirs)                 # the CPU first
    S = SR.Surface(v, t, geoms, gp)
    n = int(round(float(gp.texScale[0])))
    mv, mt = instantiate(S, [(i, j) for j in range(n) for i in range(n)])
    m = S.trace(org[:, :3], dirs[:, :3], org[:, 3], dirs[:, 3], k=1)
    assert m["flagged"].mean() <= EDGE_CAP
    keep = ~m["flagged"]
    ctx, accel = _upload_mesh(mv, mt)
    ref = util.gpu_trace(ctx, accel, api.TRACE_CLOSEST, org, dirs)
    sh = api.Shell(ctx, v, t, geoms, gp)
    got = gpu_shell_trace(sh, api.TRACE_CLOSEST, org, dirs)
    ref_hit, got_hit = ref["triIndex"] != api.GFX_INVALID_SLOT, got["primIndex"] != api.GFX_INVALID_SLOT
    assert 0.1 < ref_hit.mean() < 0.99
    bad = keep & (ref_hit != got_hit)
    assert not bad.any(), "%s: hit / miss differs from gfx_trace on %d kept rays, first %d" % (name, bad.sum(), np.nonzero(bad)[0][0])
    both = keep & ref_hit
    assert np.array_equal(np.isfinite(m["t"])[keep], ref_hit[keep])
    # theta from the model's normal at its own closest hit (gfx_trace reports the triangle by its place in the BVH8, not by its index here)
    nrm = S.normal(m["prim"][both], m["tile"][both].astype(np.float64), m["tri"][both], m["a"][both], m["b"][both])
    d64 = dirs[both, :3].astype(np.float64)
    dl = np.linalg.norm(d64, axis=1)
    rt = ref["dist"][both].astype(np.float64)
    tol = 8 * e_mesh * np.maximum(1.0, rt) + 2 * 1e-5 * abs(S.scale) / (np.maximum(np.abs((unit(d64) * nrm).sum(1)), 1e-12) * dl)
    err = np.abs(got["dist"][both].astype(np.float64) - rt)
    print("%s: gfx_shell_trace against gfx_trace on %d instantiated triangles: worst |t - t_ref| %.3e, worst ratio to the tolerance %.3f over %d rays (E_mesh %.3e)"
          % (name, len(mt), err.max(), (err / tol).max(), both.sum(), e_mesh))
    assert (err / tol).max() <= 1
    sh.close()


def test_the_height_field_as_a_shell_agrees_with_the_displacement_query(built_lib, host, e_mesh, tmp_path_factory):
    heights = (np.random.default_rng(9).integers(0, 256, (4, 4)).astype(np.float32) / np.float32(255)).astype(np.float32)
    v, t = NH.cap_mesh(n=4, mirror=(1, 2))
    geoms = [SH.height_field_geom(heights)]
    gps, gpn = api.shell_params(h_scale=0.05), api.tfdm_params(h_scale=0.05)
    org, dirs = T.mesh_rays(v, SH.N_RAYS, 5)
    nhost = NH.Host(tmp_path_factory.mktemp("nrtdsm_host"))
    host.trace(host.state(v, t, geoms, gps), api.TRACE_CLOSEST, org, dirs)                # the CPU first, both cores
    nhost.trace(nhost.state(v, t, heights, gpn), api.TRACE_CLOSEST, org, dirs)
    N = NR.Surface(v, t, heights, gpn)
    m = N.trace(org[:, :3], dirs[:, :3], org[:, 3], dirs[:, 3], k=2)
    S = SR.Surface(v, t, geoms, gps)
    ms = S.trace(org[:, :3], dirs[:, :3], org[:, 3], dirs[:, 3], k=2)
    flagged = m["flagged"] | ms["flagged"]
    print("height field as a shell: edge rays %.2f %%" % (100 * flagged.mean()))
    assert flagged.mean() <= EDGE_CAP
    keep = ~flagged
    # the two models are one surface
    h = keep & np.isfinite(m["t"])
    assert np.array_equal(np.isfinite(m["t"])[keep], np.isfinite(ms["t"])[keep]) and np.abs(m["t"][h] - ms["t"][h]).max() < 1e-6
    ctx = api.Context(0)
    sh, nr = api.Shell(ctx, v, t, geoms, gps), api.Nrtdsm(ctx, v, t, heights, gpn)
    a, b = gpu_shell_trace(sh, api.TRACE_CLOSEST, org, dirs), gpu_tfdm_trace(nr, api.TRACE_CLOSEST, org, dirs)
    ha, hb = a["primIndex"] != api.GFX_INVALID_SLOT, b["primIndex"] != api.GFX_INVALID_SLOT
    assert 0.2 < hb.mean() < 0.98
    assert np.array_equal(ha[keep], hb[keep]) and np.array_equal(ha[keep], np.isfinite(m["t"])[keep])
    assert np.array_equal(a["primIndex"][h], b["primIndex"][h]) and np.array_equal(a["primIndex"][h], m["prim"][h])
    nm = N.normal(m["prim"][h], m["alpha"][h], m["beta"][h])
    d64 = dirs[h, :3].astype(np.float64)
    dl = np.linalg.norm(d64, axis=1)
    tol = 8 * e_mesh * np.maximum(1.0, m["t"][h]) + 2 * 1e-5 * abs(N.scale) / (np.maximum(np.abs((unit(d64) * nm).sum(1)), 1e-12) * dl)
    ea, eb = np.abs(a["dist"][h].astype(np.float64) - m["t"][h]), np.abs(b["dist"][h].astype(np.float64) - m["t"][h])
    print("height field as a shell: worst ratio to the tolerance: gfx_shell_trace %.3f, gfx_nrtdsm_trace %.3f over %d rays" % ((ea / tol).max(), (eb / tol).max(), h.sum()))
    assert (ea / tol).max() <= 1 and (eb / tol).max() <= 1
    # the shell's normal faces where its winding faces: TL-BL-BR in (u, v, h) faces -h, the displacement query's normal +h
    cosn = (a["normal"][h].astype(np.float64) * b["normal"][h].astype(np.float64)).sum(1)
    assert cosn.max() < -0.999
    sh.close()
    nr.close()


def test_set_params_and_set_geometry_equal_a_fresh_object(built_lib, host):
    v, t, _, gpa, (org, dirs) = SH.case_inputs("cap_two_geoms")
    box, pyr = SH.box_geom(), SH.pyramid_geom()
    gpb = api.shell_params(h_scale=3.0, h_bias=0.01, tex_scale=(7.0, 8.0), tex_rotation=15.0, tex_offset=(0.1, -1.2))
    for gp, geoms in ((gpa, [box]), (gpb, [box]), (gpb, [box, pyr])):
        host.trace(host.state(v, t, geoms, gp), api.TRACE_CLOSEST, org, dirs)             # the CPU first
    ctx = api.Context(0)
    changed = api.Shell(ctx, v, t, [box], gpa)
    before = gpu_shell_trace(changed, api.TRACE_CLOSEST, org, dirs)
    for step, (gp, geoms) in enumerate(((gpb, [box]), (gpb, [box, pyr]))):
        if step == 0:
            changed.set_params(gp)
        else:
            changed.set_geometry(geoms)
        fresh = api.Shell(ctx, v, t, geoms, gp)
        for what in ("read_records", "read_aabbs", "read_nodes", "read_shell_nodes", "read_shell_triangles"):
            util.assert_same_bits("step %d: %s" % (step, what), getattr(changed, what)(), getattr(fresh, what)())
        after, want = gpu_shell_trace(changed, api.TRACE_CLOSEST, org, dirs), gpu_shell_trace(fresh, api.TRACE_CLOSEST, org, dirs)
        util.assert_same_bits("step %d: hits" % step, after, want)
        assert not np.array_equal(before["dist"], after["dist"])
        before = after
        fresh.close()
    assert (before["shellGeom"] == 1).any()
    changed.close()


def test_refusals_are_errors_with_a_text(built_lib, host):
    L = built_lib
    ctx = api.Context(0)
    v, t = T.quad_mesh()
    pos, tri = api.shell_box()

    def create(geoms, gp=None, v=v):
        arr, keep = api._shell_geoms(geoms)
        h = C.c_void_p()
        rc = L.gfx_shell_create(ctx.h, None, v.ctypes.data_as(C.c_void_p), C.c_uint32(v.itemsize), C.c_uint32(len(v)), t.ctypes.data_as(C.c_void_p),
                                C.c_uint32(len(t)), arr, C.c_uint32(len(keep)), C.byref(gp) if gp is not None else None, C.byref(h))
        return rc, h.value, L.gfx_last_error(ctx.h).decode()

    nan_pos, out_pos = pos.copy(), pos.copy()
    nan_pos[2, 1], out_pos[5, 1] = np.inf, -0.01
    nan_uv = v.copy()
    nan_uv["texCoord"][1, 0] = np.nan
    box = [(pos, tri)]
    refused = [
        ("no shell geometry", dict(geoms=[])),
        ("no triangles", dict(geoms=[(pos, np.zeros((0, 3), np.uint32))])),
        ("2^20", dict(geoms=[(pos, np.zeros(((1 << 20) + 1, 3), np.uint32))])),
        ("more than 8", dict(geoms=box * 9)),
        ("not finite", dict(geoms=[(nan_pos, tri)])),
        ("outside [0, 1]", dict(geoms=[(out_pos, tri)])),
        ("does not exist", dict(geoms=[(pos, tri + 3)])),
        ("targetMipLevel", dict(gp=api.tfdm_params(target_mip_level=1, local_intersection=0))),
        ("localIntersection", dict(gp=api.tfdm_params())),
        ("not finite", dict(gp=api.shell_params(h_scale=float("inf")))),
        ("positive", dict(gp=api.shell_params(tex_scale=(0.0, 1.0)))),
        ("2^22", dict(gp=api.shell_params(tex_offset=(5.0e6, 0.0)))),
        ("not finite", dict(v=nan_uv)),
    ]
    for text, kw in refused:
        rc, h, msg = create(kw.get("geoms", box), kw.get("gp"), kw.get("v", v))
        assert rc != 0 and not h and text in msg, "%s: rc %d, message %r" % (text, rc, msg)
    # the context is alive and well afterwards; a refused call leaves the object tracing bit-identically
    gp = api.shell_params(h_scale=2.0, tex_scale=(4.0, 4.0))
    org, dirs = T.cap_rays(2000)
    host.trace(host.state(v, t, box, gp), api.TRACE_CLOSEST, org, dirs)                   # the CPU first
    sh = api.Shell(ctx, v, t, box, gp)
    want = gpu_shell_trace(sh, api.TRACE_CLOSEST, org, dirs)
    assert (want["primIndex"] != api.GFX_INVALID_SLOT).mean() > 0.2
    for text, bad in [("targetMipLevel", api.tfdm_params(target_mip_level=2, local_intersection=0)), ("localIntersection", api.tfdm_params(local_intersection=api.TFDM_BILINEAR)),
                      ("not finite", api.shell_params(h_scale=float("nan"))), ("positive", api.shell_params(tex_scale=(1.0, -1.0))),
                      ("2\\^22", api.shell_params(tex_offset=(0.0, -3.0e9)))]:
        with pytest.raises(api.GfxError, match=text):
            sh.set_params(bad)
        util.assert_same_bits("hits after a refused set_params (%s)" % text, gpu_shell_trace(sh, api.TRACE_CLOSEST, org, dirs), want)
    for text, geoms in [("no shell geometry", []), ("more than 8", box * 9), ("not finite", [(nan_pos, tri)]), ("outside \\[0, 1\\]", [(out_pos, tri)])]:
        with pytest.raises(api.GfxError, match=text):
            sh.set_geometry(geoms)
        util.assert_same_bits("hits after a refused set_geometry (%s)" % text, gpu_shell_trace(sh, api.TRACE_CLOSEST, org, dirs), want)
    with pytest.raises(api.GfxError, match="mode"):
        sh.trace(5, 1, 1, 1, 1)
    with pytest.raises(api.GfxError, match="aligned"):
        sh.trace(api.TRACE_CLOSEST, 256 + 4, 256, 1, 256)
    with pytest.raises(api.GfxError, match="unknown item"):
        sh.size_of(17)
    sh.close()
