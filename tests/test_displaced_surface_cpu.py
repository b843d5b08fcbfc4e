"""No GPU: gfxexp_amd/csrc/tfdm/displaced_surface.hip.h, the surface point and the G-buffer words of a displaced hit, compiled for
the host (tests/displaced_host.cpp) and held against float64 numpy written here, over 2000 seeded synthetic hits under each of the
three exact transforms of tests/test_scene_trace_cpu.py (uniform, non-uniform, mirrored).

Where the bounds come from.
  position   org + dist * dir is one product and one sum per coordinate: at most 1.5 ulp of the larger operand; the issue's bound is
             4 ulp of max(|org|, dist |dir|) per coordinate.
  u, v       three products and two sums of fp32 values, and bcA = 1 - (bcB + bcC) itself rounded twice: below 8 x 2^-24 = 5e-7 of
             the sum of the terms' magnitudes; held to 1e-6 of that sum (the result itself may cancel to anything).
  tangent    a unit vector, compared by component to 1e-6.  The projection t - (n . t) n loses accuracy as t nears n, so the synthetic
             texCoord0Dir keeps its part orthogonal to the normal at least half its length (drawn that way, not filtered after the
             fact); the fp32 error is then a few 2^-24 and 1e-6 holds with room.
  encodings  the 16-bit polar quantiser truncates: theta is off by up to pi / 65535, phi by up to 2 pi / 65535, so a decoded unit
             vector is within their sum (1.44e-4) of the encoded one; barycentrics and texture coordinates within 1 / 65535.
  motion     with prevCamera = camera and the ray through the pixel centre the vector is zero in real arithmetic.  In fp32 the
             normalised screen position (in [0, 1]) carries about 16 roundings of 2^-24, times the 96-pixel width: 1e-4 pixel; held
             to 5e-4."""
import re

import numpy as np
import pytest

from gfxexp_amd import api
from oracle import oracle as O
from tests import displaced_host as D
from tests import scene_trace_host as S
from tests import tfdm_host as T
from tests.test_scene_trace_cpu import EXACT

W, H, N = 96, 64, 2000
POLAR_STEP = 3 * np.pi / 65535 + 1e-6


@pytest.fixture(scope="module")
def dhost(built_lib, tmp_path_factory):
    return D.DisplacedHost(tmp_path_factory.mktemp("displaced_host"))


@pytest.fixture(scope="module")
def shost(built_lib, tmp_path_factory):
    return S.SceneHost(tmp_path_factory.mktemp("scene_host"))


def _record(shost, m, user_id=0):
    root = np.zeros(1, api.TFDM_NODE_DTYPE)
    root["lo"], root["hi"], root["count"] = (0, 0, 0), (1, 1, 0.2), 1
    return shost.make_instance(m, root[0], (64, 128, 192, 256), T.CoreParams(), user_id)


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def synthetic_hits(L, seed, index_k=0):
    """N hits seen by the camera's pixel-centre rays: (cam, hits, org, dirs, base_verts, xy).  The normals are unit to fp32; each
    vertex's texCoord0Dir is drawn in WORLD space as a vector whose part orthogonal to the normal is at least half its length, and
    taken to object space through the exact inverse of L (signed permutation x powers of two)."""
    rng = np.random.default_rng(seed)
    cam = T.look_at_camera(W, H, (1.25, -3.5, 2.75), (0.5, 0.5, 0.0), fov_y_deg=40.0)
    org_all, dir_all = api.camera_rays(cam, W, H)
    pix = rng.choice(W * H, N, replace=False)
    org, dirs = org_all[pix].copy(), dir_all[pix].copy()
    xy = np.stack([pix % W, pix // W], 1).astype(np.int32)
    hits = np.zeros(N, api.SCENE_HIT_DTYPE)
    hits["dist"] = rng.uniform(0.1, 20.0, N)
    b = rng.uniform(0, 1, (N, 2))
    flip = b.sum(1) > 1
    b[flip] = 1 - b[flip]
    hits["bcB"], hits["bcC"] = b[:, 0], b[:, 1]
    hits["index"] = rng.integers(0, 300, N)
    n = _unit(rng.normal(size=(N, 3))).astype(np.float32)
    hits["normal"] = n
    hits["where"] = (index_k << 1) | rng.integers(0, 2, N)
    n64 = _unit(n.astype(np.float64))
    Linv = np.linalg.inv(np.asarray(L, np.float64))
    bv = np.zeros((N, 3, 5), np.float32)
    perp = _unit(np.cross(n64, rng.normal(size=(N, 3))))
    for k in range(3):
        along = rng.uniform(-1.0, 1.0, (N, 1))
        w = rng.uniform(0.5, 2.0, (N, 1)) * (perp * np.sqrt(1 - 0.25 * along ** 2) + 0.5 * along * n64)     # |perp part| >= 0.86 |w|
        bv[:, k, :3] = w @ Linv.T
        bv[:, k, 3:] = rng.uniform(-2.0, 3.0, (N, 2))
    return cam, hits, org, dirs, bv.reshape(N, 15), xy


def reference64(L, hits, org, dirs, bv):
    o, d = org[:, :3].astype(np.float64), dirs[:, :3].astype(np.float64)
    t = hits["dist"].astype(np.float64)[:, None]
    bcB, bcC = hits["bcB"].astype(np.float64), hits["bcC"].astype(np.float64)
    bc = np.stack([1 - (bcB + bcC), bcB, bcC], 1)
    v = bv.reshape(-1, 3, 5).astype(np.float64)
    tc_obj = np.einsum("nk,nkc->nc", bc, v[:, :, :3])
    uv = np.einsum("nk,nkc->nc", bc, v[:, :, 3:])
    uv_scale = np.einsum("nk,nkc->nc", np.abs(bc), np.abs(v[:, :, 3:]))
    n = hits["normal"].astype(np.float64)
    tw = tc_obj @ np.asarray(L, np.float64).T
    tw = tw - np.sum(n * tw, 1, keepdims=True) * n
    return o + t * d, _unit(tw), uv, uv_scale


@pytest.mark.parametrize("name", sorted(EXACT))
def test_surface_point_and_gbuffer_words_against_float64(dhost, shost, name):
    L, tr = EXACT[name]
    rec = _record(shost, S.affine(L, tr))
    table = np.concatenate([rec] * 3)
    cam, hits, org, dirs, bv, xy = synthetic_hits(L, seed=sorted(EXACT).index(name) + 5, index_k=2)
    geom, mat = np.full(N, 7, np.uint32), np.full(N, 3, np.uint32)
    out = dhost.resolve(table, hits, org, dirs, bv, geom, mat, xy, cam, W, H)
    pos64, tan64, uv64, uv_scale = reference64(L, hits, org, dirs, bv)
    pts = out["points"].astype(np.float64)
    # position: on the ray, 4 ulp of the larger operand per coordinate
    big = np.maximum(np.abs(org[:, :3]), np.abs(hits["dist"][:, None] * dirs[:, :3])).astype(np.float32)
    err_ulp = np.abs(pts[:, :3] - pos64) / np.spacing(big).astype(np.float64)
    print("%s: position worst %.2f ulp" % (name, err_ulp.max()))
    assert err_ulp.max() <= 4.0
    # normal passes through; texture coordinate and tangent
    assert np.array_equal(out["points"][:, 3:6], hits["normal"])
    uv_err = np.abs(pts[:, 9:11] - uv64) / uv_scale
    tan_err = np.abs(pts[:, 6:9] - tan64)
    n64 = hits["normal"].astype(np.float64)
    print("%s: uv worst %.2e of the terms, tangent worst %.2e, |t| - 1 worst %.2e, n . t worst %.2e" %
          (name, uv_err.max(), tan_err.max(), np.abs(np.linalg.norm(pts[:, 6:9], axis=1) - 1).max(), np.abs(np.sum(n64 * pts[:, 6:9], 1)).max()))
    assert uv_err.max() <= 1e-6 and tan_err.max() <= 1e-6
    assert np.abs(np.linalg.norm(pts[:, 6:9], axis=1) - 1).max() <= 1e-6 and np.abs(np.sum(n64 * pts[:, 6:9], 1)).max() <= 1e-6
    # the words: ids, barycentrics, position bits, normals and tangent through the oracle's decoder, texture coordinate, material
    g0, g2, g3 = out["g0"], out["g2"], out["g3"]
    assert np.all(g0[:, 0] == (api.GBUFFER_DISPLACED | 2)) and np.all(g0[:, 1] == 7) and np.array_equal(g0[:, 2], hits["index"])
    assert np.abs((g0[:, 3] & 0xFFFF) / 65535.0 - hits["bcB"]).max() <= 1 / 65535 + 1e-7 and np.abs((g0[:, 3] >> 16) / 65535.0 - hits["bcC"]).max() <= 1 / 65535 + 1e-7
    assert np.array_equal(g2[:, :3], out["points"][:, :3].view(np.uint32))
    assert np.array_equal(g2[:, 3], g3[:, 0]), "geometric and shading normal are the same word"
    dec_n, dec_t = O.decode_normal(g3[:, 0]).astype(np.float64), O.decode_normal(g3[:, 1]).astype(np.float64)
    print("%s: decoded normal worst %.2e, tangent worst %.2e (step %.2e)" % (name, np.abs(dec_n - n64).max(), np.abs(dec_t - pts[:, 6:9]).max(), POLAR_STEP))
    assert np.abs(dec_n - n64).max() <= POLAR_STEP and np.abs(dec_t - pts[:, 6:9]).max() <= POLAR_STEP
    assert np.array_equal(dhost.decode_dir(g3[:, 0]), O.decode_normal(g3[:, 0])), "the header's decoder is the contract's"
    frac = pts[:, 9:11] - np.floor(pts[:, 9:11])
    assert np.abs((g3[:, 2] & 0xFFFF) / 65535.0 - frac[:, 0]).max() <= 1 / 65535 + 1e-6 and np.abs((g3[:, 2] >> 16) / 65535.0 - frac[:, 1]).max() <= 1 / 65535 + 1e-6
    assert np.all(g3[:, 3] == 3)
    # motion vector: the same camera a frame ago, rays through the pixel centres
    print("%s: motion vector worst %.2e pixel" % (name, np.abs(out["g1"]).max()))
    assert np.abs(out["g1"]).max() <= 5e-4
    moved = T.look_at_camera(W, H, (1.5, -3.5, 2.75), (0.5, 0.5, 0.0), fov_y_deg=40.0)
    g1_moved = dhost.resolve(table, hits, org, dirs, bv, geom, mat, xy, moved, W, H)["g1"]
    assert np.abs(g1_moved).min(0).max() > 0 and np.abs(g1_moved[:, 0]).mean() > 0.5, "a camera that moved sideways gives a flow"
    assert np.all(dhost.resolve(table, hits, org, dirs, bv, geom, mat, xy, moved, W, H, reset_flow=True)["g1"] == 0)


def test_both_fallbacks_are_taken(dhost, shost):
    L, tr = EXACT["non_uniform"]
    table = _record(shost, S.affine(L, tr))
    cam, hits, org, dirs, bv, xy = synthetic_hits(L, seed=21)
    n = 64
    hits, org, dirs, bv, xy = hits[:n].copy(), org[:n], dirs[:n], bv[:n].copy().reshape(n, 3, 5), xy[:n]
    # a normal that is not finite: +z and +x, whatever the tangent was
    hits["normal"][:16, 1] = np.nan
    hits["normal"][16:32] = 0.0
    hits["normal"][16:32, 0] = np.inf
    # a tangent that is not finite under a finite normal: texCoord0Dir zero, or parallel to the normal
    bv[32:48, :, :3] = 0.0
    axis = np.zeros((16, 3), np.float32)
    axis[np.arange(16), np.arange(16) % 3] = np.where(np.arange(16) % 2, -1.0, 1.0)
    hits["normal"][48:64] = axis
    bv[48:64, :, :3] = (axis.astype(np.float64) @ np.linalg.inv(np.asarray(L, np.float64)).T)[:, None, :]
    z = np.zeros(n, np.uint32)
    pts = dhost.resolve(table, hits, org, dirs, bv.reshape(n, 15), z, z, xy, cam, W, H)["points"]
    assert np.all(pts[:32, 3:6] == (0, 0, 1)) and np.all(pts[:32, 6:9] == (1, 0, 0))
    nn = pts[32:, 3:6].astype(np.float64)
    assert np.array_equal(pts[32:, 3:6], hits["normal"][32:])
    sign = np.where(nn[:, 2] >= 0, 1.0, -1.0)
    a = -1 / (sign + nn[:, 2])
    b = nn[:, 0] * nn[:, 1] * a
    want = np.stack([1 + sign * nn[:, 0] ** 2 * a, sign * b, -sign * nn[:, 0]], 1)       # makeCoordinateSystem, common_shared.h:92-100
    got = pts[32:, 6:9].astype(np.float64)
    assert np.all(np.isfinite(got)) and np.abs(got - want).max() <= 1e-6
    assert np.abs(np.linalg.norm(got, axis=1) - 1).max() <= 1e-6 and np.abs(np.sum(got * nn, 1)).max() <= 1e-6


def test_new_entries_are_declared_exported_and_listed(built_lib):
    import os
    header = open(os.path.join(T.ROOT, "include", "gfxexp.h")).read()
    for name in ("gfx_scene_bind_displaced", "gfx_restir_primary_rays"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name + " is not declared"
        assert hasattr(built_lib, name), name + " is not exported"
        assert name in api.C_ABI_SYMBOLS
    assert re.search(r"#define\s+GFX_GBUFFER_DISPLACED\s+0x80000000u", header)
    assert api.GBUFFER_DISPLACED == 0x80000000 and hasattr(api.Context, "bind_displaced") and hasattr(api.Context, "restir_primary_rays")
