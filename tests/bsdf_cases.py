"""Case lists of the shading layer (gfxexp_amd/csrc/shading.hip.h / oracle/orc_shared.h: BSDFs, hemisphere sampler, shading frame and
bump mapping, direct lighting), shared by tests/test_bsdf_cpu.py (the oracle against the float64 statement tests/bsdf_ref.py) and
tests/test_gpu_bsdf.py (the device, through gfx_bsdf_eval, against the oracle bit for bit).  Deterministic numpy: seeded default_rng
and explicit grids; every list holds at most 2^20 elements; lists are built once per process and must not be written to.

Two domains are kept apart.  INTERIOR lists hold unit directions with |cos| >= 1/16 on both sides and materials of roughness >= 1/16
(and, for the sampler, u1 at least 2^-12 away from the lobe boundary, where fp32 and float64 may pick different lobes): there the
oracle's values are held to measured bounds against float64.  EDGE lists hold everything else: grazing and degenerate directions,
near-mirror materials, the extreme random numbers, floats around every branch point.  They are held to structure (finite, non-negative,
zero where the model is zero) and, on the GPU, to parity.

A list is a dict(mat float32 [n, 8] | None, A float32 [n, 4] | None, B float32 [n, 4] | None, C float32 [n, 16] | None) in the layout of
gfx_bsdf_eval.  LISTS maps fn name (gfxexp_amd.api.BSDF_<name>) -> list name -> builder; oracle_words() gives the oracle's result."""
import functools

import numpy as np

from tests.math_cases import around, _frozen

F, U = np.float32, np.uint32
MIN_COS = 1.0 / 16
MIN_ROUGHNESS = 1.0 / 16
LOBE_MARGIN = 2.0 ** -12
N_RANDOM = 1 << 18
WORDS = {"SETUP": 7, "EVALUATE": 3, "PDF": 1, "SAMPLE": 7, "DHR": 3, "COSINE_HEMISPHERE": 5, "COORDINATE_SYSTEM": 6, "BUMP_FRAME": 15,
         "DIRECT_LIGHTING": 9}                              # result words each function returns; the rest of its planes are 0
ONE_M23, ONE_M24, ONE_M3_24 = 1 - 2.0 ** -23, 1 - 2.0 ** -24, 1 - 3 * 2.0 ** -24


# ---------------------------------------------------------------- materials
def _mat(t, a, b=(0, 0, 0), s=0.0):
    return [F(0)] + list(a) + list(b) + [s], t


def _materials(rows):
    m = np.array([r[0] for r in rows], F)
    m[:, 0] = np.array([r[1] for r in rows], U).view(F)
    return _frozen(m)


A0, B0 = (0.6, 0.5, 0.4), (0.04, 0.05, 0.06)
SMOOTHNESS = (-0.5, 0.0, 0.5, 0.6, 0.99, 0.999, 1.0, 1.5)


@functools.lru_cache(maxsize=None)
def materials_interior():
    """Roughness >= 1/16 (the roughness 1.5 of smoothness -0.5 included), colours in and above [0, 1], black lobes."""
    rows = [_mat(0, (0.8, 0.6, 0.4)), _mat(0, (0, 0, 0)), _mat(0, (1.5, 0.2, 2.0))]
    rows += [_mat(1, A0, B0, s) for s in SMOOTHNESS if 1 - min(s, 0.999) >= MIN_ROUGHNESS]
    rows += [_mat(1, (0, 0, 0), B0, 0.6), _mat(1, A0, (0, 0, 0), 0.6), _mat(1, (0, 0, 0), (0, 0, 0), 0.6), _mat(1, (1.5, 0.2, 2.0), B0, 0.6),
             _mat(1, A0, (1.25, 1.5, 0.9), 0.6)]
    rows += [_mat(2, (0.7, 0.5, 0.3), (1.0, r, m)) for r in (0.5, 1.0) for m in (0.0, 0.5, 1.0)]
    rows += [_mat(2, (0, 0, 0), (1.0, 0.5, 0.5)), _mat(2, (1.5, 0.2, 2.0), (1.0, 0.5, 0.5))]
    return _materials(rows)


@functools.lru_cache(maxsize=None)
def materials_edge():
    """Roughness below 1/16: both sides of the 0.999 clamp, roughness 0.001 of the metallic workflow."""
    rows = [_mat(1, A0, B0, s) for s in SMOOTHNESS if 1 - min(s, 0.999) < MIN_ROUGHNESS]
    rows += [_mat(1, (0, 0, 0), B0, 0.99), _mat(1, (0, 0, 0), (0, 0, 0), 1.0)]
    rows += [_mat(2, (0.7, 0.5, 0.3), (1.0, 0.0, m)) for m in (0.0, 0.5, 1.0)]
    return _materials(rows)


def materials_all():
    return _frozen(np.concatenate([materials_interior(), materials_edge()]))


def material_type(mat):
    return np.ascontiguousarray(mat[:, 0]).view(U).astype(np.int64)


def material_class(mat):
    """A short name per element, for reports: L, PBR, and for type 1 DS, DS-a0 (black diffuse), DS-b0 (black F0: the whole specular
    lobe is the ill-conditioned (1 - l.h)^5), DS-00 (both black), DS-r>1 (smoothness below 0: roughness above 1, where 1 - roughness
    is negative and the reflectance estimate cancels)."""
    t = material_type(mat)
    a0, b0 = ~np.any(mat[:, 1:4] != 0, axis=1), ~np.any(mat[:, 4:7] != 0, axis=1)
    ds = np.where(mat[:, 7] < 0, "DS-r>1", np.where(a0 & b0, "DS-00", np.where(a0, "DS-a0", np.where(b0, "DS-b0", "DS"))))
    return np.where(t == 0, "L", np.where(t == 2, "PBR", ds))


def _cycle(mats, n, shift=0):
    return mats[(np.arange(n) + shift) % len(mats)]


# ---------------------------------------------------------------- directions
def _unit(z, phi):
    s = np.sqrt(np.maximum(0.0, 1 - z * z))
    return np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1).astype(F)


def random_upper(rng, n, min_cos=MIN_COS):
    """Unit directions (to fp32 rounding) of the upper hemisphere, uniform in cos on [min_cos, 1]."""
    z = rng.uniform(min_cos, 1.0, n)
    v = _unit(z, rng.uniform(0, 2 * np.pi, n))
    v[:, 2] = np.maximum(v[:, 2], F(min_cos))
    return v


def a4(v):
    v = np.asarray(v, F)
    out = np.zeros((len(v), 4), F)
    out[:, :v.shape[1]] = v
    return out


@functools.lru_cache(maxsize=None)
def direction_pairs():
    """2^18 random pairs (vGiven, vSampled) of the upper hemisphere, both cosines >= 1/16."""
    rng = np.random.default_rng(20261)
    return _frozen(random_upper(rng, N_RANDOM)), _frozen(random_upper(rng, N_RANDOM))


@functools.lru_cache(maxsize=None)
def edge_directions():
    """View directions outside the interior: normal incidence, grazing z in {+0, -0, 2^-24, 1e-6, 1e-3} and their negatives, below the
    1/16 cosine, non-unit, zero and NaN vectors."""
    rows = [(0, 0, 1), (0, 0, -1), (1e-4, 0, 1), (0, -1e-3, 1)]
    for z in (0.0, -0.0, 2.0 ** -24, 1e-6, 1e-3, -2.0 ** -24, -1e-3, 0.03, 0.06):
        for phi in (0.0, 2.0, 4.5):
            s = np.sqrt(1 - z * z)
            rows.append((s * np.cos(phi), s * np.sin(phi), z))
    rows += [(0, 0, 0), (-0.0, 0.0, -0.0), (0.3, 0.4, 2.0), (3.0, -4.0, 0.5), (1e-20, 0, 1e-20), (np.nan, 0, 1), (0, 0, np.nan), (0.6, np.nan, 0.8),
             (np.inf, 0, 1)]
    return _frozen(np.array(rows, F))


def _cross_lists(*arrays):
    """All combinations of the rows of the given arrays, as a tuple of arrays of equal length."""
    idx = np.meshgrid(*[np.arange(len(a)) for a in arrays], indexing="ij")
    return tuple(a[i.ravel()] for a, i in zip(arrays, idx))


def _case(mat=None, A=None, B=None, C=None):
    d = dict(mat=None if mat is None else _frozen(np.asarray(mat, F)), A=None if A is None else _frozen(a4(A)),
             B=None if B is None else _frozen(a4(B)), C=None if C is None else _frozen(np.asarray(C, F)))
    n = [len(x) for x in d.values() if x is not None]
    assert len(set(n)) == 1 and 0 < n[0] <= 1 << 20, n
    return d


# ---------------------------------------------------------------- EVALUATE / PDF / DHR
@functools.lru_cache(maxsize=None)
def pairs_interior():
    """The random pairs four times: as they are, vGiven flipped, vSampled flipped, both flipped below the surface (2^20 elements)."""
    g, s = direction_pairs()
    vg = np.concatenate([g, -g, g, -g])
    vs = np.concatenate([s, s, -s, -s])
    return _case(_cycle(materials_interior(), len(vg)), vg, vs)


@functools.lru_cache(maxsize=None)
def pairs_edge():
    """Every material with: every edge direction against a fixed and a mirrored partner and against itself; exact mirror pairs and
    vGiven == vSampled of interior directions; then the first 2^16 random pairs with the edge materials."""
    e = edge_directions()
    g, s = direction_pairs()
    g, s = g[:64], s[:64]
    mirror = g * np.array([-1, -1, 1], F)
    vg = np.concatenate([e, e, e, e, g, g, -g, g[:16]])
    vs = np.concatenate([np.tile(np.array([[0.36, 0.48, 0.8]], F), (len(e), 1)), e * np.array([-1, -1, 1], F), e, -e, mirror, g, -g,
                         np.tile(np.array([[0, 0, 1]], F), (16, 1))])
    m, i = _cross_lists(materials_all(), np.arange(len(vg)))
    g2, s2 = direction_pairs()
    k = 1 << 16
    flips = np.where(np.arange(k) % 3 == 2, -1, 1).astype(F)[:, None]
    return _case(np.concatenate([m, _cycle(materials_edge(), k)]), np.concatenate([vg[i], g2[:k] * flips]), np.concatenate([vs[i], s2[:k] * flips]))


def dhr_interior():
    c = pairs_interior()
    return _case(c["mat"][:1 << 19], c["A"][:1 << 19])


def dhr_edge():
    c = pairs_edge()
    return _case(c["mat"], c["A"])


# ---------------------------------------------------------------- SAMPLE
def _lobe_split(mat, vg):
    """wDiff / sumW of the model (float64) per element; NaN for Lambert."""
    from tests import bsdf_ref as R
    d, f0, r = R.setup(material_type(mat), mat[:, 1:4], mat[:, 4:7], mat[:, 7])
    wd, ws = R.lobe_weights(d, f0, r, vg.astype(np.float64))
    with np.errstate(all="ignore"):
        return np.where(material_type(mat) == 0, np.nan, wd / (wd + ws)), d, f0, r


@functools.lru_cache(maxsize=None)
def sample_interior():
    """2^18 random view directions (|cos| >= 1/16, every fourth below the surface) with random (u0, u1) and the interior materials; an
    element whose u1 lies within 2^-12 of the lobe boundary wDiff / sumW gets u1 moved 2^-11 away from it."""
    rng = np.random.default_rng(20262)
    vg = random_upper(rng, N_RANDOM)
    vg[3::4] *= -1
    u = rng.random((N_RANDOM, 2), F)
    mat = _cycle(materials_interior(), N_RANDOM)
    split = _lobe_split(mat, vg)[0]
    near = np.abs(u[:, 1].astype(np.float64) - split) < LOBE_MARGIN
    u[near, 1] = np.where(split[near] > 0.5, split[near] - 2 * LOBE_MARGIN, split[near] + 2 * LOBE_MARGIN).astype(F)
    assert np.all((u >= 0) & (u < 1))
    return _case(mat, vg, u)


def stratified_grid(seed=20263, k=1024):
    """k x k strata of the unit square, one jittered point in each: float32 [k^2, 2], all < 1."""
    rng = np.random.default_rng(seed)
    j, i = np.meshgrid(np.arange(k), np.arange(k), indexing="ij")
    u = (np.stack([i.ravel(), j.ravel()], axis=1) + rng.random((k * k, 2))) / k
    return np.minimum(u.astype(F), F(ONE_M24))


HISTOGRAM_VIEW_COS = (1.0, 0.5, MIN_COS)


def view_of_cos(c):
    return np.array([np.sqrt(1 - c * c) * 0.6, np.sqrt(1 - c * c) * 0.8, c], F)


@functools.lru_cache(maxsize=None)
def sample_grid():
    """The 1024 x 1024 stratified grid, materials and the three histogram view cosines cycling over it."""
    u = stratified_grid()
    views = np.stack([view_of_cos(c) for c in HISTOGRAM_VIEW_COS])
    return _case(_cycle(materials_all(), len(u)), views[(np.arange(len(u)) // 7) % 3], u)


U0_EDGE = np.array([0.0, 2.0 ** -23, ONE_M23, ONE_M24, ONE_M3_24, 0.5], F)
U1_EDGE = np.array([0.0, ONE_M23, ONE_M24, 0.5], F)


@functools.lru_cache(maxsize=None)
def u0_edge_views():
    """Unit view directions with z > 0 for the u0 / u1 edge list: z from 1 to 0.01, and 25 random ones."""
    rng = np.random.default_rng(20264)
    fixed = np.stack([view_of_cos(c) for c in (1.0, 0.9, 0.5, 0.3, MIN_COS, 0.01)])
    return _frozen(np.concatenate([fixed, random_upper(rng, 25, 0.01)]))


@functools.lru_cache(maxsize=None)
def sample_u_edge():
    """Every material x the u0-edge views x u0 in {0, 2^-23, 1 - 2^-23, 1 - 2^-24, 1 - 3 2^-24, 0.5} x 193 values of u1: {0, 1 - 2^-23,
    1 - 2^-24, 0.5} and a ramp.  All view directions are unit with z > 0: no result of this list may be NaN."""
    u1 = np.concatenate([U1_EDGE, np.linspace(0, 1, 189, endpoint=False).astype(F)])
    m, v, a, b = _cross_lists(materials_all(), u0_edge_views(), U0_EDGE, u1)
    return _case(m, v, np.stack([a, b], axis=1))


@functools.lru_cache(maxsize=None)
def sample_u0_top():
    """The two largest u0 (1 - 2^-23, the largest value of the passes' generator, and 1 - 2^-24) against 2^17 random u1 each, for the
    type 1 material of smoothness 0.6 at view cosines 1, 0.3 and 0.01: sqrt(u0) rounds to 1 or 1 - 2^-24 there and the radicand
    1 - P1^2 - P2^2 of the visible-normal sampler comes out negative for about one u1 in 10^4.  No result may be NaN."""
    rng = np.random.default_rng(20271)
    k = 1 << 17
    mat = materials_interior()[material_type(materials_interior()) == 1][3:4]
    assert mat[0, 7] == F(0.6)
    views = np.stack([view_of_cos(c) for c in (1.0, 0.3, 0.01)])
    v, u0, u1 = _cross_lists(views, np.array([ONE_M23, ONE_M24], F), rng.random(k, F))
    return _case(np.tile(mat, (len(v), 1)), v, np.stack([u0, u1], axis=1))


@functools.lru_cache(maxsize=None)
def sample_branch_edge():
    """Floats around the sampler's own branch points, for each material x view direction of a small grid:
    u1 +-64 floats around the lobe boundary wDiff / sumW; u1 +-64 floats around the value that the lobe remap takes to
    a = 1 / (1 + sv.z) inside ggx_sample (exact for materials without a diffuse lobe, where the remap is the identity);
    (u0, u1) on the four diagonals sx = +-sy of the disk map, +-4 floats; the disk's centre."""
    views = np.stack([view_of_cos(c) for c in (1.0, 0.999, 0.7, 0.3, MIN_COS, 0.01)] + [-view_of_cos(0.5)])
    m, v = _cross_lists(materials_all(), views)
    split, d, f0, r = _lobe_split(m, v)
    ok = np.isfinite(split)
    alpha = r ** 2
    sv = v.astype(np.float64) * np.sign(v[:, 2:3]).astype(np.float64) * np.stack([alpha, alpha, np.ones_like(alpha)], axis=1)
    a = 1 / (1 + sv[:, 2] / np.sqrt(np.sum(sv * sv, axis=1)))
    at_a = split + a * (1 - split)
    rows_m, rows_v, rows_u = [], [], []
    for centre in (split, at_a):
        for i in np.flatnonzero(ok & (centre > 0) & (centre < 1)):
            u1 = around([centre[i]], 64)
            u1 = u1[(u1 >= 0) & (u1 < 1)]
            for u0 in (0.25, ONE_M24):
                rows_m.append(np.tile(m[i], (len(u1), 1))); rows_v.append(np.tile(v[i], (len(u1), 1)))
                rows_u.append(np.stack([np.full(len(u1), u0, F), u1], axis=1))
    t = around([0.1, 0.25, 0.4, 0.5, 0.6, 0.75, 0.9], 4)
    t = t[(t >= 0) & (t < 1)]
    diag = np.concatenate([np.stack([t, t], axis=1), np.stack([t, (F(1) - t).astype(F)], axis=1), np.array([[0.5, 0.5]], F)])
    i, du = _cross_lists(np.arange(0, len(m), 3), diag)
    rows_m.append(m[i]); rows_v.append(v[i]); rows_u.append(du)
    return _case(np.concatenate(rows_m), np.concatenate(rows_v), np.concatenate(rows_u))


@functools.lru_cache(maxsize=None)
def sample_direction_edge():
    """Every material x every edge view direction (exactly grazing, non-unit, zero, NaN, normal incidence: the T1 = (1, 0, 0) branch) and
    near-normal views that small alpha stretches past sv.z >= 0.9999, x a 5 x 5 set of (u0, u1)."""
    near_normal = np.stack([view_of_cos(c) for c in (0.99995, 0.9999, 0.999, 0.99, 0.9)])
    u = np.array([0.0, 0.3, 0.5, 0.77, ONE_M24], F)
    m, v, a, b = _cross_lists(materials_all(), np.concatenate([edge_directions(), near_normal]), u, u)
    return _case(m, v, np.stack([a, b], axis=1))


# ---------------------------------------------------------------- COSINE_HEMISPHERE
def hemisphere_grid():
    return _case(A=stratified_grid(20265))


def hemisphere_edge():
    """u0, u1 in {0, 2^-23, 0.5, 1 - 2^-23, 1 - 2^-24, 1 - 3 2^-24} crossed; the disk's centre; the four diagonals +-4 floats."""
    e = np.array([0.0, 2.0 ** -23, 0.25, 0.5, 0.75, ONE_M23, ONE_M24, ONE_M3_24], F)
    a, b = _cross_lists(e, e)
    t = around(np.linspace(0.01, 0.99, 99), 4)
    t = t[(t >= 0) & (t < 1)]
    diag = np.concatenate([np.stack([t, t], axis=1), np.stack([t, (F(1) - t).astype(F)], axis=1)])
    return _case(A=np.concatenate([np.stack([a, b], axis=1), np.array([[0.5, 0.5]], F), diag]))


# ---------------------------------------------------------------- COORDINATE_SYSTEM / BUMP_FRAME
@functools.lru_cache(maxsize=None)
def random_normals():
    rng = np.random.default_rng(20266)
    v = rng.standard_normal((N_RANDOM, 3))
    return _frozen((v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F))


def normals_random():
    return _case(A=random_normals())


def normals_edge():
    """The axes with every sign of zero; unit normals with z +-64 floats around 0 and around -1 (z = -1 itself: the basis's pole)."""
    z0 = [0.0, -0.0]
    rows = [(sx * 1.0, y, z) for sx in (1, -1) for y in z0 for z in z0] + [(x, sy * 1.0, z) for sy in (1, -1) for x in z0 for z in z0] + \
           [(x, y, sz * 1.0) for sz in (1, -1) for x in z0 for y in z0]
    z = np.concatenate([around([0.0], 64), around([-1.0], 64)]).astype(np.float64)
    z = z[z >= -1]
    s = np.sqrt(np.maximum(0.0, 1 - z * z))
    ring = np.concatenate([np.stack([s * 0.6, s * 0.8, z], axis=1), np.stack([s, 0 * s, z], axis=1)])
    return _case(A=np.concatenate([np.array(rows, F), ring.astype(F)]))


def _frames(n, seed):
    """Unit normals with an orthogonal unit tangent (float64 Gram-Schmidt, rounded to fp32)."""
    rng = np.random.default_rng(seed)
    nrm = rng.standard_normal((n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    t = rng.standard_normal((n, 3))
    t -= nrm * np.sum(nrm * t, axis=1, keepdims=True)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    return nrm.astype(F), t.astype(F)


def _c16(*vecs):
    c = np.zeros((len(vecs[0]), 16), F)
    for k, v in enumerate(vecs):
        c[:, 4 * k:4 * k + v.shape[1]] = v
    return c


@functools.lru_cache(maxsize=None)
def bump_interior():
    """2^18 random frames, unit modified normals with z >= 1/16 and a tilt |(x, y)| >= 1/64, unit probe vectors."""
    n = N_RANDOM
    nrm, t = _frames(n, 20267)
    rng = np.random.default_rng(20268)
    mod = random_upper(rng, n, MIN_COS)
    flat = np.hypot(mod[:, 0], mod[:, 1]) < 1.0 / 64
    mod[flat] = np.array([0.6, 0, 0.8], F)
    return _case(A=nrm, B=t, C=_c16(mod, random_normals()))


@functools.lru_cache(maxsize=None)
def bump_edge():
    """Modified normals outside the interior, each in 8 frames: tilt projLength +-64 floats around 1e-3; z = 0, z < 0 and z = -0; the
    untextured (0, 0, 1); unnormalised 8-bit texel values 2 t - 1 (a 16 x 16 x 4 subgrid); the two-channel case with x^2 + y^2 > 1, whose
    z is NaN by construction; zero and NaN vectors."""
    p = around([1e-3], 64).astype(np.float64)
    rows = [np.stack([p, 0 * p, 1 + 0 * p], axis=1), np.stack([p * 0.6, p * 0.8, 0.5 + 0 * p], axis=1)]
    rows.append(np.array([(0.3, 0.4, 0.0), (0.3, 0.4, -0.0), (0.3, -0.4, -0.5), (0, 0, 1), (0, 0, -1), (1, 0, 0), (0, 0, 0), (0.9, 0.8, np.nan),
                          (np.nan, 0, 1), (1e-3, 0, 1), (0, 1e-3, 1e-3)]))
    t = (np.arange(0, 256, 17) / 255.0).astype(F)
    tz = (np.array([0, 127, 128, 255]) / 255.0).astype(F)
    x, y, z = _cross_lists(t, t, tz)
    rows.append(np.stack([F(2) * x - F(1), F(2) * y - F(1), F(2) * z - F(1)], axis=1))
    mod = np.concatenate([np.asarray(r, np.float64) for r in rows]).astype(F)
    nrm, tg = _frames(8, 20269)
    nrm[0], tg[0] = (0, 0, 1), (1, 0, 0)
    m, i = _cross_lists(mod, np.arange(8))
    return _case(A=nrm[i], B=tg[i], C=_c16(m, _cycle(random_normals(), len(m))))


# ---------------------------------------------------------------- DIRECT_LIGHTING
def _lighting(n, seed, mats, edge):
    rng = np.random.default_rng(seed)
    nrm, t = _frames(n, seed + 1)
    point = rng.uniform(-2, 2, (n, 3)).astype(F)
    v_out = random_upper(rng, n)
    # a light 0.5 to 4 away, in a direction with cosine >= 1/16 against the frame's normal, turned toward the shading point
    w_local = random_upper(rng, n).astype(np.float64)
    b = np.cross(nrm.astype(np.float64), t.astype(np.float64))
    w = w_local[:, 0:1] * t + w_local[:, 1:2] * b + w_local[:, 2:3] * nrm
    dist = rng.uniform(0.5, 4.0, (n, 1))
    pos = (point + w * dist).astype(F)
    tilt = random_upper(rng, n, 0.25).astype(np.float64)
    tn, tb = _frames(n, seed + 2)
    ln = -w * tilt[:, 2:3] + 0.2 * tilt[:, 0:1] * tn                        # roughly facing; normalised below
    ln = (ln / np.linalg.norm(ln, axis=1, keepdims=True)).astype(F)
    emit = rng.uniform(0, 20, (n, 3)).astype(F)
    inf = np.zeros(n, U)
    if edge:
        k = np.arange(n) % 8
        ln[k == 1] *= -1                                                   # the light seen from behind its own normal: 0
        pos[k == 2] = (point.astype(np.float64) - (w * dist))[k == 2].astype(F)   # the light behind the surface: the BSDF is 0
        inf[k == 3] = 1                                                    # at infinity: the position is the direction
        pos[k == 3] = w[k == 3].astype(F)
        ln[k == 3] = -pos[k == 3]
        pos[k == 4] = point[k == 4]                                        # the light at the shading point: dist2 == 0
        v_out[k == 5] *= -1                                                # seen from below
        inf[k == 6] = 1                                                    # at infinity with an unnormalised direction
        v_out[k == 7] = edge_directions()[np.arange(np.count_nonzero(k == 7)) % len(edge_directions())]
    c = _c16(nrm, t, emit, pos)
    c[:, 3], c[:, 7], c[:, 11] = ln[:, 0], ln[:, 1], ln[:, 2]
    c[:, 15] = inf.view(F)
    return _case(_cycle(mats, n), point, v_out, c)


@functools.lru_cache(maxsize=None)
def lighting_interior():
    return _lighting(N_RANDOM, 20270, materials_interior(), False)


@functools.lru_cache(maxsize=None)
def lighting_edge():
    return _lighting(1 << 16, 20280, materials_all(), True)


def setup_materials():
    return _case(materials_all())


LISTS = {
    "SETUP": {"materials": setup_materials},
    "EVALUATE": {"interior": pairs_interior, "edge": pairs_edge},
    "PDF": {"interior": pairs_interior, "edge": pairs_edge},
    "SAMPLE": {"interior": sample_interior, "grid": sample_grid, "u-edge": sample_u_edge, "u0-top": sample_u0_top, "branch-edge": sample_branch_edge,
               "direction-edge": sample_direction_edge},
    "DHR": {"interior": dhr_interior, "edge": dhr_edge},
    "COSINE_HEMISPHERE": {"grid": hemisphere_grid, "edge": hemisphere_edge},
    "COORDINATE_SYSTEM": {"random": normals_random, "edge": normals_edge},
    "BUMP_FRAME": {"interior": bump_interior, "edge": bump_edge},
    "DIRECT_LIGHTING": {"interior": lighting_interior, "edge": lighting_edge},
}

# NaN words the oracle returns per list (all result words of all elements), recorded by tests/test_bsdf_cpu.py
# (test_nan_words_are_the_recorded_ones); the device must return NaN in exactly as many words, in the same places.
NAN_WORDS = {
    ("SETUP", "materials"): 0, ("EVALUATE", "interior"): 0, ("EVALUATE", "edge"): 1014, ("PDF", "interior"): 0, ("PDF", "edge"): 1952,
    ("SAMPLE", "interior"): 0, ("SAMPLE", "grid"): 0, ("SAMPLE", "u-edge"): 0, ("SAMPLE", "u0-top"): 0, ("SAMPLE", "branch-edge"): 0,
    ("SAMPLE", "direction-edge"): 26313, ("DHR", "interior"): 0, ("DHR", "edge"): 0, ("COSINE_HEMISPHERE", "grid"): 0,
    ("COSINE_HEMISPHERE", "edge"): 0, ("COORDINATE_SYSTEM", "random"): 0, ("COORDINATE_SYSTEM", "edge"): 0, ("BUMP_FRAME", "interior"): 0,
    ("BUMP_FRAME", "edge"): 240, ("DIRECT_LIGHTING", "interior"): 0, ("DIRECT_LIGHTING", "edge"): 27500,
}


def oracle_out(fn, c):
    """The oracle's results for list c as float32 [n, WORDS[fn]]."""
    from oracle import oracle as O
    x3 = lambda a: None if a is None else np.ascontiguousarray(a[:, :3])
    if fn in ("SETUP", "EVALUATE", "PDF", "SAMPLE", "DHR"):
        mode = {"EVALUATE": 0, "PDF": 1, "SAMPLE": 2, "DHR": 3, "SETUP": 4}[fn]
        return np.ascontiguousarray(O.bsdf_eval_materials(c["mat"], mode, x3(c["A"]), x3(c["B"]))[:, :WORDS[fn]])
    if fn == "COSINE_HEMISPHERE":
        return O.cosine_hemisphere(np.ascontiguousarray(c["A"][:, :2]))
    if fn == "COORDINATE_SYSTEM":
        return O.coordinate_system(x3(c["A"]))
    C = c["C"]
    if fn == "BUMP_FRAME":
        return O.bump_frame(x3(c["A"]), x3(c["B"]), C[:, 0:3], C[:, 4:7])
    if fn == "DIRECT_LIGHTING":
        light = np.concatenate([C[:, 8:11], C[:, 12:15], C[:, [3, 7, 11]]], axis=1)
        return O.direct_lighting(c["mat"], x3(c["A"]), x3(c["B"]), C[:, 0:3], C[:, 4:7], light, np.ascontiguousarray(C[:, 15]).view(U))
    raise KeyError(fn)


def oracle_words(fn, c):
    """The oracle's result as the planes of gfx_bsdf_eval: uint32 [WORDS[fn], n]."""
    return np.ascontiguousarray(oracle_out(fn, c).T).view(U)


def nan_words(words):
    return int(np.count_nonzero(np.isnan(np.ascontiguousarray(words).view(F))))
