"""Case lists of the deterministic math contract (gm_math.hip.h / oracle/orc_math.h, contract version 1) and of the 16-bit
quantisers on top of it (shading.hip.h / oracle/orc_shared.h), shared by tests/test_math_contract_cpu.py (the oracle copy against
float64) and tests/test_gpu_math_contract.py (the device copy against the oracle, bit for bit).  Deterministic numpy with fixed
seeds; every list holds at most 2^24 elements; the lists are built once per process and must not be written to.

GPU_LISTS names, per function of gfx_math_eval, the lists the device is compared on, and oracle_words() gives the oracle's result
words for one of them.  Two kinds of input are left out of the parity lists because the host code has no defined result for them
(static_cast<int32_t> of an out-of-range float): gm_exp outside [EXP_MIN, EXP_MAX] (NaN included), and gm_sincos at
|x| >= 2^31 pi/2, where the quadrant no longer fits 32 bits."""
import functools

import numpy as np

F = np.float32
U = np.uint32
FLT_MIN = float(np.finfo(F).tiny)
FLT_MAX = float(np.finfo(F).max)


def f32_from_bits(b):
    return np.asarray(b, dtype=np.uint32).view(F)


# ---------------------------------------------------------------- the contract's domain ends, as fp32 constants (both headers)
EXP_MIN = float(f32_from_bits([0xC2AF5DC2])[0])          # -87.68312: the smallest x at which gm_exp scales by 2^-126; below it the result is 0
EXP_NORMAL_MIN = float(f32_from_bits([0xC2AEAC4F])[0])   # -87.33654: the smallest x with a normal result; [EXP_MIN, this) gives subnormals
EXP_MAX = float(f32_from_bits([0x42B0C0A5])[0])          # 88.37626: the largest x at which gm_exp scales by 2^127; above it the result is +inf
SINCOS_ULP_MAX = 1.0e4                                   # |x| up to which gm_sincos is held to an ulp bound
SINCOS_ABS_MAX = 1.0e6                                   # ... and to an absolute bound
SINCOS_PARITY_MAX = float(F(2.0 ** 31 * np.pi / 2))      # quadrant index q = rint(x 2/pi) reaches 2^31
TAN_ULP_MAX = 1.5


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _ordinal(x):
    b = np.ascontiguousarray(x, F).view(U).astype(np.int64)
    return np.where(b & 0x80000000, -(b & 0x7FFFFFFF), b)


def _from_ordinal(o):
    o = np.clip(o, -0x7F800000, 0x7F800000)              # stop at the infinities
    return np.where(o < 0, 0x80000000 | (-o), o).astype(U).view(F)


def around(values, k):
    """The 2 k + 1 consecutive floats centred on each value (float64 values are rounded to fp32 first)."""
    v = np.asarray(values, np.float64).astype(F).ravel()
    return _from_ordinal((_ordinal(v)[:, None] + np.arange(-k, k + 1)[None, :]).ravel())


# ---------------------------------------------------------------- unary functions
@functools.lru_cache(maxsize=None)
def unary_strided():
    """Every 257th fp32 bit pattern over all 2^32: +0, subnormals, normals and NaNs of both signs (-0 and the infinities
    themselves are in unary_edges)."""
    return _frozen(np.arange(0, 2 ** 32, 257, dtype=np.uint64).astype(U).view(F))


@functools.lru_cache(maxsize=None)
def unary_edges():
    """+-64 consecutive floats around every point at which a contract function switches branch, and all inputs with a subnormal
    gm_exp result."""
    ks = np.unique(np.concatenate([np.arange(0, 65), np.arange(0, 2 ** 16 + 1, 16)])).astype(np.float64)
    quadrants = ks * (np.pi / 2)                                        # quadrant switch, and between two of them the rintf tie
    ties = (ks[:-1] + 0.5) * (np.pi / 2)
    ln2 = (np.arange(-127, 129) + 0.5) * np.log(2.0)                    # floorf(x log2e + 1/2) switch of gm_exp
    exp_pts = [np.log(FLT_MIN), np.log(FLT_MAX), EXP_MIN, EXP_NORMAL_MIN, EXP_MAX, -87.5, 80.0, -80.0]
    acos_pts = [0.5, -0.5, 1.0, -1.0]
    atan_pts = [np.tan(np.pi / 8), np.tan(3 * np.pi / 8), 1.0, -np.tan(np.pi / 8), -np.tan(3 * np.pi / 8), -1.0]
    sat_pts = [2.0 ** 31, -2.0 ** 31, 2.0 ** 32, 0.0, 65535.5 / 65535, 1.0 / 65535, 0.5 / 65535, float(F(SINCOS_PARITY_MAX)), SINCOS_ULP_MAX,
               SINCOS_ABS_MAX, TAN_ULP_MAX, FLT_MIN, -FLT_MIN]
    pts = np.concatenate([quadrants, -quadrants, ties, -ties, ln2, exp_pts, acos_pts, atan_pts, sat_pts, -np.asarray(sat_pts)])
    lo, hi = _ordinal(np.array([EXP_MIN, EXP_NORMAL_MIN], F))           # negative: lo is the smaller ordinal
    subnormal_results = _from_ordinal(np.arange(lo, hi + 1))
    special = np.array([-0.0, 0.0, np.inf, -np.inf, np.nan], F)
    return _frozen(np.concatenate([around(pts, 64), subnormal_results, special]))


UNARY_LISTS = {"strided": unary_strided, "edges": unary_edges}


# ---------------------------------------------------------------- gm_atan2
ATAN2_SPECIAL_VALUES = np.array([0.0, -0.0, 1.0, -1.0, FLT_MIN, -FLT_MIN, 1e-45, -1e-45, 3e38, -3e38, np.inf, -np.inf, np.nan], F)


def atan2_special():
    """(y, x): the full cross product of ATAN2_SPECIAL_VALUES, y-major."""
    y, x = np.meshgrid(ATAN2_SPECIAL_VALUES, ATAN2_SPECIAL_VALUES, indexing="ij")
    return _frozen(np.stack([y.ravel(), x.ravel()], axis=1))


def _random_finite(rng, n):
    return ((rng.integers(0, 2, n, dtype=np.uint64) << 31) | (rng.integers(0, 255, n, dtype=np.uint64) << 23) | rng.integers(0, 1 << 23, n, dtype=np.uint64)).astype(U).view(F)


@functools.lru_cache(maxsize=None)
def atan2_pairs():
    """(y, x) pairs: the special cross product, 4 M random finite bit patterns (their ratio underflows and overflows), 1 M points
    of the unit circle, and +-8 floats in either component around the axes and the diagonals at three scales."""
    rng = np.random.default_rng(20240611)
    n = 4 << 20
    random_pairs = np.stack([_random_finite(rng, n), _random_finite(rng, n)], axis=1)
    t = rng.uniform(0.0, 2 * np.pi, 1 << 20)
    circle = np.stack([np.sin(t), np.cos(t)], axis=1).astype(F)
    near = []
    for scale in (1.0, FLT_MIN * 4, 1e30):
        for y0, x0 in ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1)):
            ys = around([y0 * scale], 8) if y0 else np.concatenate([around([0.0], 8), np.array([-0.0], F)])
            xs = around([x0 * scale], 8) if x0 else np.concatenate([around([0.0], 8), np.array([-0.0], F)])
            yy, xx = np.meshgrid(ys, xs, indexing="ij")
            near.append(np.stack([yy.ravel(), xx.ravel()], axis=1))
    return _frozen(np.concatenate([atan2_special(), random_pairs, circle] + near))


# ---------------------------------------------------------------- directions (to_polar_yup / encode_dir)
def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


@functools.lru_cache(maxsize=None)
def directions():
    """Named lists of float32 [n, 3].  `random`, `axes`, `seam` and `poles` are unit vectors (to rounding) and round-trip through
    the quantiser; `non_unit` exercises the clamp of v.y and `nan` holds one NaN per component."""
    rng = np.random.default_rng(20240612)
    random = _unit(rng.normal(size=(2 << 20, 3)))
    axes = []
    for axis in range(3):
        for sign in (1.0, -1.0):
            for za in (0.0, -0.0):
                for zb in (0.0, -0.0):
                    v = [za, zb]
                    v.insert(axis, sign)
                    axes.append(v)
    seam = []
    for vy in (0.0, 0.5, -0.7, 0.999):
        for zs in (1.0, -1.0):                                           # v.z > 0: phi wraps 2 pi -> 0; v.z < 0: phi = pi
            vz = zs * np.sqrt(1.0 - vy * vy)
            xs = np.concatenate([around([0.0, 1e-8, -1e-8], 8), np.array([-0.0], F)])
            for vx in xs:
                seam.append([vx, vy, vz])
    poles, beyond = [], []
    for ys in (1.0, -1.0):
        for vy in around([ys], 8).astype(np.float64):
            rad = np.sqrt(max(0.0, 1.0 - vy * vy))                      # up to 1e-3: theta within a few codes of the pole
            for cx, cz in ((0.0, 1.0), (-0.0, 1.0), (0.0, -1.0), (-0.0, -1.0), (1.0, 0.0), (-1.0, -0.0), (0.6, 0.8), (-0.8, -0.6)):
                (poles if abs(vy) <= 1.0 else beyond).append([cx * rad, vy, cz * rad])
            if abs(vy) <= 1.0:
                poles.append([1e-45, vy, rad])
                poles.append([-1e-45, vy, -rad])
    scale = rng.uniform(0.0, 4.0, (1 << 16, 1))
    non_unit = (_unit(rng.normal(size=(1 << 16, 3))).astype(np.float64) * scale).astype(F)
    non_unit = np.concatenate([non_unit, np.array(beyond, F), np.array([[0, 4, 0], [0, -4, 0], [0.5, 1.0000001, 0.5], [3, -1.0000001, -2], [0, 0, 0], [-0.0, -0.0, -0.0]], F)])
    nan = np.array([[np.nan, 0.6, 0.8], [0.6, np.nan, 0.8], [0.6, 0.8, np.nan]], F)
    return {"random": _frozen(random), "axes": _frozen(np.array(axes, F)), "seam": _frozen(np.array(seam, F)), "poles": _frozen(np.array(poles, F)),
            "non_unit": _frozen(non_unit), "nan": _frozen(nan)}


UNIT_DIRECTION_LISTS = ("random", "axes", "seam", "poles")


def all_directions():
    d = directions()
    return _frozen(np.concatenate([d[k] for k in ("random", "axes", "seam", "poles", "non_unit", "nan")]))


# ---------------------------------------------------------------- decode_dir
THETA_EDGE_CODES = (0, 1, 2, 32767, 32768, 65533, 65534, 65535)


@functools.lru_cache(maxsize=None)
def dir_codes_edges():
    """Every phi code for the theta codes at the poles and the equator."""
    th = np.array(THETA_EDGE_CODES, U)
    return _frozen(((th[:, None] << 16) | np.arange(65536, dtype=U)[None, :]).ravel())


@functools.lru_cache(maxsize=None)
def dir_codes_grid():
    """Every 257th theta code (0, 257, ..., 65535) against every phi code: 2^24 codes."""
    th = np.arange(0, 65536, 257, dtype=U)
    return _frozen(((th[:, None] << 16) | np.arange(65536, dtype=U)[None, :]).ravel())


# ---------------------------------------------------------------- encode_uv / encode_bc
@functools.lru_cache(maxsize=None)
def unorm_values():
    """Random values in +-8, the integers in +-8 with their neighbours, k / 65535 and (k + 1/2) / 65535 for every k (a code, and the
    middle of its cell), -0 and NaN."""
    rng = np.random.default_rng(20240613)
    k = np.arange(65536, dtype=np.float64)
    return _frozen(np.concatenate([rng.uniform(-8.0, 8.0, 1 << 20).astype(F), around(np.arange(-8, 9), 1), (k / 65535).astype(F), ((k + 0.5) / 65535).astype(F),
                                   np.array([-0.0, np.nan, np.inf, -np.inf], F)]))


@functools.lru_cache(maxsize=None)
def uv_pairs():
    """(u, v): unorm_values() against itself in another order, so that both halves of the code see every value."""
    u = unorm_values()
    return _frozen(np.stack([u, np.roll(u[::-1], 12345)], axis=1))


@functools.lru_cache(maxsize=None)
def uv_codes():
    """Codes of decode_uv / decode_bc: every value of either half against a scrambled other half."""
    k = np.arange(65536, dtype=np.uint64)
    return _frozen(np.concatenate([(k | (((k * 40503) & 0xFFFF) << 16)), ((k << 16) | ((k * 40503) & 0xFFFF))]).astype(U))


# ---------------------------------------------------------------- offset_ray_origin
@functools.lru_cache(maxsize=None)
def offset_cases():
    """(p, n): points over seven decades around the 1/32 switch between the float and the integer offset (and on it, with
    neighbours), normals of length up to 4.  The integer offset stays far from overflowing the bit pattern of p."""
    rng = np.random.default_rng(20240614)
    m = 1 << 18
    p = (rng.normal(size=(m, 3)) * 10.0 ** rng.uniform(-4, 3, (m, 1))).astype(F)
    n = (_unit(rng.normal(size=(m, 3))).astype(np.float64) * rng.uniform(0.25, 4.0, (m, 1))).astype(F)
    edge = np.concatenate([around([1 / 32, -1 / 32], 4), np.array([0.0, -0.0], F)])
    pe = np.stack([edge, np.roll(edge, 1), np.roll(edge, 7)], axis=1)
    ne = np.tile(np.array([[0.6, -0.8, 0.0], [-1, 0, 0], [0, 0, 1], [-0.0, 0.0, -1.0]], F), (len(pe) // 4 + 1, 1))[:len(pe)]
    return _frozen(np.concatenate([p, pe])), _frozen(np.concatenate([n, ne]))


# ---------------------------------------------------------------- the device's lists and the oracle's answer for them
def a4(*cols):
    """The float4 argument list of gfx_math_eval: the given columns first, zeros after."""
    a = np.zeros((len(cols[0]), 4), F)
    for i, c in enumerate(cols):
        a[:, i] = c
    return a


def _exp_domain(x):
    return x[(x >= F(EXP_MIN)) & (x <= F(EXP_MAX))]


def _sincos_domain(x):
    return x[~(np.abs(x) >= F(SINCOS_PARITY_MAX))]                       # keeps the NaNs


def _unary_lists(select=lambda x: x):
    return {name: (lambda f=f: (a4(select(f())), None)) for name, f in UNARY_LISTS.items()}


def codes_a4(q):
    """Codes as the bits of A.x."""
    return a4(np.ascontiguousarray(q, U).view(F))


# fn name (gfxexp_amd.api.MATH_<name>) -> list name -> () -> (A float32 [n, 4], B float32 [n, 4] or None)
GPU_LISTS = {
    "SINCOS": _unary_lists(_sincos_domain),
    "EXP": _unary_lists(_exp_domain),
    "ACOS": _unary_lists(),
    "ATAN": _unary_lists(),
    "ATAN2": {"pairs": lambda: (a4(atan2_pairs()[:, 0], atan2_pairs()[:, 1]), None)},
    "SAT": _unary_lists(),
    "TO_POLAR": {"directions": lambda: (a4(*all_directions().T), None)},
    "DECODE_DIR": {"edges": lambda: (codes_a4(dir_codes_edges()), None), "grid": lambda: (codes_a4(dir_codes_grid()), None)},
    "ENCODE_UV": {"pairs": lambda: (a4(uv_pairs()[:, 0], uv_pairs()[:, 1]), None)},
    "DECODE_UV": {"codes": lambda: (codes_a4(uv_codes()), None)},
    "ENCODE_BC": {"values": lambda: (a4(unorm_values()), None)},
    "DECODE_BC": {"codes": lambda: (codes_a4(uv_codes()), None)},
    "OFFSET_RAY_ORIGIN": {"points": lambda: (a4(*offset_cases()[0].T), a4(*offset_cases()[1].T))},
}

# NaN words the oracle returns for each list (all result words of all elements counted).  A property of the lists and of the
# contract, recorded by tests/test_math_contract_cpu.py; the device must return NaN in exactly as many words, in the same places.
NAN_WORDS = {
    ("SINCOS", "strided"): 261124, ("SINCOS", "edges"): 4, ("EXP", "strided"): 0, ("EXP", "edges"): 0,
    ("ACOS", "strided"): 8421249, ("ACOS", "edges"): 2226043, ("ATAN", "strided"): 65281, ("ATAN", "edges"): 1,
    ("ATAN2", "pairs"): 27, ("SAT", "strided"): 0, ("SAT", "edges"): 0, ("TO_POLAR", "directions"): 2,
    ("DECODE_DIR", "edges"): 0, ("DECODE_DIR", "grid"): 0, ("ENCODE_UV", "pairs"): 0, ("DECODE_UV", "codes"): 0,
    ("ENCODE_BC", "values"): 0, ("DECODE_BC", "codes"): 0, ("OFFSET_RAY_ORIGIN", "points"): 0,
}


def _bits(x):
    return np.ascontiguousarray(x).view(U) if np.asarray(x).dtype != U else np.ascontiguousarray(x)


def oracle_words(fn, A, B=None):
    """The result words of gfx_math_eval(fn) on (A, B) according to the oracle: a list of uint32 [n] (floats as bits); words the
    function does not return are omitted and must be 0 on the device."""
    from oracle import oracle as O
    x = np.ascontiguousarray(A[:, 0])
    if fn == "SINCOS":
        s, c = O.math_sincos(x)
        return [_bits(s), _bits(c), _bits(O.math_tan(x)), _bits(O.math_sin(x))]
    if fn == "EXP":
        return [_bits(O.math_exp(x))]
    if fn == "ACOS":
        return [_bits(O.math_acos(x))]
    if fn == "ATAN":
        return [_bits(O.math_atan(x))]
    if fn == "ATAN2":
        return [_bits(O.math_atan2(x, np.ascontiguousarray(A[:, 1])))]
    if fn == "SAT":
        i32, u32, q = O.math_sat(x)
        return [i32.view(U), u32, q]
    if fn == "TO_POLAR":
        v = np.ascontiguousarray(A[:, :3])
        phi, theta = O.to_polar(v)
        return [_bits(phi), _bits(theta), O.encode_normal(v)]
    if fn == "DECODE_DIR":
        v = O.decode_normal(x.view(U))
        return [_bits(np.ascontiguousarray(v[:, i])) for i in range(3)]
    if fn == "ENCODE_UV":
        return [O.encode_uv(np.ascontiguousarray(A[:, :2]))]
    if fn == "DECODE_UV":
        uv = O.decode_uv(x.view(U))
        return [_bits(np.ascontiguousarray(uv[:, 0])), _bits(np.ascontiguousarray(uv[:, 1]))]
    if fn == "ENCODE_BC":
        return [O.encode_bc(x)]
    if fn == "DECODE_BC":
        return [_bits(O.decode_bc(x.view(U) & 0xFFFF))]
    if fn == "OFFSET_RAY_ORIGIN":
        p = O.offset_ray_origin(np.ascontiguousarray(A[:, :3]), np.ascontiguousarray(B[:, :3]))
        return [_bits(np.ascontiguousarray(p[:, i])) for i in range(3)]
    raise KeyError(fn)


FLOAT_WORDS = {"SINCOS": 4, "EXP": 1, "ACOS": 1, "ATAN": 1, "ATAN2": 1, "SAT": 0, "TO_POLAR": 2, "DECODE_DIR": 3, "ENCODE_UV": 0, "DECODE_UV": 2,
               "ENCODE_BC": 0, "DECODE_BC": 1, "OFFSET_RAY_ORIGIN": 3}           # how many of the leading result words are floats


def nan_words(fn, words):
    """Number of NaNs among the float result words."""
    return int(sum(np.count_nonzero(np.isnan(w.view(F))) for w in words[:FLOAT_WORDS[fn]]))


# ---------------------------------------------------------------- the third copy of the sincos (host/env_tables.cpp)
def neighbor_delta_polar():
    """(r, theta) float32 [1024] of gfxh_spatial_neighbor_deltas: Halton(2, 3) through the concentric square -> disk map, in the
    host code's own fp32 operations up to the sincos, so that table[i] = (r cos theta, r sin theta) with the contract's sincos.
    Entry 0 is the centre (r = 0)."""
    def halton(base, idx):
        rec, ret, scale = F(1.0) / F(base), F(0.0), F(1.0)
        while idx:
            scale = scale * rec
            ret = ret + F(idx % base) * scale
            idx //= base
        return ret
    r, theta = np.zeros(1024, F), np.zeros(1024, F)
    quarter_pi = F(3.14159265358979323846) / F(4)
    for i in range(1024):
        sx, sy = F(2) * halton(2, i) - F(1), F(2) * halton(3, i) - F(1)
        if sx == 0 and sy == 0:
            continue
        if sx >= -sy:
            r[i], t = (sx, sy / sx) if sx > sy else (sy, F(2) - sx / sy)
        else:
            r[i], t = (-sy, F(6) + sx / sy) if sx > sy else (-sx, F(4) + sy / sx)
        theta[i] = t * quarter_pi
    return r, theta
