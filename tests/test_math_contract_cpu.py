"""CPU: the oracle copy of the deterministic math contract (oracle/orc_math.h, contract version 1) and of the 16-bit quantisers
(oracle/orc_shared.h) against numpy float64 on the fp32 inputs widened exactly, over the lists of tests/math_cases.py.
tests/test_gpu_math_contract.py holds the device copy equal to the oracle, bit for bit, on the same lists.

Errors are in ulp: units of the fp32 spacing of the reference value, with the spacing of the smallest normal (2^-149) as its floor.
Each bound was fixed this way: MEASURED[...] is the worst error of the oracle copy over exactly these lists, BOUNDS[...] is that
rounded up to the next 0.25 ulp (absolute bounds: to the next 0.25e-7).  A bound is a property of the algorithm against libm,
so a change of either copy that misses it is a change of the contract.  Outside a stated domain nothing is compared with libm: there
gm_exp and the large-argument gm_sincos are unspecified.  Within a domain no case is skipped and no result may be NaN."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import math_cases as MC

F, U = np.float32, np.uint32
SUBNORMAL_SPACING = 2.0 ** -149

# The worst input of each row is printed by the tests; DESIGN.md ("The deterministic math contract") repeats the table.  The ulp
# figures of sin, cos and tan beyond a few periods belong to the few floats that lie next to a multiple of pi/2, where the
# reference is ~1e-7 and less while the absolute error stays below 1e-7 (the float next to 1288 pi: sin = 6.7e-8, error 4.4e-12).
MEASURED = {
    "sin ulp |x|<=2pi": 1.458, "cos ulp |x|<=2pi": 5.793,
    "sin ulp |x|<=1e4": 621.8, "cos ulp |x|<=1e4": 16.14, "tan ulp |x|<=1e4": 621.8,
    "sin abs |x|<=1e6": 1.0102e-07, "cos abs |x|<=1e6": 9.213e-08,
    "tan ulp |x|<=1.5": 2.890,
    "exp ulp normal": 1.0074, "exp abs subnormal": 0.7503,
    "acos ulp [-1,1]": 1.2553, "atan ulp finite,inf": 2.779, "atan2 ulp finite pairs": 3.0125,
    "to_polar phi abs": 7.420e-07, "to_polar theta ulp": 1.2777, "decode_dir abs": 5.872e-07,
}
BOUNDS = {
    "sin ulp |x|<=2pi": 1.5, "cos ulp |x|<=2pi": 6.0,
    "sin ulp |x|<=1e4": 622.0, "cos ulp |x|<=1e4": 16.25, "tan ulp |x|<=1e4": 622.0,
    "sin abs |x|<=1e6": 1.25e-07, "cos abs |x|<=1e6": 1.0e-07,
    "tan ulp |x|<=1.5": 3.0,
    "exp ulp normal": 1.25, "exp abs subnormal": 1.0,                    # the second is set, not measured: one subnormal spacing
    "acos ulp [-1,1]": 1.5, "atan ulp finite,inf": 3.0, "atan2 ulp finite pairs": 3.25,
    "to_polar phi abs": 7.5e-07, "to_polar theta ulp": 1.5, "decode_dir abs": 6.0e-07,
}


def ulp_err(got, ref):
    """|got - ref| in units of the fp32 spacing at ref (float64), the spacing never below that of the smallest normal."""
    at = np.maximum(np.abs(ref).astype(F), F(MC.FLT_MIN))
    return np.abs(got.astype(np.float64) - ref) / np.spacing(at).astype(np.float64)


def worst(name, err, *args):
    """Prints the worst error with the input that produced it and returns it; a NaN anywhere is a failure."""
    assert len(err) > 0, name
    assert not np.any(np.isnan(err)), f"{name}: {np.count_nonzero(np.isnan(err))} results are NaN, first at {[a[np.flatnonzero(np.isnan(err))[0]] for a in args]}"
    i = int(np.argmax(err))
    where = ", ".join(f"{a[i]!r} ({int(np.asarray(a[i], F).view(U)):#010x})" for a in args)
    print(f"{name:<34s} worst {err[i]:.4g} at {where}   [{len(err)} cases]")
    return float(err[i])


def check(name, err, *args):
    w = worst(name, err, *args)
    assert w <= BOUNDS[name], f"{name}: {w} exceeds the bound {BOUNDS[name]}"
    return w


@pytest.fixture(scope="module")
def unary():
    return np.concatenate([MC.unary_strided(), MC.unary_edges()])


def measure_sincos(x, check=worst):
    out = {}
    x = x[np.abs(x) <= F(MC.SINCOS_ABS_MAX)]                               # the widest stated domain; leaves the NaNs out
    s, c = O.math_sincos(x)
    t = O.math_tan(x)
    x64 = x.astype(np.float64)
    s64, c64 = np.sin(x64), np.cos(x64)
    m = np.abs(x) <= F(2 * np.pi)                                          # where the quantisers and the frames call it
    out["sin ulp |x|<=2pi"] = check("sin ulp |x|<=2pi", ulp_err(s[m], s64[m]), x[m])
    out["cos ulp |x|<=2pi"] = check("cos ulp |x|<=2pi", ulp_err(c[m], c64[m]), x[m])
    m = np.abs(x) <= F(MC.SINCOS_ULP_MAX)
    t64 = np.tan(x64[m])
    out["sin ulp |x|<=1e4"] = check("sin ulp |x|<=1e4", ulp_err(s[m], s64[m]), x[m])
    out["cos ulp |x|<=1e4"] = check("cos ulp |x|<=1e4", ulp_err(c[m], c64[m]), x[m])
    out["tan ulp |x|<=1e4"] = check("tan ulp |x|<=1e4", ulp_err(t[m], t64), x[m])
    out["sin abs |x|<=1e6"] = check("sin abs |x|<=1e6", np.abs(s - s64), x)
    out["cos abs |x|<=1e6"] = check("cos abs |x|<=1e6", np.abs(c - c64), x)
    m2 = np.abs(x[m]) <= F(MC.TAN_ULP_MAX)
    out["tan ulp |x|<=1.5"] = check("tan ulp |x|<=1.5", ulp_err(t[m][m2], t64[m2]), x[m][m2])
    return out


def measure_exp(x, check=worst):
    out = {}
    m = (x >= F(MC.EXP_NORMAL_MIN)) & (x <= F(MC.EXP_MAX))
    y = O.math_exp(x[m])
    assert np.all(np.isfinite(y)) and np.all(y >= F(MC.FLT_MIN))          # "normal" is the oracle's own result, on the whole interval
    out["exp ulp normal"] = check("exp ulp normal", ulp_err(y, np.exp(x[m].astype(np.float64))), x[m])
    m = (x >= F(MC.EXP_MIN)) & (x < F(MC.EXP_NORMAL_MIN))
    y = O.math_exp(x[m])
    assert np.all(y > 0) and np.all(y < F(MC.FLT_MIN))                    # ... and so is "subnormal"
    out["exp abs subnormal"] = check("exp abs subnormal", np.abs(y.astype(np.float64) - np.exp(x[m].astype(np.float64))) / SUBNORMAL_SPACING, x[m])
    return out


def measure_acos(x, check=worst):
    m = np.abs(x) <= 1
    return {"acos ulp [-1,1]": check("acos ulp [-1,1]", ulp_err(O.math_acos(x[m]), np.arccos(x[m].astype(np.float64))), x[m])}


def measure_atan(x, check=worst):
    m = ~np.isnan(x)
    return {"atan ulp finite,inf": check("atan ulp finite,inf", ulp_err(O.math_atan(x[m]), np.arctan(x[m].astype(np.float64))), x[m])}


def measure_atan2(p, check=worst):
    m = np.all(np.isfinite(p), axis=1)
    y, x = np.ascontiguousarray(p[m, 0]), np.ascontiguousarray(p[m, 1])
    # the contract gives a zero no direction (the table of test_atan2_special_values pins every case by bits): the reference sees -0 as +0
    ref = np.arctan2(y.astype(np.float64) + 0.0, x.astype(np.float64) + 0.0)
    return {"atan2 ulp finite pairs": check("atan2 ulp finite pairs", ulp_err(O.math_atan2(y, x), ref), y, x)}


def test_sincos_and_tan(unary):
    measure_sincos(unary, check)
    # gm_sin is gm_sincos' sine
    x = unary[np.abs(unary) <= F(MC.SINCOS_ABS_MAX)]
    assert np.array_equal(O.math_sin(x).view(U), O.math_sincos(x)[0].view(U))


def test_exp(unary):
    measure_exp(unary, check)
    # the ends of the domain are the ends: one float further the scale factor leaves fp32 and the result is 0 / +inf
    ends = np.array([MC.EXP_MIN, MC.EXP_MAX, MC.EXP_NORMAL_MIN], F)
    below, above, sub = np.nextafter(ends[0], F(-np.inf)), np.nextafter(ends[1], F(np.inf)), np.nextafter(ends[2], F(-np.inf))
    y = O.math_exp(np.array([ends[0], below, ends[1], above, ends[2], sub], F))
    assert 0 < y[0] < MC.FLT_MIN and y[1].view(U) == 0
    assert np.isfinite(y[2]) and y[3].view(U) == 0x7F800000
    assert y[4] >= MC.FLT_MIN > y[5] > 0
    # +-80, the guard of the denoiser, is well inside
    assert MC.EXP_MIN < -80 and 80 < MC.EXP_MAX


def test_acos(unary):
    measure_acos(unary, check)
    # outside [-1, 1] the result is NaN, from the first float beyond: a property of the lists, counted here and again on the device
    out = unary[~(np.abs(unary) <= 1)]
    assert np.all(np.isnan(O.math_acos(out)))
    assert np.isnan(O.math_acos(np.array([np.nextafter(F(1), F(2)), np.nextafter(F(-1), F(-2))], F))).all()


def test_atan(unary):
    measure_atan(unary, check)


def test_atan2():
    measure_atan2(MC.atan2_pairs(), check)


def _b(x):
    return int(np.asarray(x, F).reshape(-1)[0].view(U))


HALF_PI, PI = 0x3FC90FDB, 0x40490FDB


def test_exact_values():
    z = np.array([0.0, -0.0], F)
    s, c = O.math_sincos(z)
    # sin(-0) is +0: the reduction r = fma(q, -c1, x) adds +0 to -0
    assert [_b(s[0]), _b(s[1]), _b(c[0]), _b(c[1])] == [0x00000000, 0x00000000, 0x3F800000, 0x3F800000]
    assert [_b(v) for v in O.math_tan(z)] == [0x00000000, 0x00000000]
    assert [_b(v) for v in O.math_exp(z)] == [0x3F800000, 0x3F800000]
    assert [_b(v) for v in O.math_acos(np.array([1.0, -1.0, 0.0], F))] == [0x00000000, PI, HALF_PI]
    assert [_b(v) for v in O.math_atan(np.array([np.inf, -np.inf, 0.0, -0.0], F))] == [HALF_PI, HALF_PI | 0x80000000, 0x00000000, 0x00000000]
    i32, u32, q = O.math_sat(np.array([2.0 ** 31, -2.0 ** 31, 2.0 ** 32, np.nan, -1.0, np.inf, -np.inf, 65535.5 / 65535, 1.0, -0.0, 0.5], F))
    assert list(i32) == [2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, 0, -1, 2 ** 31 - 1, -2 ** 31, 1, 1, 0, 0]
    assert list(u32) == [2 ** 31, 0, 2 ** 32 - 1, 0, 0, 2 ** 32 - 1, 0, 1, 1, 0, 0]
    assert list(q) == [65535, 0, 65535, 0, 0, 65535, 0, 65535, 65535, 0, 32767]
    below = np.nextafter(F(2.0 ** 31), F(0)), np.nextafter(F(2.0 ** 32), F(0)), np.nextafter(F(-2.0 ** 31), F(0))
    i32, u32, _ = O.math_sat(np.array(below, F))
    assert (int(i32[0]), int(u32[1]), int(i32[2])) == (2 ** 31 - 128, 2 ** 32 - 256, -2 ** 31 + 128)


NAN = 0x7FC00000      # stands for any NaN: its sign and payload are not part of the contract
# gm_atan2(y, x) over math_cases.ATAN2_SPECIAL_VALUES, as it is today and as gm_math.hip.h / orc_math.h state it.  It departs from IEEE
# atan2 where a zero's sign or two infinities would decide: (+-0, -0) = +0 (IEEE +-pi), (-0, x > 0) = +0 (IEEE -0), (-0, x < 0) = +pi
# (IEEE -pi), (+-inf, +-inf) = NaN (IEEE +-pi/4, +-3pi/4), (NaN, +-0) = +pi/2 (IEEE NaN).  to_polar_yup at the seam rests on it.
#      x = +0         -0          1           -1          FLT_MIN     -FLT_MIN    1e-45       -1e-45      3e38        -3e38       inf         -inf        nan
ATAN2_TABLE = (
    (0x00000000, 0x00000000, 0x00000000, 0x40490FDB, 0x00000000, 0x40490FDB, 0x00000000, 0x40490FDB, 0x00000000, 0x40490FDB, 0x00000000, 0x40490FDB, NAN),   # y = +0
    (0x00000000, 0x00000000, 0x00000000, 0x40490FDB, 0x00000000, 0x40490FDB, 0x00000000, 0x40490FDB, 0x00000000, 0x40490FDB, 0x00000000, 0x40490FDB, NAN),   # y = -0
    (0x3FC90FDB, 0x3FC90FDB, 0x3F490FDB, 0x4016CBE4, 0x3FC90FDB, 0x3FC90FDB, 0x3FC90FDB, 0x3FC90FDB, 0x00244BFA, 0x40490FDB, 0x00000000, 0x40490FDB, NAN),   # y = 1
    (0xBFC90FDB, 0xBFC90FDB, 0xBF490FDB, 0xC016CBE4, 0xBFC90FDB, 0xBFC90FDB, 0xBFC90FDB, 0xBFC90FDB, 0x80244BFA, 0xC0490FDB, 0x80000000, 0xC0490FDB, NAN),   # y = -1
    (0x3FC90FDB, 0x3FC90FDB, 0x00800000, 0x40490FDB, 0x3F490FDB, 0x4016CBE4, 0x3FC90FDA, 0x3FC90FDC, 0x00000000, 0x40490FDB, 0x00000000, 0x40490FDB, NAN),   # y = FLT_MIN
    (0xBFC90FDB, 0xBFC90FDB, 0x80800000, 0xC0490FDB, 0xBF490FDB, 0xC016CBE4, 0xBFC90FDA, 0xBFC90FDC, 0x80000000, 0xC0490FDB, 0x80000000, 0xC0490FDB, NAN),   # y = -FLT_MIN
    (0x3FC90FDB, 0x3FC90FDB, 0x00000001, 0x40490FDB, 0x34000000, 0x40490FDA, 0x3F490FDB, 0x4016CBE4, 0x00000000, 0x40490FDB, 0x00000000, 0x40490FDB, NAN),   # y = 1e-45
    (0xBFC90FDB, 0xBFC90FDB, 0x80000001, 0xC0490FDB, 0xB4000000, 0xC0490FDA, 0xBF490FDB, 0xC016CBE4, 0x80000000, 0xC0490FDB, 0x80000000, 0xC0490FDB, NAN),   # y = -1e-45
    (0x3FC90FDB, 0x3FC90FDB, 0x3FC90FDB, 0x3FC90FDB, 0x3FC90FDB, 0x3FC90FDB, 0x3FC90FDB, 0x3FC90FDB, 0x3F490FDB, 0x4016CBE4, 0x00000000, 0x40490FDB, NAN),   # y = 3e38
    (0xBFC90FDB, 0xBFC90FDB, 0xBFC90FDB, 0xBFC90FDB, 0xBFC90FDB, 0xBFC90FDB, 0xBFC90FDB, 0xBFC90FDB, 0xBF490FDB, 0xC016CBE4, 0x80000000, 0xC0490FDB, NAN),   # y = -3e38
    (0x3FC90FDB, 0x3FC90FDB, 0x3FC90FDB, 0x3FC90FDB, 0x3FC90FDB, 0x3FC90FDB, 0x3FC90FDB, 0x3FC90FDB, 0x3FC90FDB, 0x3FC90FDB, NAN, NAN, NAN),                 # y = inf
    (0xBFC90FDB, 0xBFC90FDB, 0xBFC90FDB, 0xBFC90FDB, 0xBFC90FDB, 0xBFC90FDB, 0xBFC90FDB, 0xBFC90FDB, 0xBFC90FDB, 0xBFC90FDB, NAN, NAN, NAN),                 # y = -inf
    (0x3FC90FDB, 0x3FC90FDB, NAN, NAN, NAN, NAN, NAN, NAN, NAN, NAN, NAN, NAN, NAN),                                                                         # y = nan
)


def test_atan2_special_values():
    p = MC.atan2_special()
    got = O.math_atan2(p[:, 0], p[:, 1])
    want = np.array(ATAN2_TABLE, U).ravel()
    nan = want == NAN
    assert np.array_equal(np.isnan(got), nan), f"NaN where a number is due or the reverse: {p[np.isnan(got) != nan]}"
    bad = (got.view(U) != want) & ~nan
    assert not np.any(bad), f"{np.count_nonzero(bad)} entries changed, first (y, x) = {p[bad][0]}: {got.view(U)[bad][0]:#010x}, table {want[bad][0]:#010x}"


# ---------------------------------------------------------------- the quantisers against float64
ROUND_TRIP_CHORD = np.hypot(np.pi / 65535, 2 * np.pi / 65535) * 1.05      # the bound of test_polar_quantiser_round_trip (test_oracle_golden.py)


def _polar64(v):
    v = v.astype(np.float64)
    theta = np.arccos(np.clip(v[:, 1], -1.0, 1.0))
    phi = np.mod(np.arctan2(-v[:, 0] + 0.0, v[:, 2] + 0.0), 2 * np.pi)
    return phi, theta


def measure_polar(check=worst):
    out = {}
    d = MC.directions()
    v = np.concatenate([d[k] for k in MC.UNIT_DIRECTION_LISTS + ("non_unit",)])
    phi, theta = O.to_polar(v)
    assert np.all((phi >= 0) & (phi < F(2 * np.pi))) and np.all((theta >= 0) & (theta <= F(np.pi)))
    phi64, theta64 = _polar64(v)
    dphi = np.abs(phi.astype(np.float64) - phi64)
    dphi = np.minimum(dphi, 2 * np.pi - dphi)                             # the seam: 2 pi - tiny is phi = 0
    out["to_polar phi abs"] = check("to_polar phi abs", dphi, v[:, 0], v[:, 1], v[:, 2])
    out["to_polar theta ulp"] = check("to_polar theta ulp", ulp_err(theta, theta64), v[:, 0], v[:, 1], v[:, 2])
    q = np.concatenate([MC.dir_codes_edges(), MC.dir_codes_grid()])
    got = O.decode_normal(q).astype(np.float64)
    k = np.arange(65536) / 65535.0                                        # float64 trigonometry once per code, gathered per element
    sp, cp, st, ct = np.sin(2 * np.pi * k), np.cos(2 * np.pi * k), np.sin(np.pi * k), np.cos(np.pi * k)
    ip, it = q & 0xFFFF, q >> 16
    ref = np.stack([-sp[ip] * st[it], ct[it], cp[ip] * st[it]], axis=1)
    out["decode_dir abs"] = check("decode_dir abs", np.max(np.abs(got - ref), axis=1), q.view(F))
    return out


def test_polar_angles_and_decode():
    measure_polar(check)


@pytest.mark.parametrize("name", MC.UNIT_DIRECTION_LISTS)
def test_direction_round_trip(name):
    """decode_dir(encode_dir(v)) within the angle bound of test_polar_quantiser_round_trip, on the seam and at the poles too."""
    v = MC.directions()[name]
    d = O.decode_normal(O.encode_normal(v)).astype(np.float64)
    chord = np.linalg.norm(d - v.astype(np.float64), axis=1)              # chord ~ angle; the lists are unit vectors to fp32 rounding
    w = worst(f"round trip chord, {name}", chord, v[:, 0], v[:, 1], v[:, 2])
    assert w < ROUND_TRIP_CHORD


def test_clamp_and_nan_directions():
    d = MC.directions()
    phi, theta = O.to_polar(d["nan"])
    # NaN in x or z: phi is NaN and its code 0; NaN in y: the select of the clamp gives -1, theta = pi
    assert np.isnan(phi[0]) and np.isnan(phi[2]) and not np.isnan(phi[1]) and not np.any(np.isnan(theta))
    assert _b(theta[1]) == PI
    q = O.encode_normal(d["nan"])
    assert q[0] & 0xFFFF == 0 and q[2] & 0xFFFF == 0 and q[1] >> 16 == 65535
    assert MC.nan_words("TO_POLAR", [phi.view(U), theta.view(U)]) == 2
    v = np.array([[0, 4, 0], [0, -4, 0], [0, 1.0000001, 0], [0, -1.0000001, 0]], F)
    _, theta = O.to_polar(v)
    assert [_b(t) for t in theta] == [0, PI, 0, PI]


def test_unorm_quantisers():
    x = MC.unorm_values()
    q = O.encode_bc(x)
    x64 = np.nan_to_num(np.clip(x.astype(np.float64), 0.0, 1.0), nan=0.0)
    exact = np.floor(x64 * 65535.0)
    assert np.all(q <= 65535)
    assert np.max(np.abs(q.astype(np.float64) - exact)) <= 1              # the fp32 product may round across a cell border
    back = O.decode_bc(q)
    assert np.array_equal(back.view(U), (q.astype(np.float64) / 65535.0).astype(F).view(U))
    assert np.max(np.abs(back.astype(np.float64) - x64)) <= 1.0 / 65535 + 2.0 ** -24
    k = np.arange(65536)
    assert np.array_equal(O.encode_bc(((k + 0.5) / 65535).astype(F))[:-1], k[:-1])     # the middle of a cell gives its code
    assert np.array_equal(O.encode_bc(O.decode_bc(k.astype(U))), k)                    # and so does the code's own value
    uv = MC.uv_pairs()
    quv = O.encode_uv(uv)
    for half, col in ((quv & 0xFFFF, uv[:, 0]), (quv >> 16, uv[:, 1])):
        c64 = col.astype(np.float64)
        with np.errstate(invalid="ignore"):
            frac = np.nan_to_num(c64 - np.floor(c64), nan=0.0)            # NaN and inf - inf encode as 0
        diff = np.abs(half.astype(np.float64) - np.floor(frac * 65535.0))
        assert np.max(np.minimum(diff, 65535 - diff)) <= 1                # -tiny wraps to 1.0 in fp32: code 65535, next to 65534
    codes = MC.uv_codes()
    duv = O.decode_uv(codes)
    assert np.array_equal(duv[:, 0].view(U), ((codes & 0xFFFF) / 65535.0).astype(F).view(U))
    assert np.array_equal(duv[:, 1].view(U), ((codes >> 16) / 65535.0).astype(F).view(U))


@pytest.mark.parametrize("fn", list(MC.GPU_LISTS))
def test_nan_words_of_the_parity_lists(fn):
    """The NaN count the device test holds the kernel to is the oracle's, and the lists keep to their size limit."""
    for name, make in MC.GPU_LISTS[fn].items():
        A, B = make()
        assert 0 < len(A) <= 1 << 24
        assert MC.nan_words(fn, MC.oracle_words(fn, A, B)) == MC.NAN_WORDS[(fn, name)], (fn, name)


def test_host_table_against_the_oracle_sincos(built_lib):
    """gfxh_spatial_neighbor_deltas (the sincos copy of host/env_tables.cpp) is r (cos, sin) of the oracle's gm_sincos."""
    from gfxexp_amd import api
    r, theta = MC.neighbor_delta_polar()
    s, c = O.math_sincos(theta)
    mine = np.stack([r * c, r * s], axis=1)
    mine[r == 0] = 0
    assert np.array_equal(mine.view(U), api.spatial_neighbor_deltas().view(U))
