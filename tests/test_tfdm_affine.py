"""CPU: the small pieces of csrc/tfdm/tfdm_core.hip.h on their own, through the host compilation (tests/tfdm_host.cpp), against
float64 numpy: the outward-rounded interval of an affine form, the enclosures of `reciprocal` and `recSqrt`, the corner sample and
the triangle / square classification.

What an enclosure may miss by is the core's own allowance for the fp32 roundings inside an operation, the one `to_interval` adds
when a form becomes an interval: 2^-19 of the sum of the magnitudes of the form's coefficients."""
import ctypes as C

import numpy as np
import pytest

from gfxexp_amd import api
from tests import tfdm_host as T
from tests import util


@pytest.fixture(scope="module")
def host(built_lib, tmp_path_factory):
    return T.Host(tmp_path_factory.mktemp("tfdm_affine"))


def _f4(a):
    return np.ascontiguousarray(a, np.float32)


def _interval(host, form):
    out = np.zeros(2, np.float32)
    host.L.tfdm_host_interval(T._p(_f4(form)), T._p(out))
    return out.astype(np.float64)


def _unary(host, op, form):
    out = np.zeros(4, np.float32)
    host.L.tfdm_host_affine_unary(C.c_int(op), T._p(_f4(form)), T._p(out))
    return out.astype(np.float64)


def _forms(rng, n, positive):
    """Random affine forms (centre, two coefficients, error term >= 0) over five decades; `positive`: the range stays above zero."""
    out = []
    while len(out) < n:
        mag = 10.0 ** rng.uniform(-3, 2)
        c = mag * (rng.uniform(0.2, 1.0) if positive else rng.uniform(-1.0, 1.0))
        u, v = mag * rng.uniform(-0.4, 0.4, 2) * rng.choice([0.0, 1e-3, 1.0])
        k = mag * rng.uniform(0, 0.15) * rng.choice([0.0, 1.0])
        f = _f4([c, u, v, k]).astype(np.float64)
        if positive and f[0] - abs(f[1]) - abs(f[2]) - f[3] <= 0.05 * f[0]:
            continue
        out.append(f)
    return out


def test_interval_is_rounded_outward(host):
    rng = np.random.default_rng(21)
    for f in _forms(rng, 2000, positive=False):
        lo, hi = _interval(host, f)
        r = abs(f[1]) + abs(f[2]) + f[3]                    # exact in float64: four fp32 terms of similar size
        assert lo <= f[0] - r and f[0] + r <= hi, (f, lo, hi)
        assert hi - lo <= 2 * r + 2.0 ** -17 * (abs(f[0]) + r), "the interval of %s is wider than its allowance" % f
    # something not finite becomes the whole line, never a NaN that a comparison would skip
    lo, hi = _interval(host, [np.inf, 1, 0, 0])
    assert lo == -np.inf and hi == np.inf
    lo, hi = _interval(host, [0, 0, 0, np.inf])
    assert lo == -np.inf and hi == np.inf


@pytest.mark.parametrize("op", ["reciprocal", "rec_sqrt"])
def test_unary_enclosure(host, op):
    """f(x) for every x the form can take lies in the resulting form evaluated at the same noise symbols, give or take its error
    term (and the allowance of the module docstring)."""
    rng = np.random.default_rng(22 if op == "reciprocal" else 23)
    g = np.linspace(-1, 1, 17)
    e1, e2, e3 = [a.ravel() for a in np.meshgrid(g, g, np.array([-1.0, 0.0, 1.0]))]
    signs = [1.0, -1.0] if op == "reciprocal" else [1.0]
    for f in _forms(rng, 600, positive=True):
        for s in signs:
            form = f * np.array([s, 1, 1, 1])
            r = _unary(host, 0 if op == "reciprocal" else 1, form)
            assert np.all(np.isfinite(r)) and r[3] >= 0
            x = form[0] + form[1] * e1 + form[2] * e2 + form[3] * e3
            want = 1.0 / x if op == "reciprocal" else 1.0 / np.sqrt(x)
            centre = r[0] + r[1] * e1 + r[2] * e2
            allow = 2.0 ** -19 * (abs(r[0]) + abs(r[1]) + abs(r[2]) + r[3])
            miss = np.abs(want - centre) - r[3]
            assert miss.max() <= allow, "%s of %s: off by %.3e beyond the error term %.3e (allowance %.3e)" % (op, form, miss.max(), r[3], allow)
            # and the approximation is worth something: the error term stays below the range of f itself
            assert r[3] <= (want.max() - want.min()) + allow
    # a range that reaches zero has no bounded answer
    for form in ([0.1, 0.2, 0, 0], [0.0, 0, 0, 0], [1.0, 0.5, 0.5, 0.1]):
        assert _unary(host, 0 if op == "reciprocal" else 1, form)[3] == np.inf
    if op == "rec_sqrt":
        assert _unary(host, 1, [-1.0, 0.1, 0, 0])[3] == np.inf


def test_corner_height_is_the_four_term_sum_with_repeat_wrap(host):
    rng = np.random.default_rng(24)
    heights = (rng.integers(0, 256, (16, 16)).astype(np.float32) / np.float32(255)).astype(np.float32)
    levels = host.levels(heights)
    host.L.tfdm_host_corner_height.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int]
    for level, m in enumerate(T.mips32(heights)):
        n = m.shape[0]
        q = np.float32(0.25)
        for px, py in [(0, 0), (1, 1), (n, n), (n - 1, 0), (-1, 2), (3 * n + 2, -2 * n - 1), (5, n + 3)]:
            a, b, c, d = (px - 1) % n, px % n, (py - 1) % n, py % n
            want = ((q * m[c, a] + q * m[c, b]) + q * m[d, a]) + q * m[d, b]
            got = np.float32(host.L.tfdm_host_corner_height(levels.ctypes.data, 16, level, px, py))
            util.assert_same_bits("corner (%d, %d) of level %d" % (px, py, level), np.array([got]), np.array([want], np.float32))


def test_classification_of_a_square_against_a_triangle(host):
    """Outside / inside / overlapping against the separating-axis test in float64.  Coordinates are multiples of 1/8, so every product
    in either code is exact and a touching pair is known as such: those are left out (either answer is right for them)."""
    rng = np.random.default_rng(25)
    host.L.tfdm_host_classify.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float]
    seen = {0: 0, 1: 0, 2: 0}
    tris = 0
    while tris < 60:
        tc = rng.integers(-40, 41, (3, 2)) / 8.0
        area = T._cross2(tc[1] - tc[0], tc[2] - tc[0])
        if area == 0:
            continue
        tris += 1
        v = np.zeros(3, api.VERTEX_DTYPE)
        v["position"] = [(0, 0, 0), (1, 0, 0), (0, 1, 0)]
        v["normal"] = (0, 0, 1)
        v["texCoord0Dir"] = (1, 0, 0)
        v["texCoord"] = tc
        rec = host.records(v, np.array([[0, 1, 2]], np.uint32), api.tfdm_params(), 64)
        assert rec["flipped"][0] == (1 if area < 0 else 0)
        s = 1.0 if area > 0 else -1.0
        for _ in range(150):
            half = float(rng.choice([0.125, 0.25, 0.5, 1.0, 2.0]))
            cx, cy = rng.integers(-48, 49, 2) / 8.0
            corners = np.array([[cx + sx * half, cy + sy * half] for sx in (-1, 1) for sy in (-1, 1)])
            axes = [np.array([1.0, 0.0]), np.array([0.0, 1.0])] + [np.array([e[1], -e[0]]) for e in (tc[1] - tc[0], tc[2] - tc[1], tc[0] - tc[2])]
            gaps = [min((tc @ a).max(), (corners @ a).max()) - max((tc @ a).min(), (corners @ a).min()) for a in axes]
            side = np.array([[s * T._cross2(tc[(k + 1) % 3] - tc[k], c - tc[k]) for k in range(3)] for c in corners])
            if min(abs(g) for g in gaps) == 0 or np.any(side == 0):
                continue
            want = 0 if min(gaps) < 0 else 1 if np.all(side > 0) else 2
            assert bool(T.overlap_sat(tc, np.array(cx), np.array(cy), half)) == (want != 0)
            got = host.L.tfdm_host_classify(rec.ctypes.data, cx, cy, half)
            assert got == want, "triangle %s, square (%g, %g) +- %g: %d, want %d" % (tc.tolist(), cx, cy, half, got, want)
            seen[want] += 1
    assert min(seen.values()) > 50, seen
