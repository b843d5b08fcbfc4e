"""No GPU: the C ABI of ReGIR over a bound set of displaced instances (GFX_DISPLACED_REGIR, gfx_pt_last_nee_rays, gfx_tfdm_set_bounds)
is declared in the header, exported by the library and mirrored in api.py; and the numpy cell-index helper the GPU test relies on
(tests/displaced_regir_host.py) is held against hand-worked positions, ones outside the grid and exactly on faces among them."""
import os
import re

import numpy as np

from gfxexp_amd import api
from tests import displaced_regir_host as G

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gfxexp.h")


def _header():
    with open(HEADER) as f:
        return f.read()


def _prototype(name):
    m = re.search(r"^int\s+%s\s*\(([^;]*)\)\s*;" % name, _header(), re.M)
    assert m, "%s is not declared in include/gfxexp.h" % name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def _define(name):
    m = re.search(r"^#define\s+%s\s+(0x[0-9A-Fa-f]+|\d+)u?\b" % name, _header(), re.M)
    assert m, "%s is not defined in include/gfxexp.h" % name
    return int(m.group(1), 0)


def test_the_new_entries_are_declared_exported_and_mirrored(built_lib):
    assert _prototype("gfx_pt_last_nee_rays") == ["gfx_ctx* ctx", "void* stream", "void* dRayOrgTmin", "void* dRayDirTmax", "void* dOccluded", "void* dOwnerPixel",
                                                  "uint32_t capacity", "uint32_t* count"]
    assert _prototype("gfx_tfdm_set_bounds") == ["gfx_tfdm_set* set", "float lo[3]", "float hi[3]"]
    for name in ("gfx_pt_last_nee_rays", "gfx_tfdm_set_bounds"):
        assert hasattr(built_lib, name), "%s is not exported by libgfxexp.so" % name
        assert name in api.C_ABI_SYMBOLS
    assert callable(api.Context.pt_last_nee_rays) and callable(api.TfdmSet.bounds)
    for fn in (api.Context.bind_displaced, api.Context.bind_displaced_kinds):
        assert "regir" in fn.__code__.co_varnames and "restir" in fn.__code__.co_varnames


def test_the_bit_is_eight_and_four_stays_unassigned():
    assert api.DISPLACED_REGIR == _define("GFX_DISPLACED_REGIR") == 8
    assert api.DISPLACED_GBUFFER_PT == _define("GFX_DISPLACED_GBUFFER_PT") == 1
    assert api.DISPLACED_RESTIR == _define("GFX_DISPLACED_RESTIR") == 2
    values = [int(v, 0) for v in re.findall(r"^#define\s+GFX_DISPLACED_\w+\s+(0x[0-9A-Fa-f]+|\d+)u?\b", _header(), re.M)]
    assert sorted(values) == [1, 2, 8], "bit 4 is pinned as an unknown bit by the existing refusal tests"


# ---------------------------------------------------------------- the cell helper
ORIGIN = np.array([-2.0, -1.5, 0.0], np.float32)
CELL = np.array([0.75, 1.25, 0.5], np.float32)          # all exact in float32, so positions on faces are exact too
DIMS = (8, 4, 6)


def _index(ix, iy, iz):
    return iz * DIMS[0] * DIMS[1] + iy * DIMS[0] + ix


def test_cell_index_inside_on_faces_and_outside_the_grid():
    f = np.float32
    cases = [((-2.0, -1.5, 0.0), (0, 0, 0)),                         # the grid's corner
             ((-1.7, -1.0, 0.2), (0, 0, 0)),
             ((-1.25, -0.25, 0.5), (1, 1, 1)),                      # exactly on three inner faces: the cell above each
             ((np.nextafter(f(-1.25), f(-2)), -0.25, 0.5), (0, 1, 1)),
             ((0.0, 0.0, 1.3), (2, 1, 2)),
             ((3.9, 3.4, 2.9), (7, 3, 5)),
             ((4.0, 3.5, 3.0), (7, 3, 5)),                          # exactly on the outer faces: index dims, clamped
             ((100.0, -100.0, 7.0), (7, 0, 5)),                     # outside: clamps to the border cells
             ((-2.5, 9.0, -0.1), (0, 3, 0)),
             ((3.0e38, -3.0e38, 1.0e30), (7, 0, 5)),
             ((np.inf, -np.inf, np.nan), (7, 0, 0))]                # the saturating conversion: +inf -> 2^32 - 1, -inf and NaN -> 0
    pos = np.array([c[0] for c in cases], np.float32)
    want = np.array([c[1] for c in cases], np.uint32)
    got = G.cell_coords(pos, ORIGIN, CELL, DIMS)
    assert np.array_equal(got, want), "\n%s\n%s" % (got, want)
    assert np.array_equal(G.cell_index(pos, ORIGIN, CELL, DIMS), np.array([_index(*c[1]) for c in cases], np.uint32))


def test_cell_index_is_the_float32_division():
    """A position whose float64 quotient is below a face and whose float32 quotient is on it goes to the cell above, as the device's
    correctly rounded float32 division puts it."""
    origin, cell = np.array([0.0, 0.0, 0.0], np.float32), np.array([0.1, 1.0, 1.0], np.float32)
    x = np.float32(0.5)
    assert float(x) / float(cell[0]) < 5.0 and np.float32(x) / cell[0] == np.float32(5.0)
    assert G.cell_coords([(x, 0.5, 0.5)], origin, cell, (8, 2, 2))[0, 0] == 5


def test_near_inner_face_counts_inner_faces_only():
    eps = 1e-3
    pos = np.array([(-1.25, 0.3, 0.2),                               # on the inner face x = -1.25
                    (-1.25 + 0.9e-3, 0.3, 0.2), (-1.25 - 0.9e-3, 0.3, 0.2),
                    (-1.25 + 1.2e-3, 0.3, 0.2),                      # just outside eps
                    (-2.0, 0.3, 0.2), (4.0, 0.3, 0.2), (-2.0004, 0.3, 0.2), (50.0, 0.3, 0.2),   # outer faces and beyond: never
                    (0.3, 0.3, 2.5 + 0.5e-3),                        # the last inner face in z
                    (0.3, 0.3, 3.0 - 0.5e-3),                        # the outer face in z
                    (0.3, -0.25 - 0.5e-3, 0.2)], np.float32)
    want = np.array([1, 1, 1, 0, 0, 0, 0, 0, 1, 0, 1], bool)
    assert np.array_equal(G.near_inner_face(pos, ORIGIN, CELL, DIMS, eps), want)


def test_count_bounds_bracket_every_perturbation():
    rng = np.random.default_rng(5)
    n = 4000
    pos = (ORIGIN + rng.random((n, 3)) * CELL * DIMS).astype(np.float32)
    pos[:200, 0] = np.float32(-1.25) + (rng.random(200) - 0.5).astype(np.float32) * np.float32(1e-3)      # a cloud on an inner face
    pos[200:260] += (30.0, 0.0, 0.0)                                 # and some outside the grid
    eps = 1e-3
    lo, hi, near = G.cell_count_bounds(pos, ORIGIN, CELL, DIMS, eps)
    assert near[:200].all() and not near[200:260].any() and lo.sum() == n - near.sum() and hi.sum() >= n
    cells = DIMS[0] * DIMS[1] * DIMS[2]
    for _ in range(4):
        moved = (pos + (rng.random((n, 3)) * 2 - 1) * 0.5 * eps).astype(np.float32)
        got = np.bincount(G.cell_index(moved, ORIGIN, CELL, DIMS), minlength=cells)
        assert np.all(lo <= got) and np.all(got <= hi)
    exact = np.bincount(G.cell_index(pos, ORIGIN, CELL, DIMS), minlength=cells)
    assert np.any(lo < exact), "the cloud on the face is what the bounds are loose for"


def test_the_offset_step_bound():
    """Against offsetRayOrigin restated here: 256 integer steps away from zero, or 1 / 65536 near the origin."""
    def offset(p, n):
        p = np.float32(p)
        if abs(p) < 1.0 / 32.0:
            return np.float32(p + np.float32(1.0 / 65536.0) * np.float32(n))
        i = np.array([p], np.float32).view(np.int32)[0] + (-1 if p < 0 else 1) * int(np.float32(256.0) * np.float32(n))
        return np.array([i], np.int32).view(np.float32)[0]
    for m in (0.01, 0.5, 1.0, 3.9999, 4.0, 7.99999, 1000.0, 1400.0):
        bound = G.max_offset_step(m)
        for p in (m, -m, np.nextafter(np.float32(m), np.float32(0)), m / 2, m / 3):
            for n in (1.0, -1.0, 0.3):
                assert abs(float(offset(p, n)) - float(np.float32(p))) <= bound, (m, p, n)
    assert G.max_offset_step(4.0) < 3e-4
