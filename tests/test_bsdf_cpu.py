"""CPU: the oracle copy of the shading layer (oracle/orc_shared.h: BSDF, GGX helpers, concentricSampleDisk, cosineSampleHemisphere,
makeCoordinateSystem, ReferenceFrame, applyBumpMapping; oracle/orc_scene.h: performDirectLighting) against the float64 statement of the
definitions in tests/bsdf_ref.py, over the lists of tests/bsdf_cases.py.  tests/test_gpu_bsdf.py holds the device copy equal to the oracle,
bit for bit, on the same lists.

Values are held to a bound on the INTERIOR lists only (unit directions with |cos| >= 1/16 on both sides, roughness >= 1/16).  Errors are in
ulp: units of the fp32 spacing of the reference value, with the spacing of the smallest normal as its floor, as in
test_math_contract_cpu.py.  For a vector that is a direction (sampled directions, frame vectors, mapped probe vectors, the shadow ray) the
reference value is the vector: the unit is the spacing of its largest component, since a component near zero carries the absolute error of
the others.  Colours, densities and weights are taken per component.  MEASURED[...] is the worst error of the oracle over exactly these
lists on the host this was written on; the assertion is four times that (the light sampler's convention), which leaves room for another
x86-64 host's differently scheduled build and still fails a wrong factor.  No interior case is skipped and no interior result may be NaN.

On ALL lists, edge lists included, the results are held to structure: where float64 is finite the oracle is finite and non-negative, and
it is zero where the model is zero."""
import functools

import numpy as np
import pytest

from tests import bsdf_cases as BC
from tests import bsdf_ref as R

F, U = np.float32, np.uint32
FLT_MIN = float(np.finfo(F).tiny)
FACTOR = 4.0

# key -> the worst figure measured on the oracle (ulp unless the key says otherwise); the assertion is FACTOR times it.
# DESIGN.md ("The shading layer on its own") repeats the table per function.
MEASURED = {
    "SETUP diffuse": 0.0, "SETUP specularF0": 0.5, "SETUP roughness": 0.0, "EVALUATE rgb [DS]": 14.09, "EVALUATE rgb [DS-00]": 223800,
    "EVALUATE rgb [DS-a0]": 16.44, "EVALUATE rgb [DS-b0]": 13.96, "EVALUATE rgb [DS-r>1]": 8.004, "EVALUATE rgb [L]": 1.147,
    "EVALUATE rgb [PBR]": 18.87, "PDF density [DS]": 13.34, "PDF density [DS-00]": 12.12, "PDF density [DS-a0]": 14.6, "PDF density [DS-b0]": 10.98,
    "PDF density [DS-r>1]": 10.13, "PDF density [L]": 0.9646, "PDF density [PBR]": 16.2, "DHR rgb [DS]": 3.62, "DHR rgb [DS-00]": 7.024,
    "DHR rgb [DS-a0]": 4.835, "DHR rgb [DS-b0]": 3.131, "DHR rgb [DS-r>1]": 11810, "DHR rgb [L]": 0.0, "DHR rgb [PBR]": 5.006,
    "SAMPLE direction [DS]": 116.6, "SAMPLE direction [DS-00]": 153.3, "SAMPLE direction [DS-a0]": 87.3, "SAMPLE direction [DS-b0]": 463.1,
    "SAMPLE direction [DS-r>1]": 152.3, "SAMPLE direction [L]": 98.31, "SAMPLE direction [PBR]": 79.78, "SAMPLE density [DS]": 2099,
    "SAMPLE density [DS-00]": 107.4, "SAMPLE density [DS-a0]": 74.22, "SAMPLE density [DS-b0]": 1445, "SAMPLE density [DS-r>1]": 1527,
    "SAMPLE density [L]": 16030, "SAMPLE density [PBR]": 4125, "SAMPLE throughput [DS]": 86610, "SAMPLE throughput [DS-00]": 398500,
    "SAMPLE throughput [DS-a0]": 44660, "SAMPLE throughput [DS-b0]": 6259, "SAMPLE throughput [DS-r>1]": 12530, "SAMPLE throughput [L]": 0.0,
    "SAMPLE throughput [PBR]": 52970, "SAMPLE density = PDF(returned) [DS]": 253.6, "SAMPLE density = PDF(returned) [DS-00]": 169.0,
    "SAMPLE density = PDF(returned) [DS-a0]": 150.6, "SAMPLE density = PDF(returned) [DS-b0]": 184.1,
    "SAMPLE density = PDF(returned) [DS-r>1]": 7.806, "SAMPLE density = PDF(returned) [L]": 0.9643, "SAMPLE density = PDF(returned) [PBR]": 258.0,
    "SAMPLE throughput x density = f cos [DS]": 49.09, "SAMPLE throughput x density = f cos [DS-00]": 579000,
    "SAMPLE throughput x density = f cos [DS-a0]": 48.86, "SAMPLE throughput x density = f cos [DS-b0]": 40.36,
    "SAMPLE throughput x density = f cos [DS-r>1]": 16.03, "SAMPLE throughput x density = f cos [L]": 1.705,
    "SAMPLE throughput x density = f cos [PBR]": 31.61, "COSINE_HEMISPHERE disk": 9.849, "COSINE_HEMISPHERE direction": 633.7,
    "COORDINATE_SYSTEM tangent": 2.181, "COORDINATE_SYSTEM bitangent": 2.175, "COORDINATE_SYSTEM orthonormality / 2^-23": 1.508,
    "BUMP_FRAME tangent": 5.885, "BUMP_FRAME bitangent": 5.755, "BUMP_FRAME normal": 2.294, "BUMP_FRAME to_local(probe)": 5.869,
    "BUMP_FRAME from_local(probe)": 5.59, "BUMP_FRAME orthonormality / 2^-23": 3.877, "BUMP_FRAME normal = from_local(modNormal)": 2.46,
    "BUMP_FRAME to_local(from_local(probe)) = probe": 8.0, "DIRECT_LIGHTING dir": 2.616, "DIRECT_LIGHTING dist2": 2.835,
    "DIRECT_LIGHTING tmax": 2.107, "DIRECT_LIGHTING rgb [DS]": 78.7, "DIRECT_LIGHTING rgb [DS-00]": 393200, "DIRECT_LIGHTING rgb [DS-a0]": 57.92,
    "DIRECT_LIGHTING rgb [DS-b0]": 59.71, "DIRECT_LIGHTING rgb [DS-r>1]": 23.76, "DIRECT_LIGHTING rgb [L]": 18.25, "DIRECT_LIGHTING rgb [PBR]": 60.25,
    "DIRECT_LIGHTING weight [DS]": 69.92, "DIRECT_LIGHTING weight [DS-00]": 265300, "DIRECT_LIGHTING weight [DS-a0]": 49.82,
    "DIRECT_LIGHTING weight [DS-b0]": 49.2, "DIRECT_LIGHTING weight [DS-r>1]": 22.15, "DIRECT_LIGHTING weight [L]": 16.45,
    "DIRECT_LIGHTING weight [PBR]": 38.8,
    # largest deviation of a (cos theta, phi) cell's share from the integral of the density over it, over the three view cosines (absolute)
    "HISTOGRAM share [L]": 2.193e-05, "HISTOGRAM share [DS]": 4.450e-05, "HISTOGRAM share [DS-black]": 3.633e-05,
    "HISTOGRAM share [DS-rough]": 2.513e-05, "HISTOGRAM share [PBR]": 3.670e-05,
}


def ulp_err(got, ref):
    at = np.maximum(np.abs(ref).astype(F), F(FLT_MIN))
    return np.abs(got.astype(np.float64) - ref) / np.spacing(at).astype(np.float64)


def vec_ulp_err(got, ref):
    """Error of a direction-like vector [n, 3] in units of the fp32 spacing of the reference's largest component: [n]."""
    at = np.maximum(np.max(np.abs(ref), axis=1).astype(F), F(FLT_MIN))
    return np.max(np.abs(got.astype(np.float64) - ref), axis=1) / np.spacing(at).astype(np.float64)


class Figures(dict):
    """Collects the worst error per key and prints it with the element that produced it."""
    def add(self, key, err, c=None, classes=None):
        err = np.asarray(err, np.float64)
        if err.ndim == 2:
            err = np.max(err, axis=1)
        assert len(err) > 0, key
        assert not np.any(np.isnan(err)), f"{key}: {np.count_nonzero(np.isnan(err))} results are NaN, first at element {int(np.flatnonzero(np.isnan(err))[0])}"
        groups = [(key, np.arange(len(err)))] if classes is None else [(f"{key} [{k}]", np.flatnonzero(classes == k)) for k in np.unique(classes)]
        for name, idx in groups:
            i = int(idx[np.argmax(err[idx])])
            where = "" if c is None else "  " + ", ".join(f"{k}={v[i][:3].tolist()}" for k, v in c.items() if v is not None and k != "C")
            print(f"{name:<46s} worst {err[i]:.5g} at element {i}{where}   [{len(idx)} cases]")
            self[name] = max(self.get(name, 0.0), float(err[i]))


def hold(figures):
    """Every figure is within FACTOR times the measured one, and every measured one was produced."""
    for key, v in figures.items():
        assert key in MEASURED, f"{key}: no measured figure recorded; this run gives {v:.5g}"
        assert v <= FACTOR * MEASURED[key], f"{key}: {v:.5g} exceeds {FACTOR:g} x the measured {MEASURED[key]:.5g}"


def material_of(c):
    mat = c["mat"]
    t = BC.material_type(mat)
    d, f0, r = R.setup(t, mat[:, 1:4], mat[:, 4:7], mat[:, 7])
    return t, d, f0, r


def w3(c, k):
    return R.widen(np.ascontiguousarray(c[k][:, :3]))


@functools.lru_cache(maxsize=None)
def oracle(fn, name):
    out = BC.oracle_out(fn, BC.LISTS[fn][name]())
    out.setflags(write=False)
    return out


# ================================================================ values on the interior lists
def measure_setup():
    c = BC.setup_materials()
    o = oracle("SETUP", "materials")
    t, d, f0, r = material_of(c)
    fig = Figures()
    fig.add("SETUP diffuse", ulp_err(o[:, 0:3], d)); fig.add("SETUP specularF0", ulp_err(o[:, 3:6], f0)); fig.add("SETUP roughness", ulp_err(o[:, 6], r))
    return fig


def measure_evaluate():
    c = BC.pairs_interior()
    t, d, f0, r = material_of(c)
    cls = BC.material_class(c["mat"])
    fig = Figures()
    fig.add("EVALUATE rgb", ulp_err(oracle("EVALUATE", "interior"), R.evaluate(t, d, f0, r, w3(c, "A"), w3(c, "B"))), c, cls)
    same = c["A"][:, 2] * c["B"][:, 2] > 0                 # the density is defined for directions on one side of the surface
    ref = R.pdf(t, d, f0, r, w3(c, "A"), w3(c, "B"))
    fig.add("PDF density", ulp_err(oracle("PDF", "interior")[same, 0], ref[same]), BC_part(c, same), cls[same])
    return fig


def BC_part(c, m):
    return {k: (None if v is None else v[m]) for k, v in c.items()}


def measure_dhr():
    c = BC.dhr_interior()
    t, d, f0, r = material_of(c)
    fig = Figures()
    fig.add("DHR rgb", ulp_err(oracle("DHR", "interior"), R.dh_reflectance(t, d, f0, r, w3(c, "A"))), c, BC.material_class(c["mat"]))
    return fig


def sample_reference(c):
    t, d, f0, r = material_of(c)
    u = R.widen(c["B"])
    return (t, d, f0, r), R.sample(t, d, f0, r, w3(c, "A"), u[:, 0], u[:, 1])


BORDERLINE_Z = 1e-4
BORDERLINE_SHARE = 1e-3


def measure_sample():
    """The sampler against the float64 construction, and against its own value and density recomputed in float64 from the direction it
    returned.  Whether a specular sample is rejected follows float64, except where the float64 reflected z is within 1e-4 of zero."""
    c = BC.sample_interior()
    o = oracle("SAMPLE", "interior")
    (t, d, f0, r), ref = sample_reference(c)
    cls = BC.material_class(c["mat"])
    fig = Figures()
    accepted = o[:, 6] > 0
    borderline = ref["specular"] & (np.abs(ref["reflected_z"]) < BORDERLINE_Z)
    differ = accepted != ref["accepted"]
    assert not np.any(differ & ~borderline), f"SAMPLE: {np.count_nonzero(differ & ~borderline)} samples are accepted on one side only, first at {int(np.flatnonzero(differ & ~borderline)[0])}"
    share = np.count_nonzero(borderline) / len(o)
    print(f"SAMPLE interior: {np.count_nonzero(borderline)} borderline of {len(o)} ({share:.2e}), {np.count_nonzero(differ)} decided differently; rejected {np.count_nonzero(~accepted)}")
    assert share <= BORDERLINE_SHARE
    rej = ~accepted & ~differ
    assert not np.any(o[rej][:, [0, 1, 2, 6]]), "SAMPLE: a rejected sample has a throughput or a density"
    both = accepted & ref["accepted"]
    m = BC_part(c, both)
    fig.add("SAMPLE direction", vec_ulp_err(o[both, 3:6], ref["direction"][both]), m, cls[both])
    fig.add("SAMPLE density", ulp_err(o[both, 6], ref["density"][both]), m, cls[both])
    fig.add("SAMPLE throughput", ulp_err(o[both, 0:3], ref["throughput"][both]), m, cls[both])
    # its own value and density, from the direction it returned
    vg, l = w3(c, "A")[both], R.widen(o[both, 3:6])
    tt, dd, ff, rr = t[both], d[both], f0[both], r[both]
    f = R.evaluate(tt, dd, ff, rr, vg, l)
    p = R.pdf(tt, dd, ff, rr, vg, l)
    fig.add("SAMPLE density = PDF(returned)", ulp_err(o[both, 6], p), m, cls[both])
    lam = (tt == 0)[:, None]
    want = np.where(lam, dd * np.abs(l[:, 2:3]) / np.pi, f * np.abs(l[:, 2:3]))       # Lambert: throughput = albedo = f cos / (cos / pi)
    fig.add("SAMPLE throughput x density = f cos", ulp_err(o[both, 0:3] * o[both, 6:7], want), m, cls[both])
    return fig


def measure_hemisphere():
    c = BC.hemisphere_grid()
    o = oracle("COSINE_HEMISPHERE", "grid")
    u = R.widen(c["A"])
    x, y = R.concentric_disk(u[:, 0], u[:, 1])
    fig = Figures()
    fig.add("COSINE_HEMISPHERE disk", vec_ulp_err(np.concatenate([o[:, 0:2], o[:, 0:1] * 0], axis=1), np.stack([x, y, 0 * x], axis=1)), c)
    fig.add("COSINE_HEMISPHERE direction", vec_ulp_err(o[:, 2:5], R.cosine_hemisphere(u[:, 0], u[:, 1])), c)
    return fig


def orthonormality(t, b, n):
    """The largest of |t.t - 1|, |b.b - 1|, |n.n - 1|, |t.b|, |t.n|, |b.n|, in units of 2^-23."""
    t, b, n = (R.widen(np.ascontiguousarray(v)) for v in (t, b, n))
    dev = np.stack([R.dot(t, t) - 1, R.dot(b, b) - 1, R.dot(n, n) - 1, R.dot(t, b), R.dot(t, n), R.dot(b, n)], axis=1)
    return np.max(np.abs(dev), axis=1) / 2.0 ** -23


def measure_frames():
    fig = Figures()
    c = BC.normals_random()
    o = oracle("COORDINATE_SYSTEM", "random")
    n = w3(c, "A")
    t, b = R.coordinate_system(n)
    fig.add("COORDINATE_SYSTEM tangent", vec_ulp_err(o[:, 0:3], t), c); fig.add("COORDINATE_SYSTEM bitangent", vec_ulp_err(o[:, 3:6], b), c)
    fig.add("COORDINATE_SYSTEM orthonormality / 2^-23", orthonormality(o[:, 0:3], o[:, 3:6], c["A"][:, :3]), c)
    c = BC.bump_interior()
    o = oracle("BUMP_FRAME", "interior")
    mod, probe = R.widen(c["C"][:, 0:3]), R.widen(c["C"][:, 4:7])
    rt, rb, rn = R.bump_frame(w3(c, "A"), w3(c, "B"), mod)
    for k, (name, ref) in enumerate((("tangent", rt), ("bitangent", rb), ("normal", rn), ("to_local(probe)", R.to_local(rt, rb, rn, probe)),
                                     ("from_local(probe)", R.from_local(rt, rb, rn, probe)))):
        fig.add("BUMP_FRAME " + name, vec_ulp_err(o[:, 3 * k:3 * k + 3], ref), c)
    fig.add("BUMP_FRAME orthonormality / 2^-23", orthonormality(o[:, 0:3], o[:, 3:6], o[:, 6:9]), c)
    # the frame's own maps, in float64 on the vectors it returned: the normal is from_local(modNormal), and to_local undoes from_local
    ft, fb, fn_ = (R.widen(o[:, 3 * k:3 * k + 3]) for k in range(3))
    before = R.from_local(*(R.widen(v) for v in (c["B"][:, :3], np.cross(c["A"][:, :3].astype(np.float64), c["B"][:, :3].astype(np.float64)).astype(F), c["A"][:, :3])), mod)
    fig.add("BUMP_FRAME normal = from_local(modNormal)", vec_ulp_err(o[:, 6:9], before), c)
    fig.add("BUMP_FRAME to_local(from_local(probe)) = probe", vec_ulp_err(R.to_local(ft, fb, fn_, R.widen(o[:, 12:15])).astype(F), probe), c)
    return fig


def lighting_reference(c):
    t, d, f0, r = material_of(c)
    C = R.widen(c["C"])
    return R.direct_lighting(t, d, f0, r, w3(c, "A"), w3(c, "B"), C[:, 0:3], C[:, 4:7], C[:, 8:11], C[:, 12:15], C[:, [3, 7, 11]],
                             np.ascontiguousarray(c["C"][:, 15]).view(U))


def measure_lighting():
    c = BC.lighting_interior()
    o = oracle("DIRECT_LIGHTING", "interior")
    ref = lighting_reference(c)
    cls = BC.material_class(c["mat"])
    fig = Figures()
    fig.add("DIRECT_LIGHTING dir", vec_ulp_err(o[:, 0:3], ref["dir"]), c)
    fig.add("DIRECT_LIGHTING dist2", ulp_err(o[:, 3], ref["dist2"]), c); fig.add("DIRECT_LIGHTING tmax", ulp_err(o[:, 4], ref["tmax"]), c)
    assert np.all(ref["lit"]) and np.all(np.any(ref["rgb"] > 0, axis=1) | ~np.any(c["mat"][:, 1:7] != 0, axis=1))
    fig.add("DIRECT_LIGHTING rgb", ulp_err(o[:, 5:8], ref["rgb"]), c, cls); fig.add("DIRECT_LIGHTING weight", ulp_err(o[:, 8], ref["weight"]), c, cls)
    return fig


MEASURES = {"setup": measure_setup, "evaluate_pdf": measure_evaluate, "dhr": measure_dhr, "sample": measure_sample, "hemisphere": measure_hemisphere,
            "frames": measure_frames, "lighting": measure_lighting}


@pytest.mark.parametrize("what", list(MEASURES))
def test_interior_values_against_float64(what):
    fig = MEASURES[what]()
    hold(fig)
    stale = [k for k in MEASURED if k.split(" ")[0] in {f.split(" ")[0] for f in fig} and k not in fig and not k.startswith("HISTOGRAM")]
    assert not stale, f"measured figures without a check: {stale}"


# ================================================================ structure on all lists
def finite_rows(*refs):
    return np.all(np.stack([np.all(np.isfinite(r.reshape(len(r), -1)), axis=1) for r in refs]), axis=0)


def in_range(*vs):
    """Vectors whose squared length fp32 can form without underflow or overflow to 0 / inf (a 1e-20 vector is finite in float64 only)."""
    with np.errstate(all="ignore"):
        return np.all(np.stack([(np.sum(v * v, axis=1) > 1e-30) & (np.sum(v * v, axis=1) < 1e30) for v in vs]), axis=0)


def assert_structure(what, got, ref, c, zero=None, where=None):
    """Where float64 is finite and non-negative (the model itself goes negative for colours and roughness outside [0, 1]): got is finite
    and non-negative; where `zero` (float64's verdict) holds, got is exactly 0, elsewhere got is zero only where float64 is (an
    underflow to 0 of a float64 value below the smallest fp32 normal is no disagreement)."""
    got = got.reshape(len(got), -1)
    ref = ref.reshape(len(ref), -1)
    ok = finite_rows(ref) & np.all(ref >= 0, axis=1) & (True if where is None else where)
    bad = ok & ~np.all(np.isfinite(got) & (got >= 0), axis=1)
    assert not np.any(bad), f"{what}: {np.count_nonzero(bad)} results are not finite and non-negative where float64 is, first {got[np.flatnonzero(bad)[0]]} at " \
                            f"{ {k: v[np.flatnonzero(bad)[0]].tolist() for k, v in c.items() if v is not None and k != 'C'} }"
    if zero is not None:
        z = ok & zero
        assert not np.any(got[z]), f"{what}: {np.count_nonzero(np.any(got[z] != 0, axis=1))} results are not 0 where the model is"
        nz = ok & ~zero & np.all(ref > FLT_MIN, axis=1)
        bad = nz & np.any(got == 0, axis=1)
        assert not np.any(bad), f"{what}: {np.count_nonzero(bad)} results are 0 where the model is not, first at element {int(np.flatnonzero(bad)[0])}"
    return int(np.count_nonzero(ok))


@pytest.mark.parametrize("name", ["interior", "edge"])
def test_structure_of_evaluate_pdf_dhr(name):
    c = BC.LISTS["EVALUATE"][name]()
    t, d, f0, r = material_of(c)
    vg, vs = w3(c, "A"), w3(c, "B")
    ref = R.evaluate(t, d, f0, r, vg, vs)
    with np.errstate(all="ignore"):
        v, l = R._upper(vg, vs)
        g = R.smith_g2(r ** 2, l, v, R.normalize(l + v))
    opposite = ~(vg[:, 2] * vs[:, 2] > 0)
    rng = in_range(vg, vs)
    # Recorded behaviour: evaluate() does not clamp l.h at 1 (sample_throughput does), so for vSampled = vGiven, where the fp32 l.h can
    # round above 1, the Schlick term (1 - l.h)^5 is a negative number of magnitude below (2^-22)^5 and a material with F0 = 0 returns
    # a negative value of that order.  Those pairs are held to "finite" and to the bound |f| < 1e-20 instead of to the sign.
    with np.errstate(all="ignore"):
        coincident = (1 - R.dot(l, R.normalize(l + v)) < 1e-6) & ~np.any(f0 != 0, axis=1) & (t != 0)
    got = oracle("EVALUATE", name)
    unit = (np.abs(np.sum(vg * vg, axis=1) - 1) < 1e-5) & (np.abs(np.sum(vs * vs, axis=1) - 1) < 1e-5)
    sel = coincident & unit & finite_rows(ref)
    assert np.all(np.isfinite(got[sel])) and np.all(got[sel] > -1e-20)
    rng &= ~coincident
    n = assert_structure(f"EVALUATE on {name}", oracle("EVALUATE", name), ref, c, zero=opposite | np.all(ref == 0, axis=1), where=rng)
    black_spec = opposite | ((t != 0) & (g == 0) & ~np.any(d != 0, axis=1))         # G == 0 leaves the diffuse lobe alone
    assert not np.any(oracle("EVALUATE", name)[finite_rows(ref) & black_spec & rng])
    same = ~opposite
    p = R.pdf(t, d, f0, r, vg, vs)
    n2 = assert_structure(f"PDF on {name}", oracle("PDF", name)[same], p[same], BC_part(c, same), where=rng[same])
    cd = BC.LISTS["DHR"][name]()
    td, dd, fd, rd = material_of(cd)
    ref = R.dh_reflectance(td, dd, fd, rd, w3(cd, "A"))
    n3 = assert_structure(f"DHR on {name}", oracle("DHR", name), ref, cd, where=in_range(w3(cd, "A")))
    assert np.all(oracle("DHR", name)[finite_rows(ref) & (td != 0)] <= 1)
    print(f"{name}: float64 finite on {n} EVALUATE, {n2} PDF, {n3} DHR elements")


@pytest.mark.parametrize("name", list(BC.LISTS["SAMPLE"]))
def test_structure_of_sample(name):
    c = BC.LISTS["SAMPLE"][name]()
    o = oracle("SAMPLE", name)
    (t, d, f0, r), ref = sample_reference(c)
    allref = np.concatenate([ref["throughput"], ref["density"][:, None]], axis=1)
    unit_view = np.abs(np.sum(w3(c, "A") ** 2, axis=1) - 1) < 1e-6
    ok = finite_rows(allref, ref["direction"]) & unit_view
    bad = ok & ~(np.all(np.isfinite(o), axis=1) & np.all(o[:, [0, 1, 2, 6]] >= 0, axis=1))
    assert not np.any(bad), f"SAMPLE on {name}: {np.count_nonzero(bad)} results are not finite and non-negative where float64 is, first {o[np.flatnonzero(bad)[0]]} at " \
                            f"element {int(np.flatnonzero(bad)[0])}: {describe(c, int(np.flatnonzero(bad)[0]))}"
    acc = o[:, 6] > 0
    unit = np.abs(np.sum(R.widen(o[:, 3:6]) ** 2, axis=1) - 1) < 1e-5
    assert np.all(unit[acc & ok]), f"SAMPLE on {name}: an accepted sample's direction is not unit"
    same_side = o[:, 5] * c["A"][:, 2] >= 0                # = 0: the cosine-hemisphere direction of u0 -> 1 lies in the horizon, with throughput 0
    assert np.all(same_side[acc & ok & (t != 0)]), f"SAMPLE on {name}: an accepted sample leaves on the other side of the surface"
    assert not np.any(o[acc & ok & (o[:, 5] == 0)][:, 0:3]), f"SAMPLE on {name}: a sample in the horizon carries throughput"
    print(f"SAMPLE on {name}: float64 finite on {np.count_nonzero(ok)} of {len(o)}, accepted {np.count_nonzero(acc)}")


def describe(c, i):
    return ", ".join(f"{k} = {v[i].tolist()}" for k, v in c.items() if v is not None)


def test_structure_of_frames_and_lighting():
    for name in BC.LISTS["BUMP_FRAME"]:
        c = BC.LISTS["BUMP_FRAME"][name]()
        o = oracle("BUMP_FRAME", name)
        mod = c["C"][:, 0:3]
        with np.errstate(all="ignore"):
            flat = np.sqrt(mod[:, 0] * mod[:, 0] + mod[:, 1] * mod[:, 1]) < F(1e-3)                # fp32, as the model states it
        nrm, t = c["A"][:, :3], c["B"][:, :3]
        untouched = np.concatenate([t, np.stack([nrm[:, 1] * t[:, 2] - nrm[:, 2] * t[:, 1], nrm[:, 2] * t[:, 0] - nrm[:, 0] * t[:, 2],
                                                 nrm[:, 0] * t[:, 1] - nrm[:, 1] * t[:, 0]], axis=1).astype(F), nrm], axis=1)
        assert np.array_equal(o[flat, 0:9].view(U), untouched[flat].view(U)), f"BUMP_FRAME on {name}: a tilt below 1e-3 changed the frame"
        rt, rb, rn = R.bump_frame(w3(c, "A"), w3(c, "B"), R.widen(mod))
        ok = finite_rows(rt, rb, rn)
        assert np.all(np.isfinite(o[ok, 0:9])), f"BUMP_FRAME on {name}: not finite where float64 is"
        assert np.any(flat) or name == "interior"
    for name in BC.LISTS["DIRECT_LIGHTING"]:
        c = BC.LISTS["DIRECT_LIGHTING"][name]()
        o = oracle("DIRECT_LIGHTING", name)
        ref = lighting_reference(c)
        allref = np.concatenate([ref["rgb"], ref["weight"][:, None], ref["dist2"][:, None], ref["tmax"][:, None]], axis=1)
        with np.errstate(all="ignore"):
            dark = ~(ref["cos_l"] > 0) | np.all(ref["rgb"] == 0, axis=1)
        sure = (np.abs(ref["cos_l"]) > 1e-5) & in_range(w3(c, "B"))                                # the sign of lpCos is float64's away from 0
        assert_structure(f"DIRECT_LIGHTING on {name}", o[sure][:, [5, 6, 7, 8, 3, 4]], allref[sure], BC_part(c, sure))
        got_dark = ~np.any(o[:, 5:9] != 0, axis=1)
        ok = finite_rows(allref) & sure
        behind = ok & ~(ref["cos_l"] > 0)
        assert np.all(got_dark[behind]) and np.count_nonzero(behind) >= (0 if name == "interior" else 1000)
        lit = ok & ~dark & np.all(ref["rgb"] > FLT_MIN, axis=1)
        assert not np.any(got_dark[lit]), f"DIRECT_LIGHTING on {name}: dark where the model is lit"
        inf = np.ascontiguousarray(c["C"][:, 15]).view(U) != 0
        assert np.all(o[inf, 4] == F(1e10) * F(0.9999))


# ================================================================ the sampler's directions follow its density
N_COS, N_PHI = 16, 32


@functools.lru_cache(maxsize=None)
def histogram_materials():
    """One material per class of the interior: L, DS (smoothness 0.6), DS without a diffuse lobe, DS of roughness 1.5, PBR (0.5, 0.5)."""
    m = BC.materials_interior()
    t = BC.material_type(m)
    pick = [0, int(np.flatnonzero((t == 1) & (m[:, 7] == F(0.6)))[0]), int(np.flatnonzero((t == 1) & ~np.any(m[:, 1:4] != 0, axis=1))[0]),
            int(np.flatnonzero((t == 1) & (m[:, 7] == F(-0.5)))[0]), int(np.flatnonzero((t == 2) & (m[:, 5] == F(0.5)) & (m[:, 6] == F(0.5)))[0])]
    return ("L", "DS", "DS-black", "DS-rough", "PBR"), m[pick]


def cell_integrals(mat1, view, sub):
    """The float64 integral of the reference density over each (cos theta, phi) cell: the cell is cut into sub x sub pieces with an
    8 x 8 Gauss-Legendre rule on each: [N_COS, N_PHI]."""
    x, w = np.polynomial.legendre.leggauss(8)
    order = 8 * sub
    cz = ((np.arange(N_COS * sub)[:, None] + (x[None, :] + 1) / 2) / (N_COS * sub)).ravel()       # cos theta nodes
    wz = np.tile(w / 2 / (N_COS * sub), N_COS * sub)
    ph = ((np.arange(N_PHI * sub)[:, None] + (x[None, :] + 1) / 2) / (N_PHI * sub)).ravel() * 2 * np.pi
    wp = np.tile(w / 2 / (N_PHI * sub), N_PHI * sub) * 2 * np.pi
    Z, P = np.meshgrid(cz, ph, indexing="ij")
    s = np.sqrt(1 - Z * Z)
    l = np.stack([s * np.cos(P), s * np.sin(P), Z], axis=-1).reshape(-1, 3)
    n = len(l)
    mat = np.tile(mat1, (n, 1))
    t = BC.material_type(mat)
    d, f0, r = R.setup(t, mat[:, 1:4], mat[:, 4:7], mat[:, 7])
    p = R.pdf(t, d, f0, r, np.tile(R.widen(view), (n, 1)), l).reshape(len(cz), len(ph)) * wz[:, None] * wp[None, :]
    return p.reshape(N_COS, order, N_PHI, order).sum(axis=(1, 3))


HIST_CASES = [(k, c) for k in range(5) for c in BC.HISTOGRAM_VIEW_COS]


@pytest.mark.parametrize("k,view_cos", HIST_CASES, ids=[f"{('L', 'DS', 'DS-black', 'DS-rough', 'PBR')[k]}-cos{c:g}" for k, c in HIST_CASES])
def test_sampled_directions_follow_the_density(k, view_cos):
    """The 1024 x 1024 stratified grid through the oracle's sampler, binned on 16 (cos theta) x 32 (phi) cells: each cell's share is the
    float64 integral of the reference density over the cell, the rejected share is one minus the sum of those integrals, and that sum --
    the integral of the density over the upper hemisphere -- is at most 1."""
    names, mats = histogram_materials()
    from oracle import oracle as O
    u = BC.stratified_grid()
    view = BC.view_of_cos(view_cos)
    n = len(u)
    o = O.bsdf_eval_materials(np.tile(mats[k], (n, 1)), 2, np.tile(view, (n, 1)), BC.a4(u)[:, :3])
    acc = o[:, 6] > 0
    l = o[acc, 3:6].astype(np.float64)
    assert np.all(l[:, 2] > 0)
    iz = np.minimum((l[:, 2] * N_COS).astype(np.int64), N_COS - 1)
    ip = np.minimum((np.mod(np.arctan2(l[:, 1], l[:, 0]), 2 * np.pi) / (2 * np.pi) * N_PHI).astype(np.int64), N_PHI - 1)
    share = np.bincount(iz * N_PHI + ip, minlength=N_COS * N_PHI).reshape(N_COS, N_PHI) / n
    want = cell_integrals(mats[k], view, 8)
    key = f"HISTOGRAM share [{names[k]}]"
    tol = FACTOR * MEASURED.get(key, 0.0)
    coarse = cell_integrals(mats[k], view, 4)
    quad = float(np.max(np.abs(want - coarse)))
    dev = float(np.max(np.abs(share - want)))
    rejected = 1 - np.count_nonzero(acc) / n
    total = float(want.sum())
    print(f"{key} cos {view_cos:g}: worst cell deviation {dev:.3e}, quadrature moved by {quad:.3e}, rejected {rejected:.6f}, 1 - integral {1 - total:.6f}")
    assert key in MEASURED, f"{key}: no measured figure recorded; this run gives {dev:.3e}"
    assert quad <= tol / 10, f"{key}: halving the quadrature moves a cell by {quad:.3e}, more than a tenth of the tolerance {tol:.3e}"
    assert dev <= tol, f"{key}: a cell's share deviates by {dev:.3e}, tolerance {tol:.3e}"
    assert total <= 1 + 1e-9
    assert abs(rejected - (1 - total)) <= tol, f"{key}: rejected share {rejected:.6f} against 1 - integral of the density {1 - total:.6f}"


# ================================================================ NaN counts
def test_nan_words_are_the_recorded_ones():
    got = {(fn, name): BC.nan_words(oracle(fn, name)) for fn, lists in BC.LISTS.items() for name in lists}
    assert got == BC.NAN_WORDS, {k: (v, BC.NAN_WORDS.get(k)) for k, v in got.items() if BC.NAN_WORDS.get(k) != v}
    # the largest random numbers with unit view directions above the surface: nothing is NaN (ggxSample clamps its radicand)
    assert got[("SAMPLE", "u-edge")] == 0 and got[("SAMPLE", "u0-top")] == 0
    for fn in BC.LISTS:
        for name in BC.LISTS[fn]:
            if name in ("interior", "grid", "random", "materials"):
                assert got[(fn, name)] == 0, (fn, name)
