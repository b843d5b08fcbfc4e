"""The shading layer's definitions in numpy float64, written from the model and sharing no code with the oracle (oracle/orc_shared.h)
or the device (gfxexp_amd/csrc/shading.hip.h).  tests/test_bsdf_cpu.py holds the oracle against these; fp32 inputs are widened exactly
(float32 -> float64 is exact) before anything is computed.

The model.  A material is (type, a, b, smoothness): type 0 is a Lambertian reflector of albedo a; type 1 has diffuse colour a, specular
F0 b and roughness 1 - min(smoothness, 0.999); type 2 is the metallic workflow with base colour a, roughness max(b.y, 0.001),
metallic b.z: diffuse = a (1 - metallic), F0 = 0.04 (1 - metallic) + a metallic.  Types 1 and 2 are one BRDF in the local frame
(normal = +z), for directions on the same side of the surface, mirrored to the upper side:
    alpha = roughness^2, h = normalize(l + v)
    D(h)      = alpha^2 / (pi cos^4(th_h) (alpha^2 + tan^2(th_h))^2)                      GGX
    Lambda(w) = (-1 + sqrt(1 + alpha^2 tan^2(th_w))) / 2,  G1(w, h) = chi+(w.h / w.z) / (1 + Lambda(w))
    G(l, v)   = chi+(l.h / l.z) chi+(v.h / v.z) / (1 + Lambda(l) + Lambda(v))             height-correlated Smith
    F         = F0 + (1 - F0) (1 - l.h)^5                                                 Schlick, F90 = 1
    f_spec    = F D G / (4 l.z v.z)
    f_diff    = a / pi * (1 + (FD90 - 1)(1 - l.z)^5) (1 + (FD90 - 1)(1 - v.z)^5) * mix(1, 1/1.51, roughness),  FD90 = roughness / 2 + 2 roughness (l.h)^2
Sampling picks the diffuse lobe (cosine hemisphere) with probability wD / (wD + wS) and the specular lobe (visible normals of the GGX,
reflected) otherwise; the density of a direction is the mixture, with the Jacobian 1 / (4 |l.h|) of the reflection."""
import numpy as np

PI = np.pi
LUMA = np.array([0.2126729, 0.7151522, 0.0721750])     # the published luminance weights of linear sRGB, to the digits the model states


def widen(x):
    x = np.asarray(x)
    assert x.dtype == np.float32
    return x.astype(np.float64)


def normalize(v):
    return v / np.sqrt(np.sum(v * v, axis=-1, keepdims=True))


def dot(a, b):
    return np.sum(a * b, axis=-1)


def mix(a, b, t):
    return a * (1 - t) + b * t


# ---------------------------------------------------------------- materials
def setup(mtype, a, b, smoothness):
    """-> diffuse [n, 3], F0 [n, 3], roughness [n]."""
    mtype = np.asarray(mtype)
    a, b, smoothness = widen(a), widen(b), widen(smoothness)
    s999 = float(np.float32(0.999))                       # the clamp is an fp32 constant of the model
    diffuse, f0, rough = a.copy(), np.zeros_like(a), np.ones(len(a))
    t1, t2 = mtype == 1, mtype == 2
    f0[t1] = b[t1]
    rough[t1] = 1 - np.minimum(smoothness[t1], s999)
    metallic = b[t2, 2:3]
    diffuse[t2] = a[t2] * (1 - metallic)
    f0[t2] = float(np.float32(0.16)) * 0.25 * (1 - metallic) + a[t2] * metallic
    rough[t2] = 1 - np.minimum(1 - b[t2, 1], s999)
    return diffuse, f0, rough


# ---------------------------------------------------------------- GGX
def tan2(w):
    return (w[..., 0] ** 2 + w[..., 1] ** 2) / w[..., 2] ** 2


def ggx_d(alpha, h):
    with np.errstate(all="ignore"):
        c2 = h[..., 2] ** 2
        d = alpha ** 2 / (PI * c2 ** 2 * (alpha ** 2 + tan2(h)) ** 2)
    return np.where(h[..., 2] > 0, d, 0.0)


def smith_lambda(alpha, w):
    with np.errstate(all="ignore"):
        return (-1 + np.sqrt(1 + alpha ** 2 * tan2(w))) / 2


def chi_plus(w, h):
    with np.errstate(all="ignore"):
        return (dot(w, h) / w[..., 2] > 0).astype(np.float64)


def smith_g1(alpha, w, h):
    return chi_plus(w, h) / (1 + smith_lambda(alpha, w))


def smith_g2(alpha, l, v, h):
    return chi_plus(l, h) * chi_plus(v, h) / (1 + smith_lambda(alpha, l) + smith_lambda(alpha, v))


def visible_normal_pdf(alpha, v, h):
    with np.errstate(all="ignore"):
        return smith_g1(alpha, v, h) * np.abs(dot(v, h)) * ggx_d(alpha, h) / np.abs(v[..., 2])


# ---------------------------------------------------------------- the BRDF
def _upper(v_given, v_sampled):
    flip = np.where(v_given[..., 2:3] >= 0, 1.0, -1.0)
    return v_given * flip, v_sampled * flip


def evaluate(mtype, diffuse, f0, rough, v_given, v_sampled):
    """f(v_given, v_sampled) [n, 3]; 0 for directions on opposite sides (or in the surface)."""
    mtype = np.asarray(mtype)
    same = v_given[..., 2] * v_sampled[..., 2] > 0
    v, l = _upper(v_given, v_sampled)
    alpha = rough ** 2
    with np.errstate(all="ignore"):
        h = normalize(l + v)
        lh = dot(l, h)
        g = smith_g2(alpha, l, v, h)
        fres = f0 + (1 - f0) * ((1 - lh) ** 5)[:, None]
        spec = fres * (ggx_d(alpha, h) * g / (4 * l[..., 2] * v[..., 2]))[:, None]
        spec = np.where((g == 0)[:, None], 0.0, spec)
        fd90 = 0.5 * rough + 2 * rough * lh ** 2
        f_in = 1 + (fd90 - 1) * (1 - l[..., 2]) ** 5
        f_out = 1 + (fd90 - 1) * (1 - v[..., 2]) ** 5
        diff = diffuse * (f_in * f_out * mix(1.0, 1 / 1.51, rough) / PI)[:, None]
        val = np.where((mtype == 0)[:, None], diffuse / PI, diff + spec)
    undefined = np.isnan(v_given[..., 2] * v_sampled[..., 2])
    return np.where(undefined[:, None], np.nan, np.where(same[:, None], val, 0.0))


def lobe_weights(diffuse, f0, rough, v_given):
    """(wDiff, wSpec) [n] for the view direction: luminance-weighted expected reflectances of the two lobes."""
    c = np.abs(v_given[..., 2])
    ef = 1 + (0.5 * rough + 2 * rough * c ** 2 - 1) * (1 - c) ** 5
    w_d = (diffuse @ LUMA) * ef ** 2 * mix(1.0, 1 / 1.51, rough)
    w_s = mix(f0 @ LUMA, 1.0, (1 - c) ** 5)
    return w_d, w_s


def pdf(mtype, diffuse, f0, rough, v_given, v_sampled):
    """The density with which sample() returns v_sampled [n], for directions on the same side of the surface."""
    mtype = np.asarray(mtype)
    v, l = _upper(v_given, v_sampled)
    w_d, w_s = lobe_weights(diffuse, f0, rough, v_given)
    with np.errstate(all="ignore"):
        h = normalize(l + v)
        p_spec = visible_normal_pdf(rough ** 2, v, h) / (4 * np.abs(dot(l, h)))
        p = (w_d * l[..., 2] / PI + w_s * p_spec) / (w_d + w_s)
        p = np.where(w_d + w_s == 0, 0.0, p)
    same = v_given[..., 2] * v_sampled[..., 2] > 0
    undefined = np.isnan(v_given[..., 2] * v_sampled[..., 2])
    return np.where(undefined, np.nan, np.where(mtype == 0, np.where(same, np.abs(v_sampled[..., 2]) / PI, 0.0), p))


def dh_reflectance(mtype, diffuse, f0, rough, v_given):
    """The cheap estimate of the directional-hemispherical reflectance [n, 3], clamped to 1."""
    mtype = np.asarray(mtype)
    c = np.abs(v_given[..., 2])
    ef = 1 + (0.5 * rough + 2 * rough * c ** 2 - 1) * (1 - c) ** 5
    d = diffuse * (ef * mix(1.0, 1 / 1.51, rough))[:, None]
    t = ((1 - c) ** 5 * (1 - rough))[:, None]
    s = f0 + (1 - f0) * t
    return np.where((mtype == 0)[:, None], diffuse, np.minimum(d + s, 1.0))


# ---------------------------------------------------------------- hemisphere sampling
def concentric_disk(u0, u1):
    """Shirley-Chiu: the square [0, 1)^2 onto the unit disk, concentric squares onto concentric circles; -> (x, y)."""
    sx, sy = 2 * u0 - 1, 2 * u1 - 1
    with np.errstate(all="ignore"):
        right_or_top = sx >= -sy
        first = sx > sy
        # the four wedges, counter-clockwise from the one around +x: r is the square's "radius", the angle runs linearly along its side
        r = np.where(right_or_top, np.where(first, sx, sy), np.where(first, -sy, -sx))
        oct_ = np.where(right_or_top, np.where(first, sy / sx, 2 - sx / sy), np.where(first, 6 + sx / sy, 4 + sy / sx))
    phi = oct_ * (PI / 4)
    x, y = r * np.cos(phi), r * np.sin(phi)
    centre = (sx == 0) & (sy == 0)
    return np.where(centre, 0.0, x), np.where(centre, 0.0, y)


def cosine_hemisphere(u0, u1):
    """Malley: the disk sample lifted to the hemisphere; density cos / pi."""
    x, y = concentric_disk(u0, u1)
    return np.stack([x, y, np.sqrt(np.maximum(0.0, 1 - x * x - y * y))], axis=-1)


def sample_visible_normal(alpha, v, u0, u1):
    """Visible-normal sampling of the GGX (Heitz 2017): stretch the view direction to the hemisphere configuration, sample the
    projected area of the hemisphere (a half disk and a squeezed half disk, chosen by u1 against 1 / (1 + stretched z)), lift,
    unstretch.  v on the upper side.  -> h [n, 3]."""
    alpha = np.asarray(alpha)[..., None]
    s = normalize(v * np.concatenate([alpha, alpha, np.ones_like(alpha)], axis=-1))
    with np.errstate(all="ignore"):
        d = np.sqrt(s[..., 0] ** 2 + s[..., 1] ** 2)
        tilted = s[..., 2] < float(np.float32(0.9999))
        t1 = np.where(tilted[:, None], np.stack([s[..., 1] / d, -s[..., 0] / d, np.zeros_like(d)], axis=-1), np.array([1.0, 0.0, 0.0]))
        t2 = np.cross(t1, s)
        t2[..., 2] = d                                     # the model states the basis with the exact 2D length as its third component
        a = 1 / (1 + s[..., 2])
        r = np.sqrt(u0)
        lower = u1 < a
        phi = PI * np.where(lower, u1 / a, 1 + (u1 - a) / (1 - a))
        p1 = r * np.cos(phi)
        p2 = r * np.sin(phi) * np.where(lower, 1.0, s[..., 2])
        n = p1[:, None] * t1 + p2[:, None] * t2 + np.sqrt(np.maximum(0.0, 1 - p1 * p1 - p2 * p2))[:, None] * s
    return normalize(n * np.concatenate([alpha, alpha, np.ones_like(alpha)], axis=-1))


def sample(mtype, diffuse, f0, rough, v_given, u0, u1):
    """-> dict(direction [n, 3], density [n], throughput [n, 3] = f cos / density, accepted [n] bool, specular [n] bool (the lobe
    picked), margin [n]: |sum u1 - wDiff| / sum, the distance of u1 from the lobe boundary).  Rejected samples (the reflected direction
    is below the surface, or both weights are 0) have density 0 and throughput 0."""
    mtype = np.asarray(mtype)
    n = len(mtype)
    lam = mtype == 0
    flip = np.where(v_given[..., 2:3] >= 0, 1.0, -1.0)
    v = v_given * flip
    w_d, w_s = lobe_weights(diffuse, f0, rough, v_given)
    total = w_d + w_s
    with np.errstate(all="ignore"):
        spec_lobe = ~(total * u1 < w_d) & ~lam
        margin = np.abs(total * u1 - w_d) / total
        u1_d = np.where(lam, u1, total * u1 / w_d)
        u1_s = (total * u1 - w_d) / w_s
        l_d = cosine_hemisphere(u0, np.where(spec_lobe, 0.5, u1_d))
        h = sample_visible_normal(rough ** 2, v, u0, np.where(spec_lobe, u1_s, 0.5))
        l_s = 2 * np.minimum(dot(v, h), 1.0)[:, None] * h - v
        l = np.where(spec_lobe[:, None], l_s, l_d)
        accepted = np.where(lam, True, (total != 0) & ~(spec_lobe & ~(l[..., 2] * v[..., 2] > 0)))
        l_world = np.where(lam[:, None], l * np.where(v_given[..., 2:3] <= 0, [1.0, 1.0, -1.0], [1.0, 1.0, 1.0]), l * flip)
        dens = np.where(lam, l[..., 2] / PI, pdf(mtype, diffuse, f0, rough, v, l))
        thr = evaluate(np.where(lam, 1, mtype), diffuse, f0, rough, v, l) * (l[..., 2] / dens)[:, None]
        thr = np.where(lam[:, None], diffuse, thr)
    dens = np.where(accepted, dens, 0.0)
    thr = np.where(accepted[:, None], thr, 0.0)
    l_world = np.where(accepted[:, None], l_world, 0.0) if n else l_world
    return dict(direction=l_world, density=dens, throughput=thr, accepted=accepted, specular=spec_lobe, margin=margin, reflected_z=l_s[..., 2])


# ---------------------------------------------------------------- frames
def coordinate_system(n):
    """The branchless orthonormal basis of Duff et al. 2017 (tangent, bitangent) for a unit normal."""
    s = np.where(n[..., 2] >= 0, 1.0, -1.0)
    with np.errstate(all="ignore"):
        a = -1 / (s + n[..., 2])
        b = n[..., 0] * n[..., 1] * a
        t = np.stack([1 + s * n[..., 0] ** 2 * a, s * b, -s * n[..., 0]], axis=-1)
        bt = np.stack([b, s + n[..., 1] ** 2 * a, -n[..., 1]], axis=-1)
    return t, bt


def quat_rotate(q, v):
    """v rotated by the unit quaternion q = (x, y, z, w)."""
    u, w = q[..., :3], q[..., 3:4]
    return v + 2 * np.cross(u, np.cross(u, v) + w * v)


def bump_quaternion(mod):
    """The half-angle quaternion that tilts +z toward the direction of mod: axis (-y, x, 0) / |(x, y)|, angle atan(|(x, y)| / z)."""
    with np.errstate(all="ignore"):
        p = np.sqrt(mod[..., 0] ** 2 + mod[..., 1] ** 2)
        half = np.arctan(p / mod[..., 2]) / 2
        s = np.sin(half)
        q = np.stack([-mod[..., 1] / p * s, mod[..., 0] / p * s, np.zeros_like(p), np.cos(half)], axis=-1)
    return q, p


def bump_frame(n, t, mod):
    """Frame (t, b = n x t, n) with the bump normal mod (given in that frame) applied: the tangent and the bitangent are rotated by the
    quaternion, the normal is mod carried out of the frame as it is.  Unchanged where mod's tilt is below 1e-3.  -> t, b, n [n, 3]."""
    b = np.cross(n, t)
    q, p = bump_quaternion(mod)
    out = lambda v: v[..., 0:1] * t + v[..., 1:2] * b + v[..., 2:3] * n
    ex, ey = np.zeros_like(mod), np.zeros_like(mod)
    ex[..., 0], ey[..., 1] = 1, 1
    keep = (p.astype(np.float32) < np.float32(1e-3))[:, None]            # the threshold compares fp32 numbers in the model
    with np.errstate(all="ignore"):
        return (np.where(keep, t, out(quat_rotate(q, ex))), np.where(keep, b, out(quat_rotate(q, ey))), np.where(keep, n, out(mod)))


def to_local(t, b, n, v):
    return np.stack([dot(t, v), dot(b, v), dot(n, v)], axis=-1)


def from_local(t, b, n, v):
    return v[..., 0:1] * t + v[..., 1:2] * b + v[..., 2:3] * n


# ---------------------------------------------------------------- direct lighting
def direct_lighting(mtype, diffuse, f0, rough, point, v_out, n, t, emittance, position, normal, at_infinity):
    """-> dict(dir, dist2, tmax, rgb, weight): the unshadowed contribution f Le / pi cos_l |cos_s| / d^2 of a light sample with a
    Lambertian emitter of radiant exitance `emittance`; 0 for a light seen from behind its own normal.  Lights at infinity give their
    direction as the position and count d = |position|."""
    inf = np.asarray(at_infinity).astype(bool)
    d = np.where(inf[:, None], position, position - point)
    dist2 = dot(d, d)
    with np.errstate(all="ignore"):
        dist = np.sqrt(dist2)
        w = d / dist[:, None]
        tmax = np.where(inf, float(np.float32(1e10)), dist) * float(np.float32(0.9999))
        w_local = to_local(t, np.cross(n, t), n, w)
        cos_l = dot(-w, normal)
        f = evaluate(mtype, diffuse, f0, rough, v_out, w_local)
        rgb = f * (emittance / PI) * (cos_l * np.abs(w_local[..., 2]) / dist2)[:, None]
        lit = cos_l > 0
    rgb = np.where(lit[:, None], rgb, 0.0)
    return dict(dir=w, dist2=dist2, tmax=tmax, rgb=rgb, weight=rgb.sum(axis=-1) / 3, lit=lit, cos_l=cos_l)
