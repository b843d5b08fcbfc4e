// displaced_surface.hip.h -- the surface point of a displaced hit as a renderer needs it: what computeSurfacePoint takes from a
// DisplacedSurfaceAttributes hit in the reference (tfdm/tfdm_shared.h:544-696) and what its G-buffer pass stores for such a
// pixel (tfdm/gpu_kernels/optix_gbuffer_kernels.cu:161-243).  Shared by k_gbuffer_resolve_scene (restir.hip), the path tracer's
// vertices on a displaced surface (pathtrace.hip) and the tests (tests/displaced_host.cpp).
//
// Inputs: a gfx_scene_hit of a displaced instance (world distance, base barycentrics, world normal), the world ray, the texture
// coordinates and texCoord0Dir of the three base vertices (the geometry gfx_scene_bind_displaced names) and the instance's
// InstanceRecord.  The position is org + dist * dir of the WORLD ray (tfdm_shared.h:575-576); geometric and shading normal are
// both the hit's normal; the tangent is texCoord0Dir interpolated on the base triangle, taken to world space by objToWorld and
// made orthogonal to the normal, with the reference's two fallbacks (a normal that is not finite becomes +z with tangent +x; a
// tangent that is not finite becomes makeCoordinateSystem's).
//
// G-buffer encoding of a displaced pixel (include/gfxexp.h): gbuffer0.instSlot = GFX_GBUFFER_DISPLACED | set index.  The motion
// vector follows a moved instance: prevPositionInWorld = curToPrev * positionInWorld (optix_gbuffer_kernels.cu:230), with the
// instance's row of the set's motion table (tfdm_instance.hip.h make_cur_to_prev; the exact identity for an instance that did not
// move, which gives prevPositionInWorld = positionInWorld and the words of the form without a matrix).
//
// Under the math contract of tfdm_core.hip.h.  The polar quantiser and the camera projection need acos / atan2 / tan: they are the
// algorithms of the "gm" contract, version 1 (gm_math.hip.h: Cody-Waite reduction + minimax kernels, every multiply-add spelled
// fmaf), restated here in plain C++ so that g++ compiles them too; the device passes encode a plain pixel with gm_math.hip.h's and
// a displaced one with these, to the same bits for the same direction.
#pragma once
#include "tfdm_instance.hip.h"

namespace gfx {
namespace tfdm {

constexpr uint32_t kGbufferDisplaced = 0x80000000u;      // GFX_GBUFFER_DISPLACED

// ---------------------------------------------------------------- the "gm" transcendental contract, version 1
constexpr float kDsPi = 3.14159265358979323846f;
constexpr float kDsTwoPi = 2 * 3.14159265358979323846f;
constexpr float kDsHalfPi = 1.5707963705062866f;
constexpr float kDsQuarterPi = 0.7853981852531433f;
GFX_TFDM_FN bool ds_finite(float x) { return (f2b(x) & 0x7F800000u) != 0x7F800000u; }
GFX_TFDM_FN bool ds_finite(V3 a) { return ds_finite(a.x) && ds_finite(a.y) && ds_finite(a.z); }
GFX_TFDM_FN uint32_t ds_f2u_sat(float x) {
    if (!(x > 0.0f)) return 0u;
    if (x >= 4294967296.0f) return 0xFFFFFFFFu;
    return static_cast<uint32_t>(x);
}
GFX_TFDM_FN void ds_sincos(float x, float& s, float& c) {
    const float q = rintf(x * 0.6366197466850281f);
    float r = fmaf(q, -1.5703125f, x);
    r = fmaf(q, -0.0004837512969970703f, r);
    r = fmaf(q, -7.549790126404332e-08f, r);
    const int32_t n = !(q == q) ? 0 : q >= 2147483648.0f ? 2147483647 : q <= -2147483648.0f ? -2147483647 - 1 : static_cast<int32_t>(q);
    const float r2 = r * r;
    float ps = fmaf(-1.9515295891e-4f, r2, 8.3321608736e-3f);
    ps = fmaf(ps, r2, -1.6666654611e-1f);
    const float sr = fmaf(ps * r2, r, r);
    float pc = fmaf(2.443315711809948e-5f, r2, -1.388731625493765e-3f);
    pc = fmaf(pc, r2, 4.166664568298827e-2f);
    const float cr = fmaf(pc * r2, r2, fmaf(-0.5f, r2, 1.0f));
    const float ss = (n & 1) ? cr : sr;
    const float cc = (n & 1) ? sr : cr;
    s = (n & 2) ? -ss : ss;
    c = ((n + 1) & 2) ? -cc : cc;
}
GFX_TFDM_FN float ds_tan(float x) { float s, c; ds_sincos(x, s, c); return s / c; }
GFX_TFDM_FN float ds_asin_core(float x) {
    const float z = x * x;
    float p = fmaf(4.2163199048e-2f, z, 2.4181311049e-2f);
    p = fmaf(p, z, 4.5470025998e-2f);
    p = fmaf(p, z, 7.4953002686e-2f);
    p = fmaf(p, z, 1.6666752422e-1f);
    return fmaf(p * z, x, x);
}
GFX_TFDM_FN float ds_acos(float x) {
    if (x > 0.5f) return 2.0f * ds_asin_core(sqrtf(0.5f * (1.0f - x)));
    if (x < -0.5f) return kDsPi - 2.0f * ds_asin_core(sqrtf(0.5f * (1.0f + x)));
    return kDsHalfPi - ds_asin_core(x);
}
GFX_TFDM_FN float ds_atan_nonneg(float t) {
    float y0 = 0.0f;
    if (t > 2.414213562373095f) { y0 = kDsHalfPi; t = -1.0f / t; }
    else if (t > 0.4142135623730950f) { y0 = kDsQuarterPi; t = (t - 1.0f) / (t + 1.0f); }
    const float z = t * t;
    float p = fmaf(8.05374449538e-2f, z, -1.38776856032e-1f);
    p = fmaf(p, z, 1.99777106478e-1f);
    p = fmaf(p, z, -3.33329491539e-1f);
    return y0 + fmaf(p * z, t, t);
}
GFX_TFDM_FN float ds_atan2(float y, float x) {
    if (x == 0.0f && y == 0.0f) return 0.0f;
    const float ax = fabsf(x), ay = fabsf(y);
    float a = (ax == 0.0f) ? kDsHalfPi : ds_atan_nonneg(ay / ax);
    if (x < 0.0f) a = kDsPi - a;
    return y < 0.0f ? -a : a;
}

// ---------------------------------------------------------------- quantisers (common/common_device.cuh:27-79 as shading.hip.h states them)
GFX_TFDM_FN uint32_t ds_q16(float x01) { const uint32_t q = ds_f2u_sat(x01 * 65535u); return q > 65535u ? 65535u : q; }
GFX_TFDM_FN uint32_t ds_encode_dir(V3 v) {
    const float cy = v.y > -1.0f ? v.y : -1.0f;                 // fmin2(fmax2(v.y, -1), 1) of to_polar_yup, as selects
    const float theta = ds_acos(cy < 1.0f ? cy : 1.0f);
    const float a = ds_atan2(-v.x, v.z) + kDsTwoPi;
    const float phi = a >= kDsTwoPi ? a - kDsTwoPi : a;
    return (ds_q16(theta / kDsPi) << 16) | ds_q16(phi / kDsTwoPi);
}
GFX_TFDM_FN V3 ds_decode_dir(uint32_t q) {
    const float phi = kDsTwoPi * ((q & 0xFFFF) / 65535.0f);
    const float theta = kDsPi * ((q >> 16) / 65535.0f);
    float sp, cp, st, ct;
    ds_sincos(phi, sp, cp);
    ds_sincos(theta, st, ct);
    return v3(-sp * st, ct, cp * st);
}
GFX_TFDM_FN uint32_t ds_encode_uv(float u, float v) { return (ds_q16(v - floorf(v)) << 16) | ds_q16(u - floorf(u)); }

// ---------------------------------------------------------------- the surface point
struct BaseVertex { V3 texCoord0Dir; float u, v; };    // what a displaced pixel takes from a vertex of its base triangle

struct DisplacedPoint {
    V3 position;         // org + dist * dir
    V3 normal;           // geometric = shading normal, world space
    V3 tangent;          // unit, orthogonal to the normal
    float u, v;          // texture coordinate of the base point
};

GFX_TFDM_FN void ds_make_coordinate_system(V3 normal, V3& tangent, V3& bitangent) {      // common_shared.h:92-100
    const float sign = normal.z >= 0 ? 1.0f : -1.0f;
    const float a = -1 / (sign + normal.z);
    const float b = normal.x * normal.y * a;
    tangent = v3(1 + sign * normal.x * normal.x * a, sign * b, -sign * normal.x);
    bitangent = v3(b, sign + normal.y * normal.y * a, -normal.y);
}

// Tangent and texture coordinate on the base triangle for a world normal `n` (the hit's, or the one a G-buffer holds); applies
// the two fallbacks, the first of which replaces `n`.
GFX_TFDM_FN void displaced_frame(const InstanceRecord& r, const BaseVertex& a, const BaseVertex& b, const BaseVertex& c, float bcB, float bcC, V3& n, V3& tangent,
                                 float& u, float& v) {
    const float bcA = 1 - (bcB + bcC);
    const V3 tcObj = bcA * a.texCoord0Dir + bcB * b.texCoord0Dir + bcC * c.texCoord0Dir;
    u = bcA * a.u + bcB * b.u + bcC * c.u;
    v = bcA * a.v + bcB * b.v + bcC * c.v;
    V3 t = mul3(r.objToWorld, 4, tcObj);
    t = normalize(t - dot(n, t) * n);
    if (!ds_finite(n)) { n = v3(0.0f, 0.0f, 1.0f); t = v3(1.0f, 0.0f, 0.0f); }
    if (!ds_finite(t)) { V3 bt; ds_make_coordinate_system(n, t, bt); }
    tangent = t;
}

GFX_TFDM_FN DisplacedPoint displaced_point(const InstanceRecord& r, const SceneHit& h, V3 org, V3 dir, const BaseVertex& a, const BaseVertex& b, const BaseVertex& c) {
    DisplacedPoint p;
    p.position = org + h.dist * dir;
    p.normal = h.normal;
    displaced_frame(r, a, b, c, h.bcB, h.bcC, p.normal, p.tangent, p.u, p.v);
    return p;
}

// ---------------------------------------------------------------- the G-buffer words of a displaced pixel
struct DisplacedGBuffer {
    uint32_t g0[4];      // gfx_gbuffer0: GFX_GBUFFER_DISPLACED | set index, bound geometry, base triangle, qbcB | qbcC << 16
    float mv[2];         // gfx_gbuffer1
    float position[3];   // gfx_gbuffer2
    uint32_t qGeometricNormal;
    uint32_t g3[4];      // gfx_gbuffer3: qShadingNormal, qShadingTangent, qTexCoord, matSlot
};

// PerspectiveCamera::calcScreenPosition (restir_di_shared.h:51-59) of `pw` under `cam`, then the motion vector of pixel (x, y):
// current raster position minus the previous one.  Matrix3x3::invert as gm_math.hip.h states it.
GFX_TFDM_FN void displaced_motion_vector(const gfx_camera& cam, V3 pw, int x, int y, float imageSizeX, float imageSizeY, bool resetFlow, float& mvx, float& mvy) {
    const float a = cam.orientation[0], b = cam.orientation[1], c = cam.orientation[2], d = cam.orientation[3], e = cam.orientation[4], f = cam.orientation[5],
                g = cam.orientation[6], h = cam.orientation[7], i = cam.orientation[8];
    const float det = a * e * i + b * f * g + c * d * h - c * e * g - b * d * i - a * f * h;
    const float rd = 1 / det;
    const float inv[9] = { (e * i - f * h) * rd, -(b * i - c * h) * rd, (b * f - c * e) * rd, -(d * i - f * g) * rd, (a * i - c * g) * rd, -(a * f - c * d) * rd,
                           (d * h - e * g) * rd, -(a * h - b * g) * rd, (a * e - b * d) * rd };
    const V3 pv = mul3(inv, 3, pw - v3(cam.position[0], cam.position[1], cam.position[2]));
    const float ax = pv.x / pv.z, ay = pv.y / pv.z;
    const float hh = 2 * ds_tan(cam.fovY / 2);
    const float ww = cam.aspect * hh;
    const float sx = 1 - (ax + 0.5f * ww) / ww;
    const float sy = 1 - (ay + 0.5f * hh) / hh;
    mvx = (x + 0.5f) - sx * imageSizeX;
    mvy = (y + 0.5f) - sy * imageSizeY;
    if (resetFlow || pw.x != pw.x) { mvx = 0.0f; mvy = 0.0f; }
}

// Where the world point `p` of an instance was before its last move: xfm_point of gm_math.hip.h (the arithmetic of the plain
// pixel's prevPositionInWorld, restir.hip gbuffer_resolve) with the instance's curToPrev, row-major 3 x 4.
GFX_TFDM_FN V3 displaced_prev_position(const float* m, V3 p) {
    return v3(m[0] * p.x + m[1] * p.y + m[2] * p.z + m[3] * 1.0f, m[4] * p.x + m[5] * p.y + m[6] * p.z + m[7] * 1.0f,
              m[8] * p.x + m[9] * p.y + m[10] * p.z + m[11] * 1.0f);
}

// curToPrev: the instance's row of the motion table; nullptr: an instance that never moved (prevPositionInWorld = positionInWorld)
GFX_TFDM_FN DisplacedGBuffer displaced_gbuffer(const DisplacedPoint& p, const SceneHit& h, uint32_t geomInstSlot, uint32_t matSlot, const gfx_camera& prevCamera,
                                               int x, int y, float imageSizeX, float imageSizeY, bool resetFlow, const float* curToPrev = nullptr) {
    DisplacedGBuffer g;
    g.g0[0] = kGbufferDisplaced | (h.where >> 1);
    g.g0[1] = geomInstSlot;
    g.g0[2] = h.index;
    g.g0[3] = ds_q16(h.bcB) | (ds_q16(h.bcC) << 16);
    const V3 prevPosition = curToPrev ? displaced_prev_position(curToPrev, p.position) : p.position;
    displaced_motion_vector(prevCamera, prevPosition, x, y, imageSizeX, imageSizeY, resetFlow, g.mv[0], g.mv[1]);
    g.position[0] = p.position.x; g.position[1] = p.position.y; g.position[2] = p.position.z;
    g.qGeometricNormal = ds_encode_dir(p.normal);
    g.g3[0] = g.qGeometricNormal;
    g.g3[1] = ds_encode_dir(p.tangent);
    g.g3[2] = ds_encode_uv(p.u, p.v);
    g.g3[3] = matSlot;
    return g;
}

} // namespace tfdm
} // namespace gfx
