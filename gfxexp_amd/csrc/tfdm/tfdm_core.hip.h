// tfdm_core.hip.h -- tessellation-free displacement mapping: the arithmetic shared by the device kernels (tfdm.hip) and the host
// (tfdm_build.h, tests/tfdm_host.cpp).  A height map displaces a base triangle mesh along its interpolated normals; a ray is
// intersected with the displaced surface without ever building the micro-triangles, by descending a min-max pyramid of the map
// with affine-arithmetic bounds of the surface over each texel.
//
// Restated from the reference in this project's own types:
//     tfdm/affine_arithmetic.h:631-1279            AAFloatOn2D and its 3-vector forms             -> AA, AA3
//     tfdm/tfdm_shared.h:736-897                    Texel, up / down / next, the triangle / square test, findRoots
//     tfdm/gpu_kernels/tfdm_intersection_kernels.h  displacedSurface_generic (Box, TwoTriangle, Bilinear) -> intersect()
//     common/basic_types.h:2602-2609               makeCoordinateSystem                             -> ray_frame()
//     tfdm/gpu_kernels/tfdm_preprocess_kernels.cu   computeTexelMinMax, computeAABBs                 -> texel_min_max(), prim_aabb()
// Where this differs from the reference, on purpose:
//   * ray-independent terms (the inverted texture transform, the composed matrices, the transformed texture coordinates, the
//     roots) are in a per-triangle record made once on the host (tfdm_build.h), not recomputed per intersection call;
//   * the interval of an affine form is rounded outward by bit steps AND widened by 2^-19 of the sum of its coefficient
//     magnitudes: the reference rounds only the final sums outward and lets the fp32 roundings of the ~30 operations in front of
//     them (each 2^-24 relative) go unaccounted; a float64 sampling of the surface finds points outside such a box;
//   * AA3 squared length bounds the error term by dot(|centre|, error) (the reference's |dot(centre, error)| cancels between axes);
//   * recSqrt of an interval that reaches zero, and any bound that is not finite, becomes (-inf, +inf): the box is then always
//     entered instead of being skipped by a NaN comparison;
//   * a ray that starts inside a Box-mode texel box leaves through the face of its smallest far distance (the reference reports
//     the face of the largest near distance there);
//   * texel indices are int32 (int16 in the reference).
// ... and in the Bilinear (Newton) local intersection, newton_bilinear() (kernels.h:362-528):
//   * the distance of a hit is the ray's parameter (the reference returns the length |S - org|, the parameter only for a unit
//     direction; an object-space direction under a scaled instance is not unit);
//   * delta = S - (org + max(t0, tmin) dir), from the ray point at the texel box's entry and not from the origin: F is the same in
//     exact arithmetic, in fp32 its cancellation scales with the texel and not with the ray's length (an absolute 1e-5 criterion
//     against a delta of length 50 would never be met).  The hit's parameter is the entry parameter plus the projected rest.
//     "Behind" stays what it is in the reference, a guess that projects behind the ray's ORIGIN (parameter < 0): the first
//     guesses of a ray that enters the box late project before the box entry although the root lies after it;
//   * a hit counts only with tmin < t < tmax, as in the other modes (the reference checks tMax alone);
//   * bcB, bcC come from the final guess on every path (the reference reads them uninitialised when it converges at iteration 0);
//   * a hit outside the base triangle is rejected by the test of the TwoTriangle branch;
//   * frontFace = dot(dir, normal) <= 0 with both in object space (the reference dots a tangent-space direction with an
//     object-space normal);
//   * the normal is normalize(cross(dS/du, dS/dv)), negated for a record with `flipped` set, so that it lies on the side of +N
//     wherever the height gradient vanishes, as in the other two modes (the reference's cross(dS/dv, dS/du) lies on the side of
//     -N for a footprint of positive area);
//   * a singular 2 x 2 system, or any NaN, ends in "no hit" after at most 10 iterations; nothing that is not finite is written
//     to a hit.
//
// Plain C++17 under the project's math contract: no contraction unless written fmaf (none here), IEEE division and sqrt, from
// libm only sqrtf / fabsf / floorf; min and max are written as selects so that signed zeros and NaNs fall the same way on both
// sides; powers of two are built from their bits.  hipcc compiles it for the device, g++ for the host, to the same bits.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define GFX_TFDM_FN __host__ __device__ __forceinline__
#else
#define GFX_TFDM_FN inline
#endif

namespace gfx {
namespace tfdm {

constexpr uint32_t kInvalid = 0xFFFFFFFFu;
constexpr int kMaxDepth = 13;              // 8192 x 8192 texels: the level offsets below stay inside 32 bits
constexpr int kStackDepth = 24;            // base-tree stack entries per ray (tfdm_build.h builds a balanced tree over <= 2^20 triangles)
constexpr uint32_t kMaxTriangles = 1u << 20;
static_assert((1u << (kStackDepth - 4)) >= kMaxTriangles, "a balanced tree over kMaxTriangles leaves is 20 deep: trace_ray pushes at most one entry per level, and a push beyond kStackDepth would be dropped");
constexpr float kMaxTexelCoord = 16777216.0f;   // |texture coordinate| x map size stays below 2^24: int32 texel indices, exact as floats
enum Local : uint32_t { kBox = 0, kTwoTriangle = 1, kBilinear = 4 };   // gfx_tfdm_local; 2 and 3 are refused at the boundary

// ---------------------------------------------------------------- scalars
GFX_TFDM_FN uint32_t f2b(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
GFX_TFDM_FN float b2f(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
GFX_TFDM_FN float pow2i(int k) { return b2f(static_cast<uint32_t>(127 + k) << 23); }    // 2^k, -126 <= k <= 127
GFX_TFDM_FN float inf() { return b2f(0x7F800000u); }
// std::fmin / std::fmax as the reference uses them (a NaN operand is ignored), as selects
GFX_TFDM_FN float fmin_(float a, float b) { return (a < b || b != b) ? a : b; }
GFX_TFDM_FN float fmax_(float a, float b) { return (a > b || b != b) ? a : b; }
GFX_TFDM_FN float next_up(float x) {
    if (x != x || x == inf()) return x;
    if (x == 0.0f) return b2f(1u);
    const uint32_t u = f2b(x);
    return b2f(x > 0.0f ? u + 1u : u - 1u);
}
GFX_TFDM_FN float next_down(float x) { return -next_up(-x); }
GFX_TFDM_FN int floor_div(int v, int m) { return (v < 0 ? v - (m - 1) : v) / m; }           // common/basic_types.h:273-282
GFX_TFDM_FN int floor_mod(int v, int m) { const int r = v % m; return r < 0 ? r + m : r; }
GFX_TFDM_FN int floor_log2(uint32_t x) { int e = 0; while (x > 1u) { x >>= 1; ++e; } return e; }   // prevPowOf2Exponent

struct V2 { float x, y; };
struct V3 { float x, y, z; };
struct F2 { float lo, hi; };                // one pyramid entry
GFX_TFDM_FN V2 v2(float x, float y) { V2 r; r.x = x; r.y = y; return r; }
GFX_TFDM_FN V3 v3(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
GFX_TFDM_FN V2 operator+(V2 a, V2 b) { return v2(a.x + b.x, a.y + b.y); }
GFX_TFDM_FN V2 operator-(V2 a, V2 b) { return v2(a.x - b.x, a.y - b.y); }
GFX_TFDM_FN V2 operator*(float s, V2 a) { return v2(s * a.x, s * a.y); }
GFX_TFDM_FN float cross2(V2 a, V2 b) { return a.x * b.y - a.y * b.x; }
GFX_TFDM_FN V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
GFX_TFDM_FN V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
GFX_TFDM_FN V3 operator*(float s, V3 a) { return v3(s * a.x, s * a.y, s * a.z); }
GFX_TFDM_FN float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
GFX_TFDM_FN V3 cross(V3 a, V3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
GFX_TFDM_FN V3 normalize(V3 a) { return (1.0f / sqrtf(dot(a, a))) * a; }
GFX_TFDM_FN V3 mul3(const float* m, int stride, V3 a) {        // rows of a row-major matrix with `stride` floats per row
    return v3(m[0] * a.x + m[1] * a.y + m[2] * a.z, m[stride] * a.x + m[stride + 1] * a.y + m[stride + 2] * a.z,
              m[2 * stride] * a.x + m[2 * stride + 1] * a.y + m[2 * stride + 2] * a.z);
}

// ---------------------------------------------------------------- affine arithmetic over two noise symbols (affine_arithmetic.h:631-814)
struct AA { float c, u, v, k; };            // centre, the coefficients of the two symbols, the accumulated error term (>= 0)
struct Interval { float lo, hi; };
GFX_TFDM_FN AA aa(float c, float u = 0.0f, float v = 0.0f, float k = 0.0f) { AA r; r.c = c; r.u = u; r.v = v; r.k = k; return r; }
GFX_TFDM_FN AA operator+(AA a, AA b) { return aa(a.c + b.c, a.u + b.u, a.v + b.v, a.k + b.k); }
GFX_TFDM_FN AA operator-(AA a, AA b) { return aa(a.c - b.c, a.u - b.u, a.v - b.v, a.k + b.k); }
GFX_TFDM_FN AA operator+(AA a, float b) { return aa(a.c + b, a.u, a.v, a.k); }
GFX_TFDM_FN AA operator*(float s, AA a) { return aa(a.c * s, a.u * s, a.v * s, a.k * fabsf(s)); }
GFX_TFDM_FN AA operator*(AA a, AA r) {      // :722-741, the same order of sums
    float p = 0.0f, q = 0.0f;
    p += fabsf(a.u); q += fabsf(r.u);
    const float nu = a.c * r.u + r.c * a.u;
    p += fabsf(a.v); q += fabsf(r.v);
    const float nv = a.c * r.v + r.c * a.v;
    p += a.k; q += r.k;
    float nk = fabsf(r.c) * a.k + fabsf(a.c) * r.k;
    nk += p * q;
    return aa(a.c * r.c, nu, nv, nk);
}
GFX_TFDM_FN Interval to_interval(AA a) {    // :661-669 with __fadd_rd / __fadd_ru as bit steps, then the widening of the header comment
    const float au = fabsf(a.u), av = fabsf(a.v), ak = fabsf(a.k);
    const float slack = next_up(((fabsf(a.c) + au) + (av + ak)) * pow2i(-19));
    Interval r;
    r.lo = next_down(next_down(next_down(next_down(a.c - au) - av) - ak) - slack);
    r.hi = next_up(next_up(next_up(next_up(a.c + au) + av) + ak) + slack);
    if (!(r.lo >= -3.0e38f && r.hi <= 3.0e38f)) { r.lo = -inf(); r.hi = inf(); }
    return r;
}
GFX_TFDM_FN AA affine_approx(AA v, float alpha, float beta, float delta) {   // :642-653
    return aa(alpha * v.c + beta, alpha * v.u, alpha * v.v, delta + fabsf(alpha) * v.k);
}
GFX_TFDM_FN AA reciprocal(AA v) {           // :750-763
    const Interval i = to_interval(v);
    const float a = i.lo, b = i.hi;
    if (!(a > 0.0f || b < 0.0f)) return aa(0.0f, 0.0f, 0.0f, inf());
    const float ab = a * b;
    const float sqrtab = (a > 0.0f ? 1.0f : -1.0f) * sqrtf(ab);
    const float alpha = -1.0f / ab;
    const float beta = (a + 2.0f * sqrtab + b) / (2.0f * ab);
    const float delta = (a - 2.0f * sqrtab + b) / (2.0f * ab);
    return affine_approx(v, alpha, beta, fabsf(delta));
}
GFX_TFDM_FN AA rec_sqrt(AA v) {             // :780-813, the min-range form
    const Interval i = to_interval(v);
    const float a = i.lo, b = i.hi;
    if (!(a > 0.0f) || b == inf()) return aa(0.0f, 0.0f, 0.0f, inf());
    const float fa = 1.0f / sqrtf(a), fb = 1.0f / sqrtf(b);
    const float alpha = -0.5f * (fb * fb * fb);
    const float beta = 0.5f * (fa + fb - alpha * (a + b));
    const float delta = 0.5f * fabsf(fa - fb - alpha * (a - b));
    return affine_approx(v, alpha, beta, delta);
}

struct AA3 { AA x, y, z; };                 // AAFloatOn2D_Vector3D / _Point3D (:910-1167)
GFX_TFDM_FN AA3 aa3(AA x, AA y, AA z) { AA3 r; r.x = x; r.y = y; r.z = z; return r; }
GFX_TFDM_FN AA3 operator+(AA3 a, AA3 b) { return aa3(a.x + b.x, a.y + b.y, a.z + b.z); }
GFX_TFDM_FN AA3 operator*(AA s, AA3 a) { return aa3(a.x * s, a.y * s, a.z * s); }
GFX_TFDM_FN AA dot(V3 a, AA3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }          // :1013-1016
GFX_TFDM_FN AA sq_length(AA3 a) {           // :973-984
    const V3 xc = v3(a.x.c, a.y.c, a.z.c), xu = v3(a.x.u, a.y.u, a.z.u), xv = v3(a.x.v, a.y.v, a.z.v), xk = v3(a.x.k, a.y.k, a.z.k);
    const V3 r = v3(fabsf(xu.x) + fabsf(xv.x) + xk.x, fabsf(xu.y) + fabsf(xv.y) + xk.y, fabsf(xu.z) + fabsf(xv.z) + xk.z);
    const float offset = 0.5f * dot(r, r);
    return aa(dot(xc, xc) + offset, 2.0f * dot(xc, xu), 2.0f * dot(xc, xv), 2.0f * dot(v3(fabsf(xc.x), fabsf(xc.y), fabsf(xc.z)), xk) + offset);
}
GFX_TFDM_FN AA3 normalize(AA3 a) { return rec_sqrt(sq_length(a)) * a; }                    // :985-989
// rows of a row-major 3 x 3 (stride 3) or 3 x 4 (stride 4) matrix times an affine vector (:1250-1259)
GFX_TFDM_FN AA3 mul3(const float* m, int stride, AA3 a) {
    return aa3(dot(v3(m[0], m[1], m[2]), a), dot(v3(m[stride], m[stride + 1], m[stride + 2]), a), dot(v3(m[2 * stride], m[2 * stride + 1], m[2 * stride + 2]), a));
}

// ---------------------------------------------------------------- the per-triangle record, the object's parameters, the map
// Everything of a base triangle that does not depend on the ray (tfdm_build.h make_record: double, rounded to float once).
// Texture coordinates here are AFTER the texture transform; the matrices are composed with it (with its inverse).
struct alignas(16) TriRecord {
    float objToTang[12];     // rows of matObjToTcTang, 3 x 4: object space -> (u, v, height) tangent space       (tfdm_main.cpp:827-830, kernels.h:88-90)
    float tcToN[9];          // rows of matTcToNInObj: (u, v, 1) -> interpolated vertex normal, not normalised    (tfdm_main.cpp:832-834, kernels.h:84)
    float tcToP[9];          // rows of matTcToPInObj: (u, v, 1) -> position on the base triangle                   (kernels.h:82-83)
    float tc[6];             // tcA, tcB, tcC
    float recArea;           // 1 / cross(tcB - tcA, tcC - tcA)
    uint32_t flipped;        // that area is negative
    int32_t rootMinX, rootMinY, rootMaxX, rootMaxY, rootLod;   // findRoots: up to 2 x 2 texels of level rootLod cover the footprint
    uint32_t numRoots;       // 0: degenerate in texture space, never hit
    uint32_t pad[4];
};
static_assert(sizeof(TriRecord) == 192, "TriRecord is 12 x 16 bytes");

struct Params {              // per object, derived from gfx_tfdm_params (tfdm_build.h make_params; kernels.h:54-59)
    float baseHeight;        // hOffset - preScale hScale hBias
    float heightScale;       // preScale hScale, preScale = 1 / sqrt(texScale.x texScale.y)
    int32_t maxDepth;        // log2(size): the level that is one texel
    int32_t targetMipLevel;
    uint32_t local;          // Local
    uint32_t pad[3];
};

// all levels of the height map / of the pyramid lie behind one another, level 0 first; element offset of `level`
GFX_TFDM_FN uint32_t level_offset(int maxDepth, int level) { return ((1u << (2 * (maxDepth + 1))) - (1u << (2 * (maxDepth - level + 1)))) / 3u; }
GFX_TFDM_FN uint32_t total_texels(int maxDepth) { return level_offset(maxDepth, maxDepth + 1); }

struct Map { const float* heights; const F2* pyramid; };

// Height at the corner (px, py) of the texel grid of `level`: include/gfxexp.h's tex2DLod contract at u = px / W with repeat wrap.
// There x = px - 0.5 exactly, so i = px - 1, alpha = beta = 0.5 and the four weights are 0.25: the contract's sum in its order.
GFX_TFDM_FN float corner_height(const float* heights, int maxDepth, int level, int px, int py) {
    const int w = 1 << (maxDepth - level);
    const float* t = heights + level_offset(maxDepth, level);
    const int i0 = floor_mod(px - 1, w), i1 = floor_mod(px, w), j0 = floor_mod(py - 1, w), j1 = floor_mod(py, w);
    return ((0.25f * t[j0 * w + i0] + 0.25f * t[j0 * w + i1]) + 0.25f * t[j1 * w + i0]) + 0.25f * t[j1 * w + i1];
}
// computeTexelMinMax (preprocess_kernels.cu:7-42): min / max of the four corner samples of a texel
GFX_TFDM_FN F2 texel_min_max(const float* heights, int maxDepth, int level, int x, int y) {
    const float a = corner_height(heights, maxDepth, level, x, y), b = corner_height(heights, maxDepth, level, x + 1, y);
    const float c = corner_height(heights, maxDepth, level, x, y + 1), d = corner_height(heights, maxDepth, level, x + 1, y + 1);
    F2 r;
    r.lo = fmin_(fmin_(fmin_(a, b), c), d);
    r.hi = fmax_(fmax_(fmax_(a, b), c), d);
    return r;
}
// generateMinMaxMipMap_generic (:88-131): the four children, then the texel's own corner samples at its own level
GFX_TFDM_FN F2 pyramid_reduce(const float* heights, const F2* pyramid, int maxDepth, int level, int x, int y) {
    const int sw = 1 << (maxDepth - level + 1);
    const F2* src = pyramid + level_offset(maxDepth, level - 1);
    float lo = inf(), hi = -inf();
    F2 m = src[(2 * y) * sw + 2 * x];          lo = fmin_(m.lo, lo); hi = fmax_(m.hi, hi);
    m = src[(2 * y) * sw + 2 * x + 1];         lo = fmin_(m.lo, lo); hi = fmax_(m.hi, hi);
    m = src[(2 * y + 1) * sw + 2 * x];         lo = fmin_(m.lo, lo); hi = fmax_(m.hi, hi);
    m = src[(2 * y + 1) * sw + 2 * x + 1];     lo = fmin_(m.lo, lo); hi = fmax_(m.hi, hi);
    const F2 own = texel_min_max(heights, maxDepth, level, x, y);
    F2 r;
    r.lo = fmin_(lo, own.lo);
    r.hi = fmax_(hi, own.hi);
    return r;
}

// ---------------------------------------------------------------- the stackless texel walk (tfdm_shared.h:736-897)
struct Texel { int x, y, lod; };
GFX_TFDM_FN bool same(Texel a, Texel b) { return a.x == b.x && a.y == b.y && a.lod == b.lod; }
GFX_TFDM_FN void up(Texel& t) { ++t.lod; t.x = floor_div(t.x, 2); t.y = floor_div(t.y, 2); }
GFX_TFDM_FN void down(Texel& t) { --t.lod; t.x *= 2; t.y *= 2; }
GFX_TFDM_FN void down(Texel& t, bool signX, bool signY) { --t.lod; t.x = 2 * t.x + (signX ? 1 : 0); t.y = 2 * t.y + (signY ? 1 : 0); }
// The next texel in ray order: the four children of a texel are visited near to far (signX / signY: the ray travels toward -x / -y);
// behind the last child the walk climbs, and stops climbing above `topLod`.  signX = signY = false is the plain order.
GFX_TFDM_FN void next(Texel& t, bool signX, bool signY, int topLod) {
    const int sx = signX ? 1 : 0, sy = signY ? 1 : 0;
    while (true) {
        const int k = 2 * floor_mod(t.x + sx, 2) + floor_mod(t.y + sy, 2);
        if (k == 1) { t.y += signY ? 1 : -1; t.x += signX ? -1 : 1; return; }
        if (k == 3) { up(t); if (t.lod > topLod) return; continue; }
        t.y += signY ? -1 : 1;
        return;
    }
}

enum Overlap : int { kOutside = 0, kInside = 1, kOverlapping = 2 };
struct Footprint {           // a base triangle in (transformed) texture space
    V2 a, b, c, lo, hi;
    bool flipped;
};
GFX_TFDM_FN Footprint footprint(const TriRecord& r) {
    Footprint f;
    f.a = v2(r.tc[0], r.tc[1]); f.b = v2(r.tc[2], r.tc[3]); f.c = v2(r.tc[4], r.tc[5]);
    f.lo = v2(fmin_(f.a.x, fmin_(f.b.x, f.c.x)), fmin_(f.a.y, fmin_(f.b.y, f.c.y)));
    f.hi = v2(fmax_(f.a.x, fmax_(f.b.x, f.c.x)), fmax_(f.a.y, fmax_(f.b.y, f.c.y)));
    f.flipped = r.flipped != 0u;
    return f;
}
GFX_TFDM_FN bool edge_outside(V2 n, V2 p, float s, float h) {    // the square's corner furthest along n, against the edge through p
    const V2 en = v2(s * n.x, s * n.y);
    const V2 e = v2(p.x + (en.x >= 0.0f ? h : -h), p.y + (en.y >= 0.0f ? h : -h));
    return en.x * e.x + en.y * e.y <= 0.0f;
}
GFX_TFDM_FN bool corner_beyond(V2 o, V2 e1, V2 corner, float s) { return s * cross2(e1, corner - o) < 0.0f; }
// testTriangleSquareIntersection2D (:817-865): interiors disjoint / square inside the triangle / anything else
GFX_TFDM_FN int classify(const Footprint& f, V2 centre, float h) {
    const V2 pa = f.a - centre, pb = f.b - centre, pc = f.c - centre;
    const V2 hiR = f.hi - centre, loR = f.lo - centre;
    if (fmin_(h, hiR.x) <= fmax_(-h, loR.x) || fmin_(h, hiR.y) <= fmax_(-h, loR.y)) return kOutside;
    const float s = f.flipped ? -1.0f : 1.0f;
    if (edge_outside(v2(f.b.y - f.a.y, f.a.x - f.b.x), pa, s, h)) return kOutside;
    if (edge_outside(v2(f.c.y - f.b.y, f.b.x - f.c.x), pb, s, h)) return kOutside;
    if (edge_outside(v2(f.a.y - f.c.y, f.c.x - f.a.x), pc, s, h)) return kOutside;
    for (int i = 0; i < 4; ++i) {
        const V2 corner = v2((i % 2) ? -h : h, (i / 2) ? -h : h);
        if (corner_beyond(pa, pb - pa, corner, s) || corner_beyond(pb, pc - pb, corner, s) || corner_beyond(pc, pa - pc, corner, s)) return kOverlapping;
    }
    return kInside;
}
GFX_TFDM_FN Texel root_texel(const TriRecord& r, uint32_t index) {
    const int w = r.rootMaxX - r.rootMinX + 1;
    Texel t;
    t.x = r.rootMinX + static_cast<int>(index) % w;
    t.y = r.rootMinY + static_cast<int>(index) / w;
    t.lod = r.rootLod;
    return t;
}
GFX_TFDM_FN float texel_scale(int maxDepth, int lod) { return pow2i(lod - maxDepth); }
GFX_TFDM_FN F2 pyramid_entry(const F2* pyramid, int maxDepth, Texel t) {    // kernels.h:177-181: repeat wrap; above the top level, the top entry
    if (t.lod >= maxDepth) return pyramid[level_offset(maxDepth, maxDepth)];
    const int w = 1 << (maxDepth - t.lod);
    return pyramid[level_offset(maxDepth, t.lod) + static_cast<uint32_t>(floor_mod(t.y, w) * w + floor_mod(t.x, w))];
}

// ---------------------------------------------------------------- boxes
struct Box { V3 lo, hi; };
// AABB_T::intersect (common/basic_types.h:3434-3448): entry and exit distance clipped to [distMin, distMax]
GFX_TFDM_FN bool box_hit(const Box& b, V3 org, V3 inv, float distMin, float distMax, float& t0, float& t1, V3& nearT, V3& farT) {
    const V3 tn = v3((b.lo.x - org.x) * inv.x, (b.lo.y - org.y) * inv.y, (b.lo.z - org.z) * inv.z);
    const V3 tf = v3((b.hi.x - org.x) * inv.x, (b.hi.y - org.y) * inv.y, (b.hi.z - org.z) * inv.z);
    nearT = v3(fmin_(tn.x, tf.x), fmin_(tn.y, tf.y), fmin_(tn.z, tf.z));
    farT = v3(fmax_(tn.x, tf.x), fmax_(tn.y, tf.y), fmax_(tn.z, tf.z));
    t0 = fmax_(fmax_(nearT.x, nearT.y), nearT.z);
    t1 = fmin_(fmin_(farT.x, farT.y), farT.z);
    const float c0 = fmax_(t0, distMin), c1 = fmin_(t1, distMax);
    return c0 <= c1 && c1 > 0.0f;
}
GFX_TFDM_FN Box box_of(AA3 a) {
    const Interval x = to_interval(a.x), y = to_interval(a.y), z = to_interval(a.z);
    Box b;
    b.lo = v3(x.lo, y.lo, z.lo);
    b.hi = v3(x.hi, y.hi, z.hi);
    return b;
}
// The tangent-space box of the displaced surface over a texel clipped to the footprint's bounds (kernels.h:173-208)
GFX_TFDM_FN Box texel_box(const TriRecord& r, const Footprint& f, const Params& p, F2 minmax, V2 centre, float scale) {
    const float amplitude = p.heightScale * (minmax.hi - minmax.lo);
    const float minHeight = p.baseHeight + p.heightScale * minmax.lo;
    const AA hBound = aa(minHeight + 0.5f * amplitude, 0.0f, 0.0f, 0.5f * amplitude);
    const V2 lo = v2(fmax_(centre.x - 0.5f * scale, f.lo.x), fmax_(centre.y - 0.5f * scale, f.lo.y));
    const V2 hi = v2(fmin_(centre.x + 0.5f * scale, f.hi.x), fmin_(centre.y + 0.5f * scale, f.hi.y));
    const V2 dim = hi - lo;
    const AA3 tc = aa3(aa(lo.x + 0.5f * dim.x, 0.5f * dim.x, 0.0f, 0.0f), aa(lo.y + 0.5f * dim.y, 0.0f, 0.5f * dim.y, 0.0f), aa(1.0f));
    const AA3 nObj = normalize(mul3(r.tcToN, 3, tc));
    const AA3 nTang = mul3(r.objToTang, 4, nObj);
    return box_of(aa3(tc.x, tc.y, aa(0.0f)) + hBound * nTang);
}

// ---------------------------------------------------------------- the intersection routine (displacedSurface_generic, kernels.h:39-562)
struct Hit { float t, bcB, bcC; V3 normal; uint32_t frontFace; };
struct Stats { uint32_t aabbTests, leafTests; };

// Ray against one micro-triangle in tangent space (kernels.h:310-328; the arithmetic of bvh8.hip.h ray_triangle)
GFX_TFDM_FN bool ray_triangle(V3 org, V3 dir, float distMin, float distMax, V3 pA, V3 pB, V3 pC, V3& n, float& t, float& bcB, float& bcC) {
    const V3 eAB = pB - pA, eCA = pA - pC;
    n = cross(eCA, eAB);
    const V3 e2 = (1.0f / dot(n, dir)) * (pA - org);
    const V3 i = cross(dir, e2);
    bcB = dot(i, eCA);
    bcC = dot(i, eAB);
    t = dot(n, e2);
    return (t < distMax) && (t > distMin) && (bcB >= 0.0f) && (bcC >= 0.0f) && (bcB + bcC <= 1.0f);
}

// makeCoordinateSystem (common/basic_types.h:2602-2609) of the normalised direction: d1, d2 span the plane across the ray
struct RayFrame { V3 d1, d2; float dirSq; };
GFX_TFDM_FN RayFrame ray_frame(V3 dir) {
    RayFrame f;
    f.dirSq = dot(dir, dir);
    const V3 d = normalize(dir);
    const float sign = d.z >= 0.0f ? 1.0f : -1.0f;
    const float a = -1.0f / (sign + d.z);
    const float b = d.x * d.y * a;
    f.d1 = v3(1.0f + sign * d.x * d.x * a, sign * b, -sign * d.x);
    f.d2 = v3(b, sign + d.y * d.y * a, -d.y);
    return f;
}

// The Bilinear local intersection (kernels.h:402-511): Newton's iteration in texture space for the point of
//     S(u, v) = P(u, v) + h(u, v) N(u, v) / |N(u, v)|,   h bilinear over the texel's four corner heights,
// on the ray's line, F(u, v) = ((S - entry) . d1, (S - entry) . d2) = 0, from the texel's centre.  `entry` is the ray point
// org + tEntry dir at the texel box's entry (the header's list of departures).  `res` is the number of texels per unit at the
// texel's level, (cx, cy) its index, lo / hi its corners.  Everything is in named scalars: nothing here is indexed at run time.
GFX_TFDM_FN bool newton_bilinear(const TriRecord& r, V2 tcA, V2 tcB, V2 tcC, V2 lo, V2 hi, float res, float cx, float cy, float hTL, float hTR, float hBL, float hBR,
                                 V3 entry, float tEntry, V3 dir, const RayFrame& fr, float tmin, float tmax, float& tOut, float& bcBOut, float& bcCOut, V3& nOut) {
    const V3 pu = v3(r.tcToP[0], r.tcToP[3], r.tcToP[6]), pv = v3(r.tcToP[1], r.tcToP[4], r.tcToP[7]);     // the Jacobians of P and N
    const V3 nu = v3(r.tcToN[0], r.tcToN[3], r.tcToN[6]), nv = v3(r.tcToN[1], r.tcToN[4], r.tcToN[7]);
    V2 g = v2(0.5f * lo.x + 0.5f * hi.x, 0.5f * lo.y + 0.5f * hi.y);
    const float behindAt = -(tEntry * fr.dirSq);          // along < behindAt: the guess projects behind the ray's origin
    float prevErr = inf();
    int errStreak = 0, behindStreak = 0, outsideStreak = 0;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int itr = 0; itr < 10; ++itr) {
        const V3 gp = v3(g.x, g.y, 1.0f);
        V3 n = mul3(r.tcToN, 3, gp);
        const float recLen = 1.0f / sqrtf(dot(n, n));
        n = recLen * n;
        const float ut = res * g.x - cx, vt = res * g.y - cy;
        const float h = (((1.0f - ut) * (1.0f - vt)) * hTL + (ut * (1.0f - vt)) * hTR) + (((1.0f - ut) * vt) * hBL + (ut * vt) * hBR);
        const V3 S = mul3(r.tcToP, 3, gp) + h * n;
        const V3 delta = S - entry;
        const float fx = dot(delta, fr.d1), fy = dot(delta, fr.d2);
        const float err = fx * fx + fy * fy;
        const float along = dot(dir, delta);
        errStreak = err > prevErr ? errStreak + 1 : 0;
        behindStreak = along < behindAt ? behindStreak + 1 : 0;
        if (errStreak >= 2 || behindStreak >= 2) return false;
        prevErr = err;
        const float hu = res * (((1.0f - vt) * hTR - (1.0f - vt) * hTL) + (vt * hBR - vt * hBL));
        const float hv = res * (((1.0f - ut) * hBL - (1.0f - ut) * hTL) + (ut * hBR - ut * hTR));
        // dS = dP + dh n + h d(N / |N|), d(N / |N|) = (dN - (dN . n) n) / |N|
        const float k = h * recLen;
        const V3 su = (pu + hu * n) + k * (nu - dot(nu, n) * n);
        const V3 sv = (pv + hv * n) + k * (nv - dot(nv, n) * n);
        if (err < 1e-5f * 1e-5f) {
            const float bcB = cross2(tcC - g, tcA - g) * r.recArea, bcC = cross2(tcA - g, tcB - g) * r.recArea;
            const float t = tEntry + along / fr.dirSq;
            V3 c = cross(su, sv);
            if (r.flipped != 0u) c = v3(-c.x, -c.y, -c.z);
            const float len2 = dot(c, c);
            if (!(bcB >= 0.0f && bcC >= 0.0f && bcB + bcC <= 1.0f) || !(along >= behindAt) || !(t > tmin && t < tmax) || !(len2 > 0.0f && len2 < inf())) return false;
            tOut = t; bcBOut = bcB; bcCOut = bcC;
            nOut = (1.0f / sqrtf(len2)) * c;
            return true;
        }
        if (itr + 1 < 10) {
            // dF / d(u, v) = ((d1 . su, d1 . sv), (d2 . su, d2 . sv)); a singular system gives a guess that is not a number,
            // which no comparison below accepts
            const float a = dot(fr.d1, su), b = dot(fr.d1, sv), c = dot(fr.d2, su), d = dot(fr.d2, sv);
            const float recDet = 1.0f / (a * d - b * c);
            g = v2(g.x - recDet * (d * fx - b * fy), g.y - recDet * (a * fy - c * fx));
            const float bcB = cross2(tcC - g, tcA - g) * r.recArea, bcC = cross2(tcA - g, tcB - g) * r.recArea, bcA = 1.0f - (bcB + bcC);
            const bool outside = g.x < lo.x || g.y < lo.y || g.x > hi.x || g.y > hi.y || bcA < 0.0f || bcB < 0.0f || bcC < 0.0f || bcA > 1.0f || bcB > 1.0f || bcC > 1.0f;
            outsideStreak = outside ? outsideStreak + 1 : 0;
            if (outsideStreak >= 3) return false;
            if (outside) g = v2(fmin_(fmax_(g.x, lo.x), hi.x), fmin_(fmax_(g.y, lo.y), hi.y));
        }
    }
    return false;
}

// The displaced surface of one base triangle against the ray (org, dir) of the base mesh's object space, inside (tmin, tmax).
// Returns whether a hit closer than tmax was found; `hit` is written only then.  kWithBilinear: the instantiation can run
// p.local == kBilinear; without it that branch is not compiled (an object of that mode never reaches such an instantiation).
template <bool kWithBilinear>
GFX_TFDM_FN bool intersect(const TriRecord& r, const Map& map, const Params& p, V3 org, V3 dir, float tmin, float tmax, Hit& hit, Stats& stats) {
    const Footprint f = footprint(r);
    const V3 orgT = mul3(r.objToTang, 4, org) + v3(r.objToTang[3], r.objToTang[7], r.objToTang[11]);
    const V3 dirT = mul3(r.objToTang, 4, dir);
    const V3 inv = v3(1.0f / dirT.x, 1.0f / dirT.y, 1.0f / dirT.z);
    const bool signX = dirT.x < 0.0f, signY = dirT.y < 0.0f;
    const int maxDepth = p.maxDepth;
    bool found = false;
    V3 hitNormal = v3(0.0f, 0.0f, 1.0f);
    const bool bilinear = kWithBilinear && p.local == kBilinear;
    const RayFrame fr = bilinear ? ray_frame(dir) : RayFrame();
    for (uint32_t rootIdx = 0; rootIdx < r.numRoots; ++rootIdx) {
        Texel cur = root_texel(r, rootIdx);
        Texel end = cur;
        const int initialLod = cur.lod;
        next(end, signX, signY, initialLod);
        while (!same(cur, end)) {
            const float scale = texel_scale(maxDepth, cur.lod);
            const V2 centre = v2((static_cast<float>(cur.x) + 0.5f) * scale, (static_cast<float>(cur.y) + 0.5f) * scale);
            // a texel outside the base triangle is skipped with its whole subtree
            if (classify(f, centre, 0.5f * scale) == kOutside) { next(cur, signX, signY, initialLod); continue; }
            ++stats.aabbTests;
            const Box box = texel_box(r, f, p, pyramid_entry(map.pyramid, maxDepth, cur), centre, scale);
            float t0, t1;
            V3 nearT, farT;
            // a ray that misses the box misses the surface inside the texel
            if (!box_hit(box, orgT, inv, tmin, tmax, t0, t1, nearT, farT)) { next(cur, signX, signY, initialLod); continue; }
            if (cur.lod > p.targetMipLevel) { down(cur, signX, signY); continue; }
            ++stats.leafTests;
            const V2 tcA = f.a, tcB = f.b, tcC = f.c;
            if (p.local == kBox) {
                // AABB_T::intersect with (u, v) + restoreHitPoint (common/basic_types.h:3467-3527): the entry face, or the exit face from inside
                const bool front = t0 >= 0.0f;
                const float t = front ? fmax_(t0, tmin) : fmin_(t1, tmax);
                if (t < tmax) {
                    const V3 sel = front ? nearT : v3(-farT.x, -farT.y, -farT.z);
                    const int axis = (sel.x >= sel.y && sel.x >= sel.z) ? 0 : (sel.y >= sel.z ? 1 : 2);
                    const float da = axis == 0 ? dirT.x : (axis == 1 ? dirT.y : dirT.z);
                    const bool posSide = front ? !(da > 0.0f) : (da > 0.0f);
                    V3 hp = orgT + t * dirT;
                    hp.x = fmin_(fmax_(hp.x, box.lo.x), box.hi.x);
                    hp.y = fmin_(fmax_(hp.y, box.lo.y), box.hi.y);
                    if (axis == 0) hp.x = posSide ? box.hi.x : box.lo.x;
                    if (axis == 1) hp.y = posSide ? box.hi.y : box.lo.y;
                    const V2 h2 = v2(hp.x, hp.y);
                    tmax = t;
                    found = true;
                    hit.bcB = cross2(tcC - h2, tcA - h2) * r.recArea;
                    hit.bcC = cross2(tcA - h2, tcB - h2) * r.recArea;
                    const float s = posSide ? 1.0f : -1.0f;
                    hitNormal = v3(axis == 0 ? s : 0.0f, axis == 1 ? s : 0.0f, axis == 2 ? s : 0.0f);
                }
            }
            else {
                const float hTL = p.baseHeight + p.heightScale * corner_height(map.heights, maxDepth, cur.lod, cur.x, cur.y);
                const float hTR = p.baseHeight + p.heightScale * corner_height(map.heights, maxDepth, cur.lod, cur.x + 1, cur.y);
                const float hBL = p.baseHeight + p.heightScale * corner_height(map.heights, maxDepth, cur.lod, cur.x, cur.y + 1);
                const float hBR = p.baseHeight + p.heightScale * corner_height(map.heights, maxDepth, cur.lod, cur.x + 1, cur.y + 1);
                if (bilinear) {
                    const float tEntry = fmax_(t0, tmin);
                    V3 n;
                    float t, bcB, bcC;
                    if (newton_bilinear(r, tcA, tcB, tcC, v2(centre.x + scale * -0.5f, centre.y + scale * -0.5f), v2(centre.x + scale * 0.5f, centre.y + scale * 0.5f),
                                        pow2i(maxDepth - cur.lod), static_cast<float>(cur.x), static_cast<float>(cur.y), hTL, hTR, hBL, hBR, org + tEntry * dir, tEntry, dir,
                                        fr, tmin, tmax, t, bcB, bcC, n)) {
                        tmax = t; found = true; hit.bcB = bcB; hit.bcC = bcC; hitNormal = n;
                    }
                    next(cur, signX, signY, initialLod);
                    continue;
                }
                const V2 tcTL = v2(centre.x + scale * -0.5f, centre.y + scale * -0.5f), tcTR = v2(centre.x + scale * 0.5f, centre.y + scale * -0.5f);
                const V2 tcBL = v2(centre.x + scale * -0.5f, centre.y + scale * 0.5f), tcBR = v2(centre.x + scale * 0.5f, centre.y + scale * 0.5f);
                // normals are normalised in object space, then taken to tangent space with the corner's height
                const V3 pTL = v3(tcTL.x, tcTL.y, 0.0f) + hTL * mul3(r.objToTang, 4, normalize(mul3(r.tcToN, 3, v3(tcTL.x, tcTL.y, 1.0f))));
                const V3 pTR = v3(tcTR.x, tcTR.y, 0.0f) + hTR * mul3(r.objToTang, 4, normalize(mul3(r.tcToN, 3, v3(tcTR.x, tcTR.y, 1.0f))));
                const V3 pBL = v3(tcBL.x, tcBL.y, 0.0f) + hBL * mul3(r.objToTang, 4, normalize(mul3(r.tcToN, 3, v3(tcBL.x, tcBL.y, 1.0f))));
                const V3 pBR = v3(tcBR.x, tcBR.y, 0.0f) + hBR * mul3(r.objToTang, 4, normalize(mul3(r.tcToN, 3, v3(tcBR.x, tcBR.y, 1.0f))));
                V3 n;
                float t, mB, mC;
                // TL-TR-BR, then TL-BR-BL; a hit counts only inside the base triangle in texture space
                if (ray_triangle(orgT, dirT, tmin, tmax, pTL, pTR, pBR, n, t, mB, mC)) {
                    const V2 h2 = ((1.0f - (mB + mC)) * tcTL + mB * tcTR) + mC * tcBR;
                    const float bcB = cross2(tcC - h2, tcA - h2) * r.recArea, bcC = cross2(tcA - h2, tcB - h2) * r.recArea;
                    if (bcB >= 0.0f && bcC >= 0.0f && bcB + bcC <= 1.0f) { tmax = t; found = true; hit.bcB = bcB; hit.bcC = bcC; hitNormal = n; }
                }
                if (ray_triangle(orgT, dirT, tmin, tmax, pTL, pBR, pBL, n, t, mB, mC)) {
                    const V2 h2 = ((1.0f - (mB + mC)) * tcTL + mB * tcBR) + mC * tcBL;
                    const float bcB = cross2(tcC - h2, tcA - h2) * r.recArea, bcC = cross2(tcA - h2, tcB - h2) * r.recArea;
                    if (bcB >= 0.0f && bcC >= 0.0f && bcB + bcC <= 1.0f) { tmax = t; found = true; hit.bcB = bcB; hit.bcC = bcC; hitNormal = n; }
                }
            }
            next(cur, signX, signY, initialLod);
        }
    }
    if (!found) return false;
    // the tangent-space normal goes back with the transpose of the upper-left 3 x 3 (the inverse transpose of tangent -> object)
    const float* m = r.objToTang;
    hit.t = tmax;
    if (bilinear) {                          // the normal of the smooth surface is in object space already
        hit.normal = hitNormal;
        hit.frontFace = dot(dir, hitNormal) <= 0.0f ? 1u : 0u;
        return true;
    }
    hit.normal = normalize(v3(m[0] * hitNormal.x + m[4] * hitNormal.y + m[8] * hitNormal.z, m[1] * hitNormal.x + m[5] * hitNormal.y + m[9] * hitNormal.z,
                              m[2] * hitNormal.x + m[6] * hitNormal.y + m[10] * hitNormal.z));
    hit.frontFace = dot(dirT, hitNormal) <= 0.0f ? 1u : 0u;
    return true;
}

// ---------------------------------------------------------------- per-triangle object-space box (computeAABBs, preprocess_kernels.cu:159-363)
GFX_TFDM_FN Box prim_aabb(const TriRecord& r, const F2* pyramid, const Params& p) {
    const Footprint f = footprint(r);
    const int maxDepth = p.maxDepth;
    float minH = inf(), maxH = -inf();
    for (uint32_t rootIdx = 0; rootIdx < r.numRoots; ++rootIdx) {
        Texel cur = root_texel(r, rootIdx);
        // a footprint as large as the map: the top entry bounds everything
        if (cur.lod >= maxDepth) { const F2 m = pyramid[level_offset(maxDepth, maxDepth)]; minH = m.lo; maxH = m.hi; break; }
        Texel end = cur;
        const int initialLod = cur.lod;
        next(end, false, false, initialLod);
        while (!same(cur, end)) {
            const float scale = texel_scale(maxDepth, cur.lod);
            const int k = classify(f, v2((static_cast<float>(cur.x) + 0.5f) * scale, (static_cast<float>(cur.y) + 0.5f) * scale), 0.5f * scale);
            if (k == kOutside) next(cur, false, false, initialLod);
            else if (k == kInside || cur.lod <= p.targetMipLevel) {
                const F2 m = pyramid_entry(pyramid, maxDepth, cur);
                minH = fmin_(minH, m.lo);
                maxH = fmax_(maxH, m.hi);
                next(cur, false, false, initialLod);
            }
            else down(cur);
        }
    }
    Box out;
    out.lo = v3(inf(), inf(), inf());
    out.hi = v3(-inf(), -inf(), -inf());
    if (!(minH <= maxH)) return out;       // nothing of the map under the footprint (numRoots == 0): an empty box
    const float amplitude = p.heightScale * (maxH - minH);
    const float base = p.baseHeight + p.heightScale * minH;
    const AA hBound = aa(base + 0.5f * amplitude, 0.0f, 0.0f, 0.5f * amplitude);
    // a triangle is the union of three parallelograms, each spanned by half of two edges from one vertex
    for (int pg = 0; pg < 3; ++pg) {
        const V2 t0 = v2(r.tc[2 * pg], r.tc[2 * pg + 1]);
        const V2 t1 = v2(r.tc[2 * ((pg + 1) % 3)], r.tc[2 * ((pg + 1) % 3) + 1]);
        const V2 t2 = v2(r.tc[2 * ((pg + 2) % 3)], r.tc[2 * ((pg + 2) % 3) + 1]);
        const V2 centre = (0.5f * t0 + 0.25f * t1) + 0.25f * t2;
        const V2 e0 = 0.25f * (t1 - t0), e1 = 0.25f * (t2 - t0);
        const AA3 tc = aa3(aa(centre.x, e0.x, e1.x, 0.0f), aa(centre.y, e0.y, e1.y, 0.0f), aa(1.0f));
        const AA3 pObj = mul3(r.tcToP, 3, tc);
        const AA3 nObj = normalize(mul3(r.tcToN, 3, tc));
        const Box b = box_of(pObj + hBound * nObj);
        out.lo = v3(fmin_(out.lo.x, b.lo.x), fmin_(out.lo.y, b.lo.y), fmin_(out.lo.z, b.lo.z));
        out.hi = v3(fmax_(out.hi.x, b.hi.x), fmax_(out.hi.y, b.hi.y), fmax_(out.hi.z, b.hi.z));
    }
    return out;
}

// ---------------------------------------------------------------- the tree over the per-triangle boxes, and one ray through it
// 32-byte node of a binary tree (tfdm_build.h build_tree).  Inner node: count == 0, children at `first` and `first + 1`.
// Leaf: count == 1, `first` is the primitive index.
struct alignas(16) Node { float lo[3]; uint32_t first; float hi[3]; uint32_t count; };
static_assert(sizeof(Node) == 32, "Node is two 16-byte loads");

struct TraceHit { float t, bcB, bcC; uint32_t prim; V3 normal; uint32_t frontFace; };
struct TraceStats { uint32_t aabbTests, leafTests, primTests; };

GFX_TFDM_FN Box node_box(const Node& n) { Box b; b.lo = v3(n.lo[0], n.lo[1], n.lo[2]); b.hi = v3(n.hi[0], n.hi[1], n.hi[2]); return b; }

// One ray, closest hit (kAny: any hit).  `Stack` has push(uint32 node, float key), pop(uint32&, float&), empty(): the device
// keeps it in an LDS column per lane, the host in an array.  Equal distances go to the lower primitive index.
//
// Every node has a key: where the ray enters its box, less a slack that is one number per ray (2^-17 of the magnitudes of the
// root box's entry and exit: the roundings of the slab test and of intersect()'s distance are some 2^-20 of them).  A node is
// walked while its key is no larger than the current hit distance, and a triangle's hit counts only from its leaf's key on.
// intersect() works in the base triangle's tangent frame and can report a point well in front of the box prim_aabb puts around
// P + h N / |N| (small triangles with strongly differing vertex normals).  Such a hit used to win or to be lost by whether its leaf
// was reached before a nearer leaf's hit had put the leaf's box behind the current distance.  With the rule, a hit that counts lies
// at or behind its leaf's key, an inner box is the union of its children's (its key is no larger than theirs: the same slack, and
// rounding is monotone), and the current distance only shrinks: a node that is skipped holds no hit that could have won.  So the
// result depends neither on the order of the walk nor on the tree's shape.
template <bool kAny, bool kWithBilinear, class Stack>
GFX_TFDM_FN bool trace_ray_local(const Node* nodes, const TriRecord* records, const Map& map, const Params& p, V3 org, V3 dir, float tmin, float tmax,
                           Stack& stack, TraceHit& best, TraceStats& ts) {
    best.t = tmax; best.bcB = 0.0f; best.bcC = 0.0f; best.prim = kInvalid; best.normal = v3(0.0f, 0.0f, 0.0f); best.frontFace = 0u;
    const V3 inv = v3(1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z);
    float t0, t1;
    V3 nearT, farT;
    if (!box_hit(node_box(nodes[0]), org, inv, tmin, tmax, t0, t1, nearT, farT)) return false;
    float slack = (fabsf(t0) + fabsf(t1)) * pow2i(-17);
    if (!(slack >= 0.0f)) slack = inf();         // a NaN: nothing is skipped and every hit counts
    uint32_t cur = 0u;
    float curKey = t0 - slack;
    while (true) {
        const Node n = nodes[cur];
        bool popNext = true;
        if (n.count != 0u) {
            const uint32_t prim = n.first;
            // the bound lets an equal distance through for a lower primitive index only
            const float bound = (best.prim != kInvalid && prim < best.prim) ? next_up(best.t) : best.t;
            Hit h;
            Stats s;
            s.aabbTests = 0u; s.leafTests = 0u;
            ++ts.primTests;
            const bool got = intersect<kWithBilinear>(records[prim], map, p, org, dir, tmin, bound, h, s);
            ts.aabbTests += s.aabbTests; ts.leafTests += s.leafTests;
            if (got && h.t >= curKey) {
                best.t = h.t; best.bcB = h.bcB; best.bcC = h.bcC; best.prim = prim; best.normal = h.normal; best.frontFace = h.frontFace;
                if (kAny) return true;
            }
        }
        else {
            float a0, a1, b0, b1;
            // (the far clip is the ray's own: what the current distance skips is decided by the key)
            bool hitA = box_hit(node_box(nodes[n.first]), org, inv, tmin, tmax, a0, a1, nearT, farT);
            bool hitB = box_hit(node_box(nodes[n.first + 1u]), org, inv, tmin, tmax, b0, b1, nearT, farT);
            const float keyA = a0 - slack, keyB = b0 - slack;
            hitA = hitA && keyA <= best.t;
            hitB = hitB && keyB <= best.t;
            if (hitA && hitB) {
                const bool aFirst = a0 <= b0;
                stack.push(aFirst ? n.first + 1u : n.first, aFirst ? keyB : keyA);
                cur = aFirst ? n.first : n.first + 1u;
                curKey = aFirst ? keyA : keyB;
                popNext = false;
            }
            else if (hitA || hitB) { cur = hitA ? n.first : n.first + 1u; curKey = hitA ? keyA : keyB; popNext = false; }
        }
        if (popNext) {
            bool have = false;
            while (!stack.empty()) {
                stack.pop(cur, curKey);
                if (curKey <= best.t) { have = true; break; }     // entered behind the current hit: skipped
            }
            if (!have) break;
        }
    }
    return best.prim != kInvalid;
}
// ... with the instantiation chosen by the object's mode (the host; a kernel names its own)
template <bool kAny, class Stack>
GFX_TFDM_FN bool trace_ray(const Node* nodes, const TriRecord* records, const Map& map, const Params& p, V3 org, V3 dir, float tmin, float tmax,
                           Stack& stack, TraceHit& best, TraceStats& ts) {
    if (p.local == kBilinear) return trace_ray_local<kAny, true>(nodes, records, map, p, org, dir, tmin, tmax, stack, best, ts);
    return trace_ray_local<kAny, false>(nodes, records, map, p, org, dir, tmin, tmax, stack, best, ts);
}

} // namespace tfdm
} // namespace gfx
