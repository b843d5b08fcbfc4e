// nrtdsm_core.hip.h -- non-recursive traversal for displacement mapping (NRTDSM): the arithmetic shared by the device kernels
// (nrtdsm.hip) and the host (nrtdsm_build.h, tests/nrtdsm_host.cpp).  A base triangle and its vertex normals span a prism; the
// straight ray becomes a curve in the prism's canonical space (alpha, beta, h), which is walked through the min-max pyramid of the
// height map as a quadtree and intersected with the map's micro-triangles by a cubic in h.  The surface it intersects,
//     S(alpha, beta) = P(alpha, beta) + (baseHeight + heightScale h(tc(alpha, beta))) N(alpha, beta),
// interpolates P, tc and N linearly and does NOT renormalise N: on an edge that two base triangles share both evaluate the same
// expression of the same two vertices, so the surface is continuous there (tfdm_core.hip.h displaces along normalize(N) in a
// per-triangle tangent space, and is not).
//
// Shared with TFDM and not restated: V2 / V3 / F2, Params, level_offset, corner_height, pyramid_entry, the triangle / square test
// classify(), ray_triangle(), ray_frame(), box_hit(), Node, Hit, TraceHit (tfdm_core.hip.h).
//
// Restated from the reference in this project's own types:
//     nrtdsm/gpu_kernels/nrtdsm_preprocess_kernels.cu:143-357   computeAABBs_generic<false>                 -> prim_bounds()
//     nrtdsm/gpu_kernels/nrtdsm_intersection_kernels.h:47-115   testRayVsBilinearPatch                      -> patch_range()
//                                                     :186-240  testRayVsPrism (enter / leave)              -> prism_range()
//                                                     :340-384  solveQuadraticEquation                      -> solve_quadratic()
//                                                     :520-613  findSingleRootClosed<3, false>              -> single_root()
//                                                     :616-794  solveCubicEquationNumerical<false>          -> solve_cubic()
//                                                     :802-863  the canonical- and texture-space ray        -> ray_poly()
//                                                     :985-1073 testNonlinearRayVsAabb with shared solves   -> box_range()
//                                                     :1078-1218 testNonlinearRayVsMicroTriangle            -> micro_triangle()
//                                                     :1523-1628 MipMapStack_T<3>                           -> Stack3
//                                                     :1632-2220 detailedSurface_generic<., false>          -> intersect()
// Where this differs from the reference, on purpose:
//   * both roots of a side patch count for the prism's enter / leave distances (the reference keeps the nearer one only, so a ray
//     that enters and leaves through the same bilinear wall gets an empty range); and a line with exactly one crossing found (an
//     infinite line crosses a closed prism an even number of times: one was lost to rounding at a seam) keeps the ray's whole range;
//   * a hit counts only with tmin < t < tmax (the reference's upper bound is the prism's leave distance times 1.0001);
//   * the base-triangle test has the same -1e-5 slack as the micro-triangle test (the reference: none), so that a hit on a shared
//     edge is accepted by at least one of the two neighbours;
//   * the normal is normalised and multiplied by the sign of det(SB - SA, SC - SA, N), so it lies on the side of +h whatever the
//     winding of the vertices against their normals; mirrored texture coordinates need no negation (the gradient of the height
//     function in object space does not know about them; tests/nrtdsm_ref.py holds this against d S / d alpha x d S / d beta);
//   * every loop is bounded: the safeguarded Newton / bisection stage of single_root() stops after kSolverCap steps and returns
//     its current iterate (the reference: while (true)); the descent stops after kMaxDescent iterations per base triangle and
//     reports a miss; a record whose root level would not fit the 24-level stack has no roots;
//   * a ray that is not finite or has a zero direction misses without entering anything;
//   * texel indices are int32 (int16 in the reference); powers of two are built from their bits (std::pow there).
//
// Plain C++17 under the project's math contract (tfdm_core.hip.h): +, -, x, / and sqrt only, no contraction; min, max, copysign
// and the sign test are written on the bits.  No local array is indexed at run time: the plane solves, the children and the
// roots live in named scalars and are chosen by selects.
#pragma once
#include "../tfdm/tfdm_core.hip.h"

namespace gfx {
namespace nrtdsm {

using namespace tfdm;

constexpr uint32_t kMaxDescent = 1u << 22;    // descent iterations per base triangle and ray; beyond: a miss
constexpr int kNewtonSteps = 16;              // plain Newton steps of single_root (:537)
constexpr int kSolverCap = 64;                // safeguarded steps after them; at the cap the current iterate is the root
constexpr int kStackLevels = 24;              // Stack3: one byte per level in three 64-bit words
constexpr float kSolverEps = 1e-5f;           // stopping width in h (:1124)
constexpr float kEdgeSlack = -1e-5f;          // barycentric slack of the base- and micro-triangle tests (:1204)

// Everything of a base triangle the query needs.  Positions, normals and texture coordinates are the caller's floats (the
// texture coordinates after the texture transform); minHeight / amplitude (object units) come from k_nrtdsm_prim.
struct alignas(16) PrismRecord {
    float pos[9];            // A, B, C
    float nrm[9];            // vertex normals as given: not normalised here, not renormalised anywhere
    float tc[6];             // tcA, tcB, tcC after the texture transform
    float minHeight;         // hOffset + s (min over the footprint - hBias)          (preprocess_kernels.cu:339-341)
    float amplitude;         // s (max - min)
    int32_t rootMinX, rootMinY, rootMaxX, rootMaxY, rootLod;   // findRoots with target level 0 (nrtdsm_shared.h:945-975)
    uint32_t numRoots;       // 0: degenerate in texture space or out of range, never hit
    uint32_t flipped;        // the footprint's area is negative
    uint32_t pad[3];
};
static_assert(sizeof(PrismRecord) == 144, "PrismRecord is 9 x 16 bytes");

// ---------------------------------------------------------------- scalars
GFX_TFDM_FN float nan_() { return b2f(0x7FC00000u); }
GFX_TFDM_FN bool finite_(float x) { return fabsf(x) < inf(); }                       // false for NaN and the infinities
GFX_TFDM_FN float copysign_(float mag, float sgn) { return b2f((f2b(mag) & 0x7FFFFFFFu) | (f2b(sgn) & 0x80000000u)); }
GFX_TFDM_FN bool differ_(float a, float b) { return ((f2b(a) ^ f2b(b)) >> 31) != 0u; }   // testIfDifferentSigns (:516)
GFX_TFDM_FN float quad(float a, float b, float c, float x) { return (a * x + b) * x + c; }
GFX_TFDM_FN V3 neg(V3 a) { return v3(-a.x, -a.y, -a.z); }
GFX_TFDM_FN V3 lerp3(V3 a, V3 b, float t) { return (1.0f - t) * a + t * b; }
GFX_TFDM_FN V3 rec_pos(const float* p, int v) { return v3(p[3 * v], p[3 * v + 1], p[3 * v + 2]); }

GFX_TFDM_FN Footprint footprint(const PrismRecord& r) {
    Footprint f;
    f.a = v2(r.tc[0], r.tc[1]); f.b = v2(r.tc[2], r.tc[3]); f.c = v2(r.tc[4], r.tc[5]);
    f.lo = v2(fmin_(f.a.x, fmin_(f.b.x, f.c.x)), fmin_(f.a.y, fmin_(f.b.y, f.c.y)));
    f.hi = v2(fmax_(f.a.x, fmax_(f.b.x, f.c.x)), fmax_(f.a.y, fmax_(f.b.y, f.c.y)));
    f.flipped = r.flipped != 0u;
    return f;
}
GFX_TFDM_FN Texel root_texel(const PrismRecord& r, uint32_t index) {
    const int w = r.rootMaxX - r.rootMinX + 1;
    Texel t;
    t.x = r.rootMinX + static_cast<int>(index) % w;
    t.y = r.rootMinY + static_cast<int>(index) / w;
    t.lod = r.rootLod;
    return t;
}

// ---------------------------------------------------------------- per-triangle heights and box (preprocess_kernels.cu:143-357)
// min / max of the pyramid over the footprint, then the union of the six prism corners.  Writes minHeight / amplitude.
GFX_TFDM_FN Box prim_bounds(PrismRecord& r, const F2* pyramid, const Params& p) {
    const Footprint f = footprint(r);
    const int maxDepth = p.maxDepth;
    float minH = inf(), maxH = -inf();
    for (uint32_t rootIdx = 0; rootIdx < r.numRoots; ++rootIdx) {
        Texel cur = root_texel(r, rootIdx);
        if (cur.lod >= maxDepth) { const F2 m = pyramid[level_offset(maxDepth, maxDepth)]; minH = m.lo; maxH = m.hi; break; }
        Texel end = cur;
        const int initialLod = cur.lod;
        next(end, false, false, initialLod);
        while (!same(cur, end)) {
            const float scale = texel_scale(maxDepth, cur.lod);
            const int k = classify(f, v2((static_cast<float>(cur.x) + 0.5f) * scale, (static_cast<float>(cur.y) + 0.5f) * scale), 0.5f * scale);
            if (k == kOutside) next(cur, false, false, initialLod);
            else if (k == kInside || cur.lod <= 0) {
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
    r.amplitude = p.heightScale * (maxH - minH);
    r.minHeight = p.baseHeight + p.heightScale * minH;
    if (!finite_(r.minHeight) || !finite_(r.amplitude)) { r.minHeight = 0.0f; r.amplitude = 0.0f; r.numRoots = 0u; return out; }
    for (int v = 0; v < 3; ++v) {
        const V3 pv = rec_pos(r.pos, v), nv = rec_pos(r.nrm, v);
        const V3 a = pv + r.minHeight * nv, b = pv + (r.minHeight + r.amplitude) * nv;
        out.lo = v3(fmin_(out.lo.x, fmin_(a.x, b.x)), fmin_(out.lo.y, fmin_(a.y, b.y)), fmin_(out.lo.z, fmin_(a.z, b.z)));
        out.hi = v3(fmax_(out.hi.x, fmax_(a.x, b.x)), fmax_(out.hi.y, fmax_(a.y, b.y)), fmax_(out.hi.z, fmax_(a.z, b.z)));
    }
    return out;
}

// ---------------------------------------------------------------- polynomials (:326-794)
// a x^2 + b x + c = 0 inside [lo, hi]: the roots in ascending order, NaN where there is none; returns their number
GFX_TFDM_FN uint32_t solve_quadratic(float a, float b, float c, float lo, float hi, float& r0, float& r1) {
    r0 = nan_(); r1 = nan_();
    if (a == 0.0f) {
        if (b == 0.0f) return 0u;
        const float x = -c / b;
        if (x >= lo && x <= hi) { r0 = x; return 1u; }
        return 0u;
    }
    const float D = b * b - 4.0f * a * c;
    if (!(D >= 0.0f)) return 0u;
    if (D == 0.0f) {
        const float x = -b / (2.0f * a);
        if (x >= lo && x <= hi) { r0 = x; return 1u; }
        return 0u;
    }
    const float temp = -0.5f * (b + copysign_(sqrtf(D), b));
    float x0 = c / temp, x1 = temp / a;
    if (x0 > x1) { const float t = x0; x0 = x1; x1 = t; }
    uint32_t n = 0u;
    if (x0 >= lo && x0 <= hi) { r0 = x0; n = 1u; }
    if (x1 >= lo && x1 <= hi) { if (n == 0u) r0 = x1; else r1 = x1; ++n; }
    return n;
}

struct Cubic { float c0, c1, c2, c3; };      // c3 x^3 + c2 x^2 + c1 x + c0
GFX_TFDM_FN float eval(const Cubic& k, float x) { return ((k.c3 * x + k.c2) * x + k.c1) * x + k.c0; }
GFX_TFDM_FN float eval_deriv(const Cubic& k, float x) { return ((3.0f * k.c3) * x + 2.0f * k.c2) * x + k.c1; }

// The one root inside a bracket whose end values differ in sign (:520-613 with boundError = false): kNewtonSteps plain Newton
// steps clamped to the bracket, then at most kSolverCap steps of Newton safeguarded by bisection.
GFX_TFDM_FN float single_root(const Cubic& k, float lo, float hi, float yLo, float eps) {
    float xr = (lo + hi) / 2.0f;
    if (hi - lo <= 2.0f * eps) return xr;
    const float xr0 = xr;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int itr = 0; itr < kNewtonSteps; ++itr) {
        const float xn = xr - eval(k, xr) / eval_deriv(k, xr);
        const float xc = fmin_(fmax_(xn, lo), hi);          // a NaN step clamps to lo
        if (fabsf(xc - xr) <= eps) return xc;
        xr = xc;
    }
    if (!finite_(xr)) xr = xr0;
    float yr = eval(k, xr);
    float xLo = lo, xHi = hi;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int itr = 0; itr < kSolverCap; ++itr) {
        if (differ_(yLo, yr)) xHi = xr; else xLo = xr;
        const float xn = xr - yr / eval_deriv(k, xr);
        if (xn > xLo && xn < xHi) {
            const float step = fabsf(xr - xn);
            xr = xn;
            if (!(step > eps)) break;
            yr = eval(k, xr);
        }
        else {
            xr = (xLo + xHi) / 2.0f;
            if (xr == xLo || xr == xHi || xHi - xLo <= 2.0f * eps) break;
            yr = eval(k, xr);
        }
    }
    return xr;
}

// Roots of a cubic inside [xMin, xMax] (:616-794 with boundError = false): split at the derivative's roots, solve the first
// bracket that changes sign numerically, the rest by deflation.  Returns their number; r0..r2 in the order found.
GFX_TFDM_FN uint32_t solve_cubic(const Cubic& k, float xMin, float xMax, float eps, float& r0, float& r1, float& r2) {
    r0 = nan_(); r1 = nan_(); r2 = nan_();
    if (k.c3 == 0.0f) return solve_quadratic(k.c2, k.c1, k.c0, xMin, xMax, r0, r1);
    const float a = k.c3, b = k.c2, c = k.c1;
    const float Dq = (2.0f * b) * (2.0f * b) - 12.0f * a * c;
    const float yMin = eval(k, xMin), yMax = eval(k, xMax);
    // the bracket to solve, and from where the deflated quadratic is searched (NaN: not at all)
    bool have = false;
    float bLo = xMin, bHi = xMax, yLo = yMin, deflateFrom = nan_();
    if (Dq > 0.0f) {
        const float temp = -b - 0.5f * copysign_(sqrtf(Dq), b);
        float cp0 = c / temp, cp1 = temp / (3.0f * a);
        if (cp0 > cp1) { const float t = cp0; cp0 = cp1; cp1 = t; }
        if (xMax <= cp0 || (xMin >= cp0 && xMax <= cp1) || xMin >= cp1) have = differ_(yMin, yMax);
        else if (cp0 > xMin) {
            const float yCp0 = eval(k, cp0), yCp1 = eval(k, cp1);
            if (differ_(yMin, yCp0)) {
                have = true; bHi = cp0;
                if (differ_(yCp0, yMax) || (cp1 < xMax && differ_(yCp0, yCp1))) deflateFrom = cp0;
            }
            else if (cp1 < xMax) {
                if (differ_(yCp0, yCp1)) { have = true; bLo = cp0; bHi = cp1; yLo = yCp0; if (differ_(yCp1, yMax)) deflateFrom = cp1; }
                else if (differ_(yCp1, yMax)) { have = true; bLo = cp1; yLo = yCp1; }
            }
            else if (differ_(yCp0, yMax)) { have = true; bLo = cp0; yLo = yCp0; }
        }
        else {
            const float yCp1 = eval(k, cp1);
            if (differ_(yMin, yCp1)) { have = true; bHi = cp1; if (differ_(yCp1, yMax)) deflateFrom = cp1; }
            else if (differ_(yCp1, yMax)) { have = true; bLo = cp1; yLo = yCp1; }
        }
    }
    else have = differ_(yMin, yMax);
    if (!have) return 0u;
    r0 = single_root(k, bLo, bHi, yLo, eps);
    if (deflateFrom != deflateFrom) return 1u;
    const float d2 = k.c3, d1 = k.c2 + r0 * d2, d0 = k.c1 + r0 * d1;      // deflatePolynomial<3> (:507-514)
    return 1u + solve_quadratic(d2, d1, d0, deflateFrom, xMax, r1, r2);
}

// ---------------------------------------------------------------- ray against prism (:47-115, :186-240)
struct Range { float lo, hi; uint32_t count; };
GFX_TFDM_FN void add(Range& r, float t) { r.lo = fmin_(r.lo, t); r.hi = fmax_(r.hi, t); ++r.count; }

GFX_TFDM_FN void patch_root(float u, V3 dir, V3 ra, V3 rb, V3 eAC, V3 eBD, Range& r) {
    if (!(u >= 0.0f && u <= 1.0f)) return;
    const V3 pAB = lerp3(ra, rb, u), pCD = lerp3(eAC, eBD, u);
    V3 n = cross(dir, pCD);
    const float recDet = 1.0f / dot(n, n);
    n = cross(n, pAB);
    const float t = dot(n, pCD) * recDet, v = dot(n, dir) * recDet;
    if (v >= 0.0f && v <= 1.0f && finite_(t)) add(r, t);
}
// the bilinear patch A-B / C-D ("Cool Patches", Ray Tracing Gems ch. 8) against the whole line
GFX_TFDM_FN void patch_range(V3 org, V3 dir, V3 pA, V3 pB, V3 pC, V3 pD, Range& r) {
    const V3 eAB = pB - pA, eAC = pC - pA, eBD = pD - pB, eCD = pD - pC;
    const V3 ra = pA - org, rb = pB - org;
    const float a = dot(cross(eAB, neg(eCD)), dir);
    float b = dot(cross(rb, dir), eBD);
    const float c = dot(cross(ra, dir), eAC);
    b -= a + c;
    const float det = b * b - 4.0f * a * c;
    if (!(det >= 0.0f)) return;
    float u1, u2;
    if (a == 0.0f) { u1 = -c / b; u2 = -1.0f; }
    else {
        const float temp = -0.5f * (b + copysign_(sqrtf(det), b));
        u1 = temp / a;
        u2 = c / temp;
    }
    patch_root(u1, dir, ra, rb, eAC, eBD, r);
    patch_root(u2, dir, ra, rb, eAC, eBD, r);
}
GFX_TFDM_FN void triangle_range(V3 org, V3 dir, V3 pA, V3 pB, V3 pC, Range& r) {
    V3 n;
    float t, bcB, bcC;
    if (ray_triangle(org, dir, -inf(), inf(), pA, pB, pC, n, t, bcB, bcC)) add(r, t);
}
// enter / leave distance of the line through the prism A B C (bottom) D E F (top), clipped to [tmin, tmax]
GFX_TFDM_FN bool prism_range(V3 org, V3 dir, float tmin, float tmax, V3 pA, V3 pB, V3 pC, V3 pD, V3 pE, V3 pF, float& enter, float& leave) {
    Range r;
    r.lo = inf(); r.hi = -inf(); r.count = 0u;
    triangle_range(org, dir, pC, pB, pA, r);
    triangle_range(org, dir, pD, pE, pF, r);
    patch_range(org, dir, pA, pB, pD, pE, r);
    patch_range(org, dir, pB, pC, pE, pF, r);
    patch_range(org, dir, pC, pA, pF, pD, r);
    if (r.count == 1u) { r.lo = -inf(); r.hi = inf(); }
    enter = fmax_(r.lo, tmin);
    leave = fmin_(r.hi, tmax);
    return enter <= leave && leave > 0.0f;
}

// ---------------------------------------------------------------- the ray in canonical and texture space (:802-863)
struct Prism { V3 pA, pB, pC, nA, nB, nC; };        // positions at map value 0, normals times the height of map value 1
// alpha(h) = bcB(h) / dn(h), beta(h) = bcC(h) / dn(h), u(h) = tu(h) / dn(h), v(h) = tv(h) / dn(h): quadratics, [2] x^2 + [1] x + [0]
struct RayPoly { float bcB2, bcB1, bcB0, bcC2, bcC1, bcC0, dn2, dn1, dn0, tu2, tu1, tu0, tv2, tv1, tv0; };
GFX_TFDM_FN RayPoly ray_poly(const Prism& P, V3 org, V3 e0, V3 e1, V2 tcA, V2 tcB, V2 tcC) {
    const V3 eABo = P.pB - P.pA, eACo = P.pC - P.pA, fABo = P.nB - P.nA, fACo = P.nC - P.nA, eAOo = org - P.pA;
    const V2 eAB = v2(dot(eABo, e0), dot(eABo, e1)), eAC = v2(dot(eACo, e0), dot(eACo, e1));
    const V2 fAB = v2(dot(fABo, e0), dot(fABo, e1)), fAC = v2(dot(fACo, e0), dot(fACo, e1));
    const V2 eAO = v2(dot(eAOo, e0), dot(eAOo, e1)), NA = v2(dot(P.nA, e0), dot(P.nA, e1));
    RayPoly q;
    q.dn2 = fAB.x * fAC.y - fAB.y * fAC.x;
    q.dn1 = eAB.x * fAC.y + fAB.x * eAC.y - eAB.y * fAC.x - fAB.y * eAC.x;
    q.dn0 = eAB.x * eAC.y - eAB.y * eAC.x;
    q.bcB2 = -NA.x * fAC.y + NA.y * fAC.x;
    q.bcB1 = eAO.x * fAC.y - eAC.y * NA.x - eAO.y * fAC.x + NA.y * eAC.x;
    q.bcB0 = eAO.x * eAC.y - eAO.y * eAC.x;
    q.bcC2 = -(-NA.x * fAB.y + NA.y * fAB.x);
    q.bcC1 = -(eAO.x * fAB.y - eAB.y * NA.x - eAO.y * fAB.x + NA.y * eAB.x);
    q.bcC0 = -(eAO.x * eAB.y - eAO.y * eAB.x);
    const float a2 = q.dn2 - q.bcB2 - q.bcC2, a1 = q.dn1 - q.bcB1 - q.bcC1, a0 = q.dn0 - q.bcB0 - q.bcC0;
    q.tu2 = a2 * tcA.x + q.bcB2 * tcB.x + q.bcC2 * tcC.x; q.tv2 = a2 * tcA.y + q.bcB2 * tcB.y + q.bcC2 * tcC.y;
    q.tu1 = a1 * tcA.x + q.bcB1 * tcB.x + q.bcC1 * tcC.x; q.tv1 = a1 * tcA.y + q.bcB1 * tcB.y + q.bcC1 * tcC.y;
    q.tu0 = a0 * tcA.x + q.bcB0 * tcB.x + q.bcC0 * tcC.x; q.tv0 = a0 * tcA.y + q.bcB0 * tcB.y + q.bcC0 * tcC.y;
    return q;
}
// computeSignedDistance (:868-877): the ray parameter of the point (alpha, beta, h) of the prism
GFX_TFDM_FN float signed_distance(const Prism& P, V3 org, V3 dir, float recSq, float h, float alpha, float beta) {
    const V3 SA = P.pA + h * P.nA, SB = P.pB + h * P.nB, SC = P.pC + h * P.nC;
    return recSq * dot(dir, (((1.0f - alpha - beta) * SA + alpha * SB) + beta * SC) - org);
}
GFX_TFDM_FN void add_curve_point(const Prism& P, const RayPoly& q, V3 org, V3 dir, float recSq, float h, float recDn, Range& r) {
    const float alpha = quad(q.bcB2, q.bcB1, q.bcB0, h) * recDn, beta = quad(q.bcC2, q.bcC1, q.bcC0, h) * recDn;
    add(r, signed_distance(P, org, dir, recSq, h, alpha, beta));
}

// ---------------------------------------------------------------- the curved ray against a box in (u, v, h) (:882-1073, :1896-1940)
// Where the curve crosses a plane u = const (or v = const): up to two h in [0, 1], and the other texture coordinate there.
struct PlaneSolve { float h0, h1, w0, w1; };
GFX_TFDM_FN PlaneSolve solve_plane(float a2, float a1, float a0, float b2, float b1, float b0, const RayPoly& q, float plane) {
    PlaneSolve s;
    solve_quadratic(a2 - plane * q.dn2, a1 - plane * q.dn1, a0 - plane * q.dn0, 0.0f, 1.0f, s.h0, s.h1);
    s.w0 = finite_(s.h0) ? quad(b2, b1, b0, s.h0) / quad(q.dn2, q.dn1, q.dn0, s.h0) : nan_();
    s.w1 = finite_(s.h1) ? quad(b2, b1, b0, s.h1) / quad(q.dn2, q.dn1, q.dn0, s.h1) : nan_();
    return s;
}
GFX_TFDM_FN void side_plane(const Prism& P, const RayPoly& q, V3 org, V3 dir, float recSq, float h, float w, float wLo, float wHi, float hLo, float hHi, Range& r) {
    if (w >= wLo && w <= wHi && h >= hLo && h <= hHi) add_curve_point(P, q, org, dir, recSq, h, 1.0f / quad(q.dn2, q.dn1, q.dn0, h), r);
}
GFX_TFDM_FN void height_plane(const Prism& P, const RayPoly& q, V3 org, V3 dir, float recSq, float h, float uLo, float uHi, float vLo, float vHi, Range& r) {
    const float dn = quad(q.dn2, q.dn1, q.dn0, h);
    if (dn != 0.0f) {
        const float recDn = 1.0f / dn;
        const float u = quad(q.tu2, q.tu1, q.tu0, h) * recDn, v = quad(q.tv2, q.tv1, q.tv0, h) * recDn;
        if (u >= uLo && u <= uHi && v >= vLo && v <= vHi) add_curve_point(P, q, org, dir, recSq, h, recDn, r);
    }
}
// the signed-distance interval of the curve inside the box, clipped to [distMin, distMax]
GFX_TFDM_FN bool box_range(const Prism& P, const RayPoly& q, V3 org, V3 dir, float recSq, float uLo, float uHi, float vLo, float vHi, float hLo, float hHi,
                           const PlaneSolve& sULo, const PlaneSolve& sUHi, const PlaneSolve& sVLo, const PlaneSolve& sVHi, float distMin, float distMax,
                           float& d0, float& d1) {
    Range r;
    r.lo = inf(); r.hi = -inf(); r.count = 0u;
    height_plane(P, q, org, dir, recSq, hLo, uLo, uHi, vLo, vHi, r);
    height_plane(P, q, org, dir, recSq, hHi, uLo, uHi, vLo, vHi, r);
    side_plane(P, q, org, dir, recSq, sULo.h0, sULo.w0, vLo, vHi, hLo, hHi, r);
    side_plane(P, q, org, dir, recSq, sULo.h1, sULo.w1, vLo, vHi, hLo, hHi, r);
    side_plane(P, q, org, dir, recSq, sUHi.h0, sUHi.w0, vLo, vHi, hLo, hHi, r);
    side_plane(P, q, org, dir, recSq, sUHi.h1, sUHi.w1, vLo, vHi, hLo, hHi, r);
    side_plane(P, q, org, dir, recSq, sVLo.h0, sVLo.w0, uLo, uHi, hLo, hHi, r);
    side_plane(P, q, org, dir, recSq, sVLo.h1, sVLo.w1, uLo, uHi, hLo, hHi, r);
    side_plane(P, q, org, dir, recSq, sVHi.h0, sVHi.w0, uLo, uHi, hLo, hHi, r);
    side_plane(P, q, org, dir, recSq, sVHi.h1, sVHi.w1, uLo, uHi, hLo, hHi, r);
    d0 = fmax_(r.lo, distMin);
    d1 = fmin_(r.hi, distMax);
    return d0 <= d1 && d1 > 0.0f;
}

// ---------------------------------------------------------------- the curved ray against a micro-triangle (:1078-1218)
// mA, mB, mC: (u, v, map value) of the micro-triangle.  Writes the hit only where it is nearer than `hitDist`.
GFX_TFDM_FN bool micro_triangle(const Prism& P, V2 tcA, V2 tcB, V2 tcC, V3 mA, V3 mB, V3 mC, V3 org, V3 dir, float recSq, float distMin, V3 e0, V3 e1,
                                const RayPoly& q, float& hitDist, float& hitAlpha, float& hitBeta, V3& hitNormal) {
    const V3 nTex = normalize(cross(mB - mA, mC - mA));
    const float KTex = -dot(nTex, mA);
    const V3 nCan = v3(nTex.x * (tcB.x - tcA.x) + nTex.y * (tcB.y - tcA.y), nTex.x * (tcC.x - tcA.x) + nTex.y * (tcC.y - tcA.y), nTex.z);
    const float KCan = nTex.x * tcA.x + nTex.y * tcA.y + KTex;
    const float minH = fmin_(fmin_(mA.z, mB.z), mC.z) - 1e-4f, maxH = fmax_(fmax_(mA.z, mB.z), mC.z) + 1e-4f;
    Cubic k;
    k.c0 = nTex.x * q.tu0 + nTex.y * q.tv0 + KTex * q.dn0;
    k.c1 = nTex.x * q.tu1 + nTex.y * q.tv1 + nTex.z * q.dn0 + KTex * q.dn1;
    k.c2 = nTex.x * q.tu2 + nTex.y * q.tv2 + nTex.z * q.dn1 + KTex * q.dn2;
    k.c3 = nTex.z * q.dn2;
    float r0, r1, r2;
    const uint32_t numRoots = solve_cubic(k, minH, maxH, kSolverEps, r0, r1, r2);
    // the micro-triangle's own barycentrics of a point of its plane (:1191-1206)
    const V3 mAB = mB - mA, mAC = mC - mA;
    const float dABAB = dot(mAB, mAB), dABAC = dot(mAB, mAC), dACAC = dot(mAC, mAC);
    const float recM = 1.0f / (dABAB * dACAC - dABAC * dABAC);
    bool found = false;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (uint32_t i = 0; i < 3u; ++i) {
        if (i >= numRoots) break;
        const float h = i == 0u ? r0 : (i == 1u ? r1 : r2);
        const V3 SA = P.pA + h * P.nA, SB = P.pB + h * P.nB, SC = P.pC + h * P.nC;
        const V3 eSABo = SB - SA, eSACo = SC - SA, eSAOo = org - SA;
        const V2 eSAB = v2(dot(eSABo, e0), dot(eSABo, e1)), eSAC = v2(dot(eSACo, e0), dot(eSACo, e1)), eSAO = v2(dot(eSAOo, e0), dot(eSAOo, e1));
        // a11 alpha + a12 beta = b1, a21 alpha + a22 beta = b2: the best conditioned pair of the ray's two equations and the plane's
        float a11 = eSAB.x, a12 = eSAC.x, a21 = eSAB.y, a22 = eSAC.y, b1 = eSAO.x, b2 = eSAO.y;
        float det = eSAB.x * eSAC.y - eSAC.x * eSAB.y;
        const float planeRhs = -nCan.z * h - KCan;
        const float det1 = eSAB.x * nCan.y - eSAC.x * nCan.x;
        if (fabsf(det1) > fabsf(det)) { a21 = nCan.x; a22 = nCan.y; b2 = planeRhs; det = det1; }
        const float det2 = eSAB.y * nCan.y - eSAC.y * nCan.x;
        if (fabsf(det2) > fabsf(det)) { a11 = eSAB.y; a12 = eSAC.y; b1 = eSAO.y; a21 = nCan.x; a22 = nCan.y; b2 = planeRhs; det = det2; }
        const float recDet = 1.0f / det;
        const float alpha = recDet * (a22 * b1 - a12 * b2), beta = recDet * (-a21 * b1 + a11 * b2);
        if (!(alpha >= kEdgeSlack && beta >= kEdgeSlack && alpha + beta <= 1.0f - kEdgeSlack)) continue;
        const V2 hp = ((1.0f - alpha - beta) * tcA + alpha * tcB) + beta * tcC;
        const V3 mAP = v3(hp.x, hp.y, h) - mA;
        const float dAPAB = dot(mAP, mAB), dAPAC = dot(mAP, mAC);
        const float mB_ = recM * (dACAC * dAPAB - dABAC * dAPAC), mC_ = recM * (dABAB * dAPAC - dABAC * dAPAB);
        const float mA_ = 1.0f - (mB_ + mC_);
        if (!(mA_ > kEdgeSlack && mB_ > kEdgeSlack && mC_ > kEdgeSlack)) continue;
        const float dist = signed_distance(P, org, dir, recSq, h, alpha, beta);
        if (!(dist > distMin && dist < hitDist)) continue;
        // the gradient of the plane's function in object space: cofactors of (SB - SA, SC - SA, N) applied to -nCan, times the
        // sign of their determinant
        const V3 N = ((1.0f - alpha - beta) * P.nA + alpha * P.nB) + beta * P.nC;
        const V3 c12 = cross(eSACo, N), c20 = cross(N, eSABo), c01 = cross(eSABo, eSACo);
        V3 n = (-nCan.x * c12 + -nCan.y * c20) + -nCan.z * c01;
        if (dot(eSABo, c12) < 0.0f) n = neg(n);
        const float len2 = dot(n, n);
        if (!(len2 > 0.0f && len2 < inf())) continue;
        hitDist = dist; hitAlpha = alpha; hitBeta = beta;
        hitNormal = (1.0f / sqrtf(len2)) * n;
        found = true;
    }
    return found;
}

// ---------------------------------------------------------------- the compact stack (:1523-1628)
// One byte per level: a 2-bit count and up to three 2-bit entries (bit 0: x offset, bit 1: y offset), nearest first.
struct Stack3 { uint64_t w0, w1, w2; };
GFX_TFDM_FN uint32_t stack_get(const Stack3& s, int level) {
    const uint64_t w = level < 8 ? s.w0 : (level < 16 ? s.w1 : s.w2);
    return static_cast<uint32_t>(w >> ((level & 7) * 8)) & 0xFFu;
}
GFX_TFDM_FN void stack_put(Stack3& s, int level, uint32_t byte) {
    const int shift = (level & 7) * 8;
    const uint64_t keep = ~(static_cast<uint64_t>(0xFFu) << shift), val = static_cast<uint64_t>(byte & 0xFFu) << shift;
    if (level < 8) s.w0 = (s.w0 & keep) | val;
    else if (level < 16) s.w1 = (s.w1 & keep) | val;
    else s.w2 = (s.w2 & keep) | val;
}
GFX_TFDM_FN void sort2(float& dA, uint32_t& eA, float& dB, uint32_t& eB) {
    if (dA > dB) { const float d = dA; dA = dB; dB = d; const uint32_t e = eA; eA = eB; eB = e; }
}

// ---------------------------------------------------------------- the intersection routine (detailedSurface_generic, :1632-2220)
constexpr uint32_t kNoEntry = 0xFFu;

// The displaced surface of one base triangle against the ray (org, dir) inside (tmin, tmax); e0, e1: the ray's frame; recSq =
// 1 / |dir|^2.  `hit` is written only when a hit closer than tmax was found.  `iterations` counts the descent's iterations.
GFX_TFDM_FN bool intersect(const PrismRecord& r, const Map& map, const Params& p, V3 org, V3 dir, V3 e0, V3 e1, float recSq, float tmin, float tmax,
                           Hit& hit, Stats& stats, uint32_t& iterations) {
    iterations = 0u;
    if (r.numRoots == 0u || r.rootLod >= kStackLevels) return false;
    const V3 posA = rec_pos(r.pos, 0), posB = rec_pos(r.pos, 1), posC = rec_pos(r.pos, 2);
    const V3 nrmA = rec_pos(r.nrm, 0), nrmB = rec_pos(r.nrm, 1), nrmC = rec_pos(r.nrm, 2);
    float enter, leave;
    {
        const float hLo = r.minHeight, hHi = r.minHeight + r.amplitude;
        if (!prism_range(org, dir, tmin, tmax, posA + hLo * nrmA, posB + hLo * nrmB, posC + hLo * nrmC, posA + hHi * nrmA, posB + hHi * nrmB, posC + hHi * nrmC, enter, leave))
            return false;
    }
    Prism P;
    P.pA = posA + p.baseHeight * nrmA; P.pB = posB + p.baseHeight * nrmB; P.pC = posC + p.baseHeight * nrmC;
    P.nA = p.heightScale * nrmA; P.nB = p.heightScale * nrmB; P.nC = p.heightScale * nrmC;
    const Footprint f = footprint(r);
    const float distMin = fmax_(enter * 0.9999f, tmin);
    float hitDist = fmin_(leave * 1.0001f, tmax);
    const RayPoly q = ray_poly(P, org, e0, e1, f.a, f.b, f.c);
    const int maxDepth = p.maxDepth;
    bool found = false;
    float hitAlpha = 0.0f, hitBeta = 0.0f;
    V3 hitNormal = v3(0.0f, 0.0f, 0.0f);
    Stack3 stack;
    stack.w0 = 0u; stack.w1 = 0u; stack.w2 = 0u;
    for (uint32_t rootIdx = 0; rootIdx < r.numRoots; ++rootIdx) {
        Texel cur = root_texel(r, rootIdx);
        const int initialLod = cur.lod;
        uint32_t entry = static_cast<uint32_t>(floor_mod(cur.x, 2)) | (static_cast<uint32_t>(floor_mod(cur.y, 2)) << 1);
        while (cur.lod <= initialLod) {
            if (++iterations > kMaxDescent) return false;
            if (entry == kNoEntry) {
                const uint32_t byte = stack_get(stack, cur.lod), count = byte & 3u;
                if (count == 0u) { up(cur); continue; }
                entry = (byte >> 2) & 3u;
                stack_put(stack, cur.lod, ((byte >> 2) & ~3u) | (count - 1u));
            }
            cur.x = floor_div(cur.x, 2) * 2 + static_cast<int>(entry & 1u);
            cur.y = floor_div(cur.y, 2) * 2 + static_cast<int>(entry >> 1);
            const float scale = texel_scale(maxDepth, cur.lod);
            const V2 centre = v2((static_cast<float>(cur.x) + 0.5f) * scale, (static_cast<float>(cur.y) + 0.5f) * scale);
            // a texel outside the base triangle is skipped with its whole subtree
            if (classify(f, centre, 0.5f * scale) == kOutside) { entry = kNoEntry; continue; }
            if (cur.lod > 0) {
                // the four children share planes: three u solves and three v solves serve all of them
                const float u0 = static_cast<float>(cur.x) * scale, u1 = centre.x, u2 = (static_cast<float>(cur.x) + 1.0f) * scale;
                const float v0 = static_cast<float>(cur.y) * scale, v1 = centre.y, v2_ = (static_cast<float>(cur.y) + 1.0f) * scale;
                const PlaneSolve sU0 = solve_plane(q.tu2, q.tu1, q.tu0, q.tv2, q.tv1, q.tv0, q, u0);
                const PlaneSolve sU1 = solve_plane(q.tu2, q.tu1, q.tu0, q.tv2, q.tv1, q.tv0, q, u1);
                const PlaneSolve sU2 = solve_plane(q.tu2, q.tu1, q.tu0, q.tv2, q.tv1, q.tv0, q, u2);
                const PlaneSolve sV0 = solve_plane(q.tv2, q.tv1, q.tv0, q.tu2, q.tu1, q.tu0, q, v0);
                const PlaneSolve sV1 = solve_plane(q.tv2, q.tv1, q.tv0, q.tu2, q.tu1, q.tu0, q, v1);
                const PlaneSolve sV2 = solve_plane(q.tv2, q.tv1, q.tv0, q.tu2, q.tu1, q.tu0, q, v2_);
                down(cur);
                float dist0 = inf(), dist1 = inf(), dist2 = inf(), dist3 = inf();
                uint32_t numValid = 0u;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
                for (uint32_t i = 0; i < 4u; ++i) {
                    ++stats.aabbTests;
                    const bool uHalf = (i & 1u) != 0u, vHalf = (i >> 1) != 0u;
                    Texel child;
                    child.x = cur.x + (uHalf ? 1 : 0); child.y = cur.y + (vHalf ? 1 : 0); child.lod = cur.lod;
                    const F2 mm = pyramid_entry(map.pyramid, maxDepth, child);
                    float d0, d1;
                    const bool in = box_range(P, q, org, dir, recSq, uHalf ? u1 : u0, uHalf ? u2 : u1, vHalf ? v1 : v0, vHalf ? v2_ : v1, mm.lo, mm.hi,
                                              uHalf ? sU1 : sU0, uHalf ? sU2 : sU1, vHalf ? sV1 : sV0, vHalf ? sV2 : sV1, distMin, hitDist, d0, d1);
                    const float dist = in ? 0.5f * (d0 + d1) : inf();
                    if (in) ++numValid;
                    if (i == 0u) dist0 = dist; else if (i == 1u) dist1 = dist; else if (i == 2u) dist2 = dist; else dist3 = dist;
                }
                uint32_t e0_ = 0u, e1_ = 1u, e2_ = 2u, e3_ = 3u;
                sort2(dist0, e0_, dist1, e1_);
                sort2(dist2, e2_, dist3, e3_);
                sort2(dist0, e0_, dist2, e2_);
                sort2(dist1, e1_, dist3, e3_);
                sort2(dist1, e1_, dist2, e2_);
                if (numValid == 0u) entry = kNoEntry;
                else {
                    entry = e0_;
                    const uint32_t rest = numValid - 1u;
                    if (rest > 0u) stack_put(stack, cur.lod, rest | (e1_ << 2) | (rest > 1u ? e2_ << 4 : 0u) | (rest > 2u ? e3_ << 6 : 0u));
                }
                continue;
            }
            ++stats.leafTests;
            const float hTL = corner_height(map.heights, maxDepth, 0, cur.x, cur.y), hTR = corner_height(map.heights, maxDepth, 0, cur.x + 1, cur.y);
            const float hBL = corner_height(map.heights, maxDepth, 0, cur.x, cur.y + 1), hBR = corner_height(map.heights, maxDepth, 0, cur.x + 1, cur.y + 1);
            const float uL = static_cast<float>(cur.x) * scale, vT = static_cast<float>(cur.y) * scale;
            const float uR = static_cast<float>(cur.x + 1) * scale, vB = static_cast<float>(cur.y + 1) * scale;
            const V3 mTL = v3(uL, vT, hTL), mBR = v3(uR, vB, hBR);
#if defined(__HIPCC__)
#pragma unroll 1
#endif
            for (int tri = 0; tri < 2; ++tri) {      // TL-BL-BR, then TL-BR-TR
                const V3 mB = tri == 0 ? v3(uL, vB, hBL) : mBR, mC = tri == 0 ? mBR : v3(uR, vT, hTR);
                if (micro_triangle(P, f.a, f.b, f.c, mTL, mB, mC, org, dir, recSq, distMin, e0, e1, q, hitDist, hitAlpha, hitBeta, hitNormal)) found = true;
            }
            entry = kNoEntry;
        }
    }
    if (!found) return false;
    hit.t = hitDist; hit.bcB = hitAlpha; hit.bcC = hitBeta;
    hit.normal = hitNormal;
    hit.frontFace = dot(dir, hitNormal) <= 0.0f ? 1u : 0u;
    return true;
}

// ---------------------------------------------------------------- one ray through the tree over the per-triangle boxes
struct TraceStats { uint32_t aabbTests, leafTests, primTests, maxIterations; };

GFX_TFDM_FN bool ray_ok(V3 org, V3 dir, float tmin, float tmax) {
    const float dd = dot(dir, dir);
    return finite_(org.x) && finite_(org.y) && finite_(org.z) && finite_(dir.x) && finite_(dir.y) && finite_(dir.z) && dd > 0.0f && finite_(dd) &&
           finite_(1.0f / dd) && tmin == tmin && tmax == tmax;
}

// As tfdm::trace_ray_local: closest hit (kAny: any hit); equal distances go to the lower primitive index.
template <bool kAny, class Stack>
GFX_TFDM_FN bool trace_ray(const Node* nodes, const PrismRecord* records, const Map& map, const Params& p, V3 org, V3 dir, float tmin, float tmax, Stack& stack,
                           TraceHit& best, TraceStats& ts) {
    best.t = tmax; best.bcB = 0.0f; best.bcC = 0.0f; best.prim = kInvalid; best.normal = v3(0.0f, 0.0f, 0.0f); best.frontFace = 0u;
    if (!ray_ok(org, dir, tmin, tmax)) return false;
    const V3 inv = v3(1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z);
    float t0, t1;
    V3 nearT, farT;
    if (!box_hit(node_box(nodes[0]), org, inv, tmin, tmax, t0, t1, nearT, farT)) return false;
    const RayFrame fr = ray_frame(dir);
    const float recSq = 1.0f / fr.dirSq;
    uint32_t cur = 0u;
    while (true) {
        const Node n = nodes[cur];
        bool popNext = true;
        if (n.count != 0u) {
            const uint32_t prim = n.first;
            const float bound = (best.prim != kInvalid && prim < best.prim) ? next_up(best.t) : best.t;
            Hit h;
            Stats s;
            s.aabbTests = 0u; s.leafTests = 0u;
            uint32_t iterations;
            ++ts.primTests;
            const bool got = intersect(records[prim], map, p, org, dir, fr.d1, fr.d2, recSq, tmin, bound, h, s, iterations);
            ts.aabbTests += s.aabbTests; ts.leafTests += s.leafTests;
            ts.maxIterations = iterations > ts.maxIterations ? iterations : ts.maxIterations;
            if (got) {
                best.t = h.t; best.bcB = h.bcB; best.bcC = h.bcC; best.prim = prim; best.normal = h.normal; best.frontFace = h.frontFace;
                if (kAny) return true;
            }
        }
        else {
            float a0, a1, b0, b1;
            const bool hitA = box_hit(node_box(nodes[n.first]), org, inv, tmin, best.t, a0, a1, nearT, farT);
            const bool hitB = box_hit(node_box(nodes[n.first + 1u]), org, inv, tmin, best.t, b0, b1, nearT, farT);
            if (hitA && hitB) {
                const bool aFirst = a0 <= b0;
                stack.push(aFirst ? n.first + 1u : n.first, aFirst ? b0 : a0);
                cur = aFirst ? n.first : n.first + 1u;
                popNext = false;
            }
            else if (hitA || hitB) { cur = hitA ? n.first : n.first + 1u; popNext = false; }
        }
        if (popNext) {
            bool have = false;
            while (!stack.empty()) {
                float entry;
                stack.pop(cur, entry);
                if (entry <= best.t) { have = true; break; }
            }
            if (!have) break;
        }
    }
    return best.prim != kInvalid;
}

} // namespace nrtdsm
} // namespace gfx
