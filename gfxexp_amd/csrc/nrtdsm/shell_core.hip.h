// shell_core.hip.h -- shell mapping, the second half of NRTDSM: a small triangle mesh authored in a unit tile of shell space
// (u, v, h) is repeated over a base mesh like a texture and intersected without ever being instantiated.  The arithmetic shared by
// the device kernels (shell.hip) and the host (shell_build.h, tests/shell_host.cpp).  A shell-space point (u, v, h) lies at
//     S = P(alpha, beta) + (baseHeight + heightScale h) N(alpha, beta),
// (alpha, beta) the barycentrics of (u, v) in the base triangle's texture footprint; P and N interpolate linearly, N is NOT
// renormalised.  Tile (i, j), for any integers, holds the shell mesh shifted by (i, j, 0).
//
// From nrtdsm_core.hip.h, unchanged and not restated: the prism and its record, prism_range, ray_poly, box_range, the bounded
// cubic solver, micro_triangle (which takes any (u, v, h) triangle), Stack3, ray_ok.  The record's root fields hold the tile
// roots: nrtdsm::make_record with maxDepth 0 is the reference's findRootsForShellMapping (level L >= 0 is a square of 2^L tiles).
//
// Restated from the reference in this project's own types:
//     nrtdsm/nrtdsm_shared.h:917-943                              findRootsForShellMapping                 -> nrtdsm::make_record(.., 0)
//     nrtdsm/gpu_kernels/nrtdsm_preprocess_kernels.cu:85-140      traverseShellBvh                         -> tile_heights()
//                                                    :143-357     computeAABBs_generic<true>               -> prim_bounds()
//     nrtdsm/gpu_kernels/nrtdsm_intersection_kernels.h:1263-1519  testNonlinearRayVsShellBvh               -> traverse()
//                                                     :1632-2220  detailedSurface_generic<., true>         -> intersect()
// Where this differs from the reference, on purpose (besides what nrtdsm_core.hip.h lists, which holds here too):
//   * the shell BVH is the tree's own binary one (tfdm::Node, two 16-byte loads, one triangle per leaf) and not the 8-wide one of
//     :1284-1313: the traversal keeps one entry per level in an LDS column and no ordering words;
//   * a shell node's box is tested with plane solves of its own that are clipped to the shell's height range [hLo, hHi] (the
//     reference clips every plane solve to [0, 1], :882-960, and loses a shell mesh that is taller than it is wide);
//   * the rectangle / triangle test of a shell node is closed: a box of no width (an axis-aligned wall of the shell mesh) that
//     touches the footprint is entered (testTriangleRectangleIntersection2D, nrtdsm_shared.h:868-915, calls it outside);
//   * the normal points to the side the shell triangle's winding faces in shell space ((u, v, h) right-handed), whatever the base
//     triangle's parametrisation: it is the object-space gradient of the triangle's plane function, and a gradient does not know
//     about mirrored texture coordinates (the reference negates for them, :2076);
//   * frontFace = dot(dir, n) < 0 (:2210 has <=);
//   * every loop is bounded: tile descent and node visits together stop after kMaxDescent iterations per base triangle and ray.
//
// Plain C++17 under the project's math contract, as nrtdsm_core.hip.h.  No local array is indexed at run time.
#pragma once
#include "nrtdsm_core.hip.h"

namespace gfx {
namespace shell {

using namespace nrtdsm;
using nrtdsm::TraceStats;          // tfdm's has no iteration count

constexpr uint32_t kMaxShellTriangles = 1u << 20;
constexpr uint32_t kMaxGeoms = 8u;                 // the reference's material slots per shell
constexpr float kMaxTileCoord = 4194304.0f;        // |texture coordinate| < 2^22: the root level stays below kStackLevels

// One triangle of the shell mesh in (u, v, h); `geom` is the index of the geometry it came from.  A leaf of the shell BVH names
// its triangle by its index in the concatenation of the geometries.
struct alignas(16) ShellTri { float a[3], b[3], c[3]; uint32_t geom; uint32_t pad[2]; };
static_assert(sizeof(ShellTri) == 48, "ShellTri is three 16-byte loads");

struct ShellMap { const Node* nodes; const ShellTri* tris; };
struct ShellHit { float t, bcB, bcC; V3 normal; uint32_t frontFace, tri, geom; int32_t tileX, tileY; };
struct TraceShellHit { float t, bcB, bcC; uint32_t prim; V3 normal; uint32_t frontFace, tri, geom; int32_t tileX, tileY; };

// ---------------------------------------------------------------- rectangle against the footprint, closed
// interiors and borders disjoint / rectangle inside the triangle / anything else.  The corners are used as they are stored.
GFX_TFDM_FN bool rect_edge_outside(V2 a, V2 b, float s, V2 lo, V2 hi) {
    const V2 en = v2(s * (b.y - a.y), s * (a.x - b.x));                      // outward
    const V2 c = v2(en.x >= 0.0f ? lo.x : hi.x, en.y >= 0.0f ? lo.y : hi.y);  // the corner furthest inward
    return en.x * (c.x - a.x) + en.y * (c.y - a.y) > 0.0f;
}
GFX_TFDM_FN bool rect_corner_beyond(const Footprint& f, float s, V2 c) {
    return s * cross2(f.b - f.a, c - f.a) < 0.0f || s * cross2(f.c - f.b, c - f.b) < 0.0f || s * cross2(f.a - f.c, c - f.c) < 0.0f;
}
GFX_TFDM_FN int classify_rect(const Footprint& f, V2 lo, V2 hi) {
    if (hi.x < f.lo.x || lo.x > f.hi.x || hi.y < f.lo.y || lo.y > f.hi.y) return kOutside;
    const float s = f.flipped ? -1.0f : 1.0f;
    if (rect_edge_outside(f.a, f.b, s, lo, hi) || rect_edge_outside(f.b, f.c, s, lo, hi) || rect_edge_outside(f.c, f.a, s, lo, hi)) return kOutside;
    if (rect_corner_beyond(f, s, lo) || rect_corner_beyond(f, s, v2(hi.x, lo.y)) || rect_corner_beyond(f, s, v2(lo.x, hi.y)) || rect_corner_beyond(f, s, hi)) return kOverlapping;
    return kInside;
}

// ---------------------------------------------------------------- the curved ray against one box in (u, v, h)
// nrtdsm::solve_plane with the clip range given: [cLo, cHi] must hold the box's own height range
GFX_TFDM_FN PlaneSolve solve_plane_in(float a2, float a1, float a0, float b2, float b1, float b0, const RayPoly& q, float plane, float cLo, float cHi) {
    PlaneSolve s;
    solve_quadratic(a2 - plane * q.dn2, a1 - plane * q.dn1, a0 - plane * q.dn0, cLo, cHi, s.h0, s.h1);
    s.w0 = finite_(s.h0) ? quad(b2, b1, b0, s.h0) / quad(q.dn2, q.dn1, q.dn0, s.h0) : nan_();
    s.w1 = finite_(s.h1) ? quad(b2, b1, b0, s.h1) / quad(q.dn2, q.dn1, q.dn0, s.h1) : nan_();
    return s;
}
GFX_TFDM_FN bool curve_box(const Prism& P, const RayPoly& q, V3 org, V3 dir, float recSq, float uLo, float uHi, float vLo, float vHi, float hLo, float hHi,
                           float distMin, float distMax, float& d0, float& d1) {
    const PlaneSolve sULo = solve_plane_in(q.tu2, q.tu1, q.tu0, q.tv2, q.tv1, q.tv0, q, uLo, hLo, hHi);
    const PlaneSolve sUHi = solve_plane_in(q.tu2, q.tu1, q.tu0, q.tv2, q.tv1, q.tv0, q, uHi, hLo, hHi);
    const PlaneSolve sVLo = solve_plane_in(q.tv2, q.tv1, q.tv0, q.tu2, q.tu1, q.tu0, q, vLo, hLo, hHi);
    const PlaneSolve sVHi = solve_plane_in(q.tv2, q.tv1, q.tv0, q.tu2, q.tu1, q.tu0, q, vHi, hLo, hHi);
    return box_range(P, q, org, dir, recSq, uLo, uHi, vLo, vHi, hLo, hHi, sULo, sUHi, sVLo, sVHi, distMin, distMax, d0, d1);
}
GFX_TFDM_FN V3 tri_vertex(const float* p, float sx, float sy) { return v3(p[0] + sx, p[1] + sy, p[2]); }

// ---------------------------------------------------------------- the shell BVH by the curve (:1263-1519)
// The shell mesh shifted into tile (tileX, tileY) against the curved ray.  A child's box is tested first against the footprint
// (a box outside the base triangle is skipped with its subtree), then by the curve; the nearer child, by the mid distance of its
// interval, is visited first and the other waits on `stack` with its entry distance.  tmax is the best hit so far.  `stack` is
// empty on entry and on return.  Returns whether a closer hit was found.
template <bool kAny, class Stack>
GFX_TFDM_FN bool traverse(const Prism& P, const Footprint& f, const RayPoly& q, const ShellMap& map, int tileX, int tileY, V3 org, V3 dir, float recSq, float distMin,
                          V3 e0, V3 e1, Stack& stack, float& hitDist, float& hitAlpha, float& hitBeta, V3& hitNormal, uint32_t& hitTri, Stats& stats,
                          uint32_t& iterations) {
    const float sx = static_cast<float>(tileX), sy = static_cast<float>(tileY);
    bool found = false;
    uint32_t cur = 0u;
    {
        const Node n = map.nodes[0];
        const V2 lo = v2(n.lo[0] + sx, n.lo[1] + sy), hi = v2(n.hi[0] + sx, n.hi[1] + sy);
        if (classify_rect(f, lo, hi) == kOutside) return false;
        ++stats.aabbTests;
        float d0, d1;
        if (!curve_box(P, q, org, dir, recSq, lo.x, hi.x, lo.y, hi.y, n.lo[2], n.hi[2], distMin, hitDist, d0, d1)) return false;
    }
    while (true) {
        if (++iterations > kMaxDescent) { while (!stack.empty()) { float e; stack.pop(cur, e); } return found; }
        const Node n = map.nodes[cur];
        bool popNext = true;
        if (n.count != 0u) {
            ++stats.leafTests;
            const ShellTri t = map.tris[n.first];
            if (micro_triangle(P, f.a, f.b, f.c, tri_vertex(t.a, sx, sy), tri_vertex(t.b, sx, sy), tri_vertex(t.c, sx, sy), org, dir, recSq, distMin, e0, e1, q,
                               hitDist, hitAlpha, hitBeta, hitNormal)) {
                found = true;
                hitTri = n.first;
                if (kAny) { while (!stack.empty()) { float e; stack.pop(cur, e); } return true; }
            }
        }
        else {
            float a0 = 0.0f, a1 = 0.0f, b0 = 0.0f, b1 = 0.0f;
            bool hitA, hitB;
            {
                const Node c = map.nodes[n.first];
                const V2 lo = v2(c.lo[0] + sx, c.lo[1] + sy), hi = v2(c.hi[0] + sx, c.hi[1] + sy);
                hitA = classify_rect(f, lo, hi) != kOutside;
                if (hitA) { ++stats.aabbTests; hitA = curve_box(P, q, org, dir, recSq, lo.x, hi.x, lo.y, hi.y, c.lo[2], c.hi[2], distMin, hitDist, a0, a1); }
            }
            {
                const Node c = map.nodes[n.first + 1u];
                const V2 lo = v2(c.lo[0] + sx, c.lo[1] + sy), hi = v2(c.hi[0] + sx, c.hi[1] + sy);
                hitB = classify_rect(f, lo, hi) != kOutside;
                if (hitB) { ++stats.aabbTests; hitB = curve_box(P, q, org, dir, recSq, lo.x, hi.x, lo.y, hi.y, c.lo[2], c.hi[2], distMin, hitDist, b0, b1); }
            }
            if (hitA && hitB) {
                const bool aFirst = 0.5f * (a0 + a1) <= 0.5f * (b0 + b1);
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
                if (entry <= hitDist) { have = true; break; }        // entered behind the current hit: skipped
            }
            if (!have) break;
        }
    }
    return found;
}

// ---------------------------------------------------------------- the intersection routine (detailedSurface_generic<., true>)
// The shell-mapped surface over one base triangle against the ray (org, dir) inside (tmin, tmax).  The tiles are walked as a
// quadtree whose every square has the height range of the shell BVH's root; at level 0 the shell BVH is traversed with the
// tile's shift.  `hit` is written only when a hit closer than tmax was found.
template <bool kAny, class Stack>
GFX_TFDM_FN bool intersect(const PrismRecord& r, const ShellMap& map, const Params& p, V3 org, V3 dir, V3 e0, V3 e1, float recSq, float tmin, float tmax,
                           Stack& shellStack, ShellHit& hit, Stats& stats, uint32_t& iterations) {
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
    const float hLo = map.nodes[0].lo[2], hHi = map.nodes[0].hi[2];
    bool found = false;
    float hitAlpha = 0.0f, hitBeta = 0.0f;
    V3 hitNormal = v3(0.0f, 0.0f, 0.0f);
    uint32_t hitTri = 0u;
    int hitTileX = 0, hitTileY = 0;
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
            const float scale = pow2i(cur.lod);
            const V2 centre = v2((static_cast<float>(cur.x) + 0.5f) * scale, (static_cast<float>(cur.y) + 0.5f) * scale);
            // a square of tiles outside the base triangle is skipped with everything in it
            if (classify(f, centre, 0.5f * scale) == kOutside) { entry = kNoEntry; continue; }
            if (cur.lod > 0) {
                const float u0 = static_cast<float>(cur.x) * scale, u1 = centre.x, u2 = (static_cast<float>(cur.x) + 1.0f) * scale;
                const float v0 = static_cast<float>(cur.y) * scale, v1 = centre.y, v2_ = (static_cast<float>(cur.y) + 1.0f) * scale;
                down(cur);
                float dist0 = inf(), dist1 = inf(), dist2 = inf(), dist3 = inf();
                uint32_t numValid = 0u;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
                for (uint32_t i = 0; i < 4u; ++i) {
                    ++stats.aabbTests;
                    const bool uHalf = (i & 1u) != 0u, vHalf = (i >> 1) != 0u;
                    float d0, d1;
                    const bool in = curve_box(P, q, org, dir, recSq, uHalf ? u1 : u0, uHalf ? u2 : u1, vHalf ? v1 : v0, vHalf ? v2_ : v1, hLo, hHi, distMin, hitDist, d0, d1);
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
            if (traverse<kAny>(P, f, q, map, cur.x, cur.y, org, dir, recSq, distMin, e0, e1, shellStack, hitDist, hitAlpha, hitBeta, hitNormal, hitTri, stats, iterations)) {
                found = true; hitTileX = cur.x; hitTileY = cur.y;
            }
            if (iterations > kMaxDescent) return false;
            if (kAny && found) { rootIdx = r.numRoots; break; }
            entry = kNoEntry;
        }
    }
    if (!found) return false;
    hit.t = hitDist; hit.bcB = hitAlpha; hit.bcC = hitBeta;
    hit.normal = neg(hitNormal);             // micro_triangle's normal lies against the winding (on the side of +h for a height field)
    hit.frontFace = dot(dir, hit.normal) < 0.0f ? 1u : 0u;
    hit.tri = hitTri; hit.geom = map.tris[hitTri].geom; hit.tileX = hitTileX; hit.tileY = hitTileY;
    return true;
}

// ---------------------------------------------------------------- per-triangle heights and box (computeAABBs_generic<true>)
// The heights of the shell mesh in tile (tileX, tileY) over the footprint: the union of [lo.h, hi.h] over the nodes that lie
// inside the footprint and the leaves that overlap it (:85-140).  `stack` is empty on entry and on return.
template <class Stack>
GFX_TFDM_FN void tile_heights(const Footprint& f, const ShellMap& map, int tileX, int tileY, Stack& stack, float& minH, float& maxH, uint32_t& iterations) {
    const float sx = static_cast<float>(tileX), sy = static_cast<float>(tileY);
    stack.push(0u, 0.0f);
    while (!stack.empty()) {
        uint32_t cur;
        float unused;
        stack.pop(cur, unused);
        if (++iterations > kMaxDescent) continue;          // the caller takes the root's range
        const Node n = map.nodes[cur];
        const int k = classify_rect(f, v2(n.lo[0] + sx, n.lo[1] + sy), v2(n.hi[0] + sx, n.hi[1] + sy));
        if (k == kOutside) continue;
        if (k == kInside || n.count != 0u) { minH = fmin_(minH, n.lo[2]); maxH = fmax_(maxH, n.hi[2]); continue; }
        stack.push(n.first + 1u, 0.0f);
        stack.push(n.first, 0.0f);
    }
}

// min / max of the shell mesh over the footprint in every tile it overlaps, then the union of the six prism corners.  Writes
// minHeight / amplitude; a footprint that no shell geometry overlaps gets no roots and an empty box.
template <class Stack>
GFX_TFDM_FN Box prim_bounds(PrismRecord& r, const ShellMap& map, const Params& p, Stack& stack) {
    const Footprint f = footprint(r);
    const float rootLo = map.nodes[0].lo[2], rootHi = map.nodes[0].hi[2];
    float minH = inf(), maxH = -inf();
    uint32_t iterations = 0u;
    bool whole = false;
    for (uint32_t rootIdx = 0; rootIdx < r.numRoots && !whole; ++rootIdx) {
        Texel cur = root_texel(r, rootIdx);
        Texel end = cur;
        const int initialLod = cur.lod;
        next(end, false, false, initialLod);
        while (!same(cur, end)) {
            if (++iterations > kMaxDescent) { whole = true; break; }
            const float scale = pow2i(cur.lod);
            const int k = classify(f, v2((static_cast<float>(cur.x) + 0.5f) * scale, (static_cast<float>(cur.y) + 0.5f) * scale), 0.5f * scale);
            if (k == kOutside) next(cur, false, false, initialLod);
            else if (k == kInside) { whole = true; break; }             // one whole tile at least lies inside the triangle
            else if (cur.lod > 0) down(cur);
            else {
                tile_heights(f, map, cur.x, cur.y, stack, minH, maxH, iterations);
                if (minH <= rootLo && maxH >= rootHi) { whole = true; break; }
                next(cur, false, false, initialLod);
            }
        }
    }
    if (whole) { minH = rootLo; maxH = rootHi; }
    Box out;
    out.lo = v3(inf(), inf(), inf());
    out.hi = v3(-inf(), -inf(), -inf());
    r.minHeight = 0.0f; r.amplitude = 0.0f;
    if (!(minH <= maxH)) { r.numRoots = 0u; return out; }
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

// ---------------------------------------------------------------- one ray through the tree over the per-triangle boxes
// As nrtdsm::trace_ray: closest hit (kAny: any hit); equal distances go to the lower primitive index.  `stack` serves the base
// tree, `shellStack` the shell BVH.
template <bool kAny, class Stack>
GFX_TFDM_FN bool trace_ray(const Node* nodes, const PrismRecord* records, const ShellMap& map, const Params& p, V3 org, V3 dir, float tmin, float tmax, Stack& stack,
                           Stack& shellStack, TraceShellHit& best, TraceStats& ts) {
    best.t = tmax; best.bcB = 0.0f; best.bcC = 0.0f; best.prim = kInvalid; best.normal = v3(0.0f, 0.0f, 0.0f); best.frontFace = 0u;
    best.tri = 0u; best.geom = 0u; best.tileX = 0; best.tileY = 0;
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
            ShellHit h;
            Stats s;
            s.aabbTests = 0u; s.leafTests = 0u;
            uint32_t iterations;
            ++ts.primTests;
            const bool got = intersect<kAny>(records[prim], map, p, org, dir, fr.d1, fr.d2, recSq, tmin, bound, shellStack, h, s, iterations);
            ts.aabbTests += s.aabbTests; ts.leafTests += s.leafTests;
            ts.maxIterations = iterations > ts.maxIterations ? iterations : ts.maxIterations;
            if (got) {
                best.t = h.t; best.bcB = h.bcB; best.bcC = h.bcC; best.prim = prim; best.normal = h.normal; best.frontFace = h.frontFace;
                best.tri = h.tri; best.geom = h.geom; best.tileX = h.tileX; best.tileY = h.tileY;
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

} // namespace shell
} // namespace gfx
