// tfdm_build.h -- host-only set-up of a displaced object (csrc/tfdm/displaced_object.h and tests/tfdm_host.cpp include it): the derived
// parameters, the height mips, the per-triangle records and the tree over the per-triangle boxes.
//
// The records follow tfdm/tfdm_main.cpp:780-843 (matObjToTcTang, matTcToBc, matTcToNInObj in double, stored as float) and then
// fold in what tfdm_intersection_kernels.h:54-90 recomputes per call: the texture transform and its inverse, the transformed
// texture coordinates, the reciprocal area, the flip flag and findRoots (tfdm_shared.h:867-897).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "gfxexp.h"
#include "tfdm_core.hip.h"

namespace gfx {
namespace tfdm {

// kernels.h:54-59; decompose() of a T R S matrix returns the scale it was built from, so preScale comes straight from texScale
inline Params make_params(const gfx_tfdm_params& g, uint32_t size) {
    Params p;
    std::memset(&p, 0, sizeof(p));
    const float preScale = 1.0f / sqrtf(g.texScale[0] * g.texScale[1]);
    p.baseHeight = g.hOffset - preScale * g.hScale * g.hBias;
    p.heightScale = preScale * g.hScale;
    p.maxDepth = floor_log2(size);
    p.targetMipLevel = static_cast<int32_t>(g.targetMipLevel);
    p.local = g.localIntersection;
    return p;
}

// All levels behind one another (level_offset).  One level given: the coarser ones are the 2 x 2 mean ((a + b) + (c + d)) * 0.25f.
inline std::vector<float> make_levels(const float* const* levels, uint32_t numLevels, uint32_t size) {
    const int maxDepth = floor_log2(size);
    std::vector<float> out(total_texels(maxDepth));
    for (int l = 0; l <= maxDepth; ++l) {
        const uint32_t w = size >> l;
        float* dst = out.data() + level_offset(maxDepth, l);
        if (static_cast<uint32_t>(l) < numLevels && (l == 0 || numLevels > 1)) { std::memcpy(dst, levels[l], sizeof(float) * w * w); continue; }
        const float* src = out.data() + level_offset(maxDepth, l - 1);
        for (uint32_t y = 0; y < w; ++y)
            for (uint32_t x = 0; x < w; ++x) {
                const float a = src[(2 * y) * 2 * w + 2 * x], b = src[(2 * y) * 2 * w + 2 * x + 1];
                const float c = src[(2 * y + 1) * 2 * w + 2 * x], d = src[(2 * y + 1) * 2 * w + 2 * x + 1];
                dst[y * w + x] = ((a + b) + (c + d)) * 0.25f;
            }
    }
    return out;
}

// translate(offset) * rotate(degrees) * scale, tfdm_main.cpp:2581-2584; row-major 3 x 3 in double
inline void texture_transform(const gfx_tfdm_params& g, double m[9]) {
    const double a = static_cast<double>(g.texRotation) * 3.14159265358979323846 / 180.0;
    const double c = std::cos(a), s = std::sin(a);
    m[0] = c * g.texScale[0]; m[1] = -s * g.texScale[1]; m[2] = g.texOffset[0];
    m[3] = s * g.texScale[0]; m[4] = c * g.texScale[1];  m[5] = g.texOffset[1];
    m[6] = 0.0; m[7] = 0.0; m[8] = 1.0;
}

inline bool invert3(const double m[9], double out[9]) {
    const double c0 = m[4] * m[8] - m[5] * m[7], c1 = m[5] * m[6] - m[3] * m[8], c2 = m[3] * m[7] - m[4] * m[6];
    const double det = m[0] * c0 + m[1] * c1 + m[2] * c2;
    if (det == 0.0 || !std::isfinite(det)) return false;
    const double r = 1.0 / det;
    out[0] = c0 * r; out[1] = (m[2] * m[7] - m[1] * m[8]) * r; out[2] = (m[1] * m[5] - m[2] * m[4]) * r;
    out[3] = c1 * r; out[4] = (m[0] * m[8] - m[2] * m[6]) * r; out[5] = (m[2] * m[3] - m[0] * m[5]) * r;
    out[6] = c2 * r; out[7] = (m[1] * m[6] - m[0] * m[7]) * r; out[8] = (m[0] * m[4] - m[1] * m[3]) * r;
    return true;
}

// findRoots (tfdm_shared.h:867-897) on the footprint's bounds, in float as there
inline void find_roots(TriRecord& r, int maxDepth, int targetMipLevel) {
    const Footprint f = footprint(r);
    const float dx = f.hi.x - f.lo.x, dy = f.hi.y - f.lo.y;
    const float d = dy > dx ? dy : dx;
    r.numRoots = 0;
    // no roots (the triangle is never hit) where a texel index of the finest level would leave the range a float holds exactly;
    // gfx_tfdm_create / set_params refuse such coordinates, this keeps the walk finite for whoever calls the core directly
    const float lim = kMaxTexelCoord * pow2i(-maxDepth);
    if (!(d > 0.0f) || !(fabsf(f.lo.x) < lim) || !(fabsf(f.lo.y) < lim) || !(fabsf(f.hi.x) < lim) || !(fabsf(f.hi.y) < lim)) return;
    const float recD = 1.0f / d;
    int start = maxDepth - (recD >= 2147483648.0f ? 31 : floor_log2(static_cast<uint32_t>(recD))) - 1;
    start = std::max(start, 0);
    while (true) {
        const int k = maxDepth - start;
        const float res = k >= -126 ? pow2i(k) : 0.0f;
        const int minX = static_cast<int>(floorf(res * f.lo.x)), minY = static_cast<int>(floorf(res * f.lo.y));
        const int maxX = static_cast<int>(floorf(res * f.hi.x)), maxY = static_cast<int>(floorf(res * f.hi.y));
        if (maxX - minX < 2 && maxY - minY < 2 && start >= targetMipLevel) {
            r.rootMinX = minX; r.rootMinY = minY; r.rootMaxX = maxX; r.rootMaxY = maxY; r.rootLod = start;
            r.numRoots = static_cast<uint32_t>((maxX - minX + 1) * (maxY - minY + 1));
            return;
        }
        ++start;
    }
}

// One record; positions / normals / texture coordinates of the three vertices as the caller's floats.
inline TriRecord make_record(const float pA[3], const float pB[3], const float pC[3], const float nA[3], const float nB[3], const float nC[3],
                             const float tA[2], const float tB[2], const float tC[2], const gfx_tfdm_params& g, int maxDepth) {
    TriRecord r;
    std::memset(&r, 0, sizeof(r));
    double X[9];
    texture_transform(g, X);
    const double P[3][3] = { { pA[0], pA[1], pA[2] }, { pB[0], pB[1], pB[2] }, { pC[0], pC[1], pC[2] } };
    const double N[3][3] = { { nA[0], nA[1], nA[2] }, { nB[0], nB[1], nB[2] }, { nC[0], nC[1], nC[2] } };
    const double T[3][2] = { { tA[0], tA[1] }, { tB[0], tB[1] }, { tC[0], tC[1] } };
    // tangent frame of the untransformed texture coordinates (tfdm_main.cpp:790-819)
    double dp01[3], dp02[3], gn[3];
    for (int k = 0; k < 3; ++k) { dp01[k] = P[1][k] - P[0][k]; dp02[k] = P[2][k] - P[0][k]; }
    gn[0] = dp01[1] * dp02[2] - dp01[2] * dp02[1]; gn[1] = dp01[2] * dp02[0] - dp01[0] * dp02[2]; gn[2] = dp01[0] * dp02[1] - dp01[1] * dp02[0];
    const double gl = std::sqrt(gn[0] * gn[0] + gn[1] * gn[1] + gn[2] * gn[2]);
    const double dt01[2] = { T[1][0] - T[0][0], T[1][1] - T[0][1] }, dt02[2] = { T[2][0] - T[0][0], T[2][1] - T[0][1] };
    const double det = dt01[0] * dt02[1] - dt01[1] * dt02[0];
    if (!(gl > 0.0) || det == 0.0 || !std::isfinite(det)) return r;        // degenerate in space or in texture space: numRoots stays 0
    for (int k = 0; k < 3; ++k) gn[k] /= gl;
    const double recDet = 1.0 / det;
    double F[9];                                                           // columns tc0Dir, tc1Dir, geometric normal
    for (int k = 0; k < 3; ++k) {
        F[3 * k + 0] = recDet * (dt02[1] * dp01[k] - dt01[1] * dp02[k]);
        F[3 * k + 1] = recDet * (-dt02[0] * dp01[k] + dt01[0] * dp02[k]);
        F[3 * k + 2] = gn[k];
    }
    double Fi[9];
    if (!invert3(F, Fi)) return r;
    double M[12];                                                          // object -> untransformed tangent space, 3 x 4 (:827-830)
    for (int row = 0; row < 3; ++row) {
        for (int c = 0; c < 3; ++c) M[4 * row + c] = Fi[3 * row + c];
        const double at = row < 2 ? T[0][row] : 0.0;
        M[4 * row + 3] = at - (Fi[3 * row] * P[0][0] + Fi[3 * row + 1] * P[0][1] + Fi[3 * row + 2] * P[0][2]);
    }
    // ... composed with the texture transform on (u, v) (kernels.h:88-90)
    for (int c = 0; c < 4; ++c) {
        const double u = X[0] * M[c] + X[1] * M[4 + c] + (c == 3 ? X[2] : 0.0);
        const double v = X[3] * M[c] + X[4] * M[4 + c] + (c == 3 ? X[5] : 0.0);
        r.objToTang[c] = static_cast<float>(u);
        r.objToTang[4 + c] = static_cast<float>(v);
        r.objToTang[8 + c] = static_cast<float>(M[8 + c]);
    }
    // transformed texture coordinates; (u, v, 1) -> barycentrics is the inverse of their matrix (:832, kernels.h:80-81)
    double tc[3][2];
    for (int v = 0; v < 3; ++v) {
        tc[v][0] = X[0] * T[v][0] + X[1] * T[v][1] + X[2];
        tc[v][1] = X[3] * T[v][0] + X[4] * T[v][1] + X[5];
        r.tc[2 * v] = static_cast<float>(tc[v][0]);
        r.tc[2 * v + 1] = static_cast<float>(tc[v][1]);
    }
    const double B[9] = { tc[0][0], tc[1][0], tc[2][0], tc[0][1], tc[1][1], tc[2][1], 1.0, 1.0, 1.0 };
    double Bi[9];
    if (!invert3(B, Bi)) return r;
    for (int row = 0; row < 3; ++row)
        for (int c = 0; c < 3; ++c) {
            r.tcToN[3 * row + c] = static_cast<float>(N[0][row] * Bi[c] + N[1][row] * Bi[3 + c] + N[2][row] * Bi[6 + c]);
            r.tcToP[3 * row + c] = static_cast<float>(P[0][row] * Bi[c] + P[1][row] * Bi[3 + c] + P[2][row] * Bi[6 + c]);
        }
    // the area, its sign and the roots from the stored floats: the barycentrics of a hit are computed from these same numbers
    const float area = cross2(v2(r.tc[2] - r.tc[0], r.tc[3] - r.tc[1]), v2(r.tc[4] - r.tc[0], r.tc[5] - r.tc[1]));
    if (area == 0.0f) return r;
    r.recArea = 1.0f / area;
    r.flipped = area < 0.0f ? 1u : 0u;
    find_roots(r, maxDepth, static_cast<int>(g.targetMipLevel));
    const float* f = r.objToTang;
    for (int i = 0; i < 36; ++i) if (!std::isfinite(f[i])) r.numRoots = 0;     // objToTang, tcToN, tcToP and tc are contiguous
    return r;
}

// A balanced binary tree over the boxes (six floats each): sort the range along the longest axis of its centroids, halve it.
// A box that is empty (lo > hi) is left out.  Node 0 is the root; depth <= ceil(log2(n)) <= 20, within kStackDepth.
inline std::vector<Node> build_tree(const float* boxes, uint32_t n) {
    struct Item { float c[3]; uint32_t prim; };
    std::vector<Item> items;
    for (uint32_t i = 0; i < n; ++i) {
        const float* b = boxes + 6 * i;
        if (!(b[0] <= b[3] && b[1] <= b[4] && b[2] <= b[5])) continue;
        Item it;
        for (int k = 0; k < 3; ++k) { const float c = 0.5f * b[k] + 0.5f * b[3 + k]; it.c[k] = std::isfinite(c) ? c : 0.0f; }
        it.prim = i;
        items.push_back(it);
    }
    std::vector<Node> nodes(1);
    if (items.empty()) {                   // nothing to hit: a leaf on primitive 0, whose record has no roots
        Node& r = nodes[0];
        for (int k = 0; k < 3; ++k) { r.lo[k] = 0.0f; r.hi[k] = 0.0f; }
        r.first = 0; r.count = 1;
        return nodes;
    }
    struct Work { uint32_t node, begin, end; };
    std::vector<Work> work{ { 0u, 0u, static_cast<uint32_t>(items.size()) } };
    while (!work.empty()) {
        const Work w = work.back();
        work.pop_back();
        float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
        float clo[3] = { INFINITY, INFINITY, INFINITY }, chi[3] = { -INFINITY, -INFINITY, -INFINITY };
        for (uint32_t i = w.begin; i < w.end; ++i) {
            const float* b = boxes + 6 * items[i].prim;
            for (int k = 0; k < 3; ++k) {
                lo[k] = std::min(lo[k], b[k]); hi[k] = std::max(hi[k], b[3 + k]);
                clo[k] = std::min(clo[k], items[i].c[k]); chi[k] = std::max(chi[k], items[i].c[k]);
            }
        }
        Node nd;
        for (int k = 0; k < 3; ++k) { nd.lo[k] = lo[k]; nd.hi[k] = hi[k]; }
        if (w.end - w.begin == 1) { nd.first = items[w.begin].prim; nd.count = 1; nodes[w.node] = nd; continue; }
        int axis = 0;
        if (chi[1] - clo[1] > chi[axis] - clo[axis]) axis = 1;
        if (chi[2] - clo[2] > chi[axis] - clo[axis]) axis = 2;
        std::sort(items.begin() + w.begin, items.begin() + w.end, [axis](const Item& a, const Item& b) {
            return a.c[axis] < b.c[axis] || (a.c[axis] == b.c[axis] && a.prim < b.prim); });
        const uint32_t mid = w.begin + (w.end - w.begin) / 2;
        nd.first = static_cast<uint32_t>(nodes.size());
        nd.count = 0;
        nodes[w.node] = nd;
        nodes.resize(nodes.size() + 2);
        work.push_back({ nd.first + 1u, mid, w.end });
        work.push_back({ nd.first, w.begin, mid });
    }
    return nodes;
}

// the host's stack for trace_ray (a push beyond kStackDepth would be dropped: tfdm_core.hip.h asserts build_tree's depth fits)
struct HostStack {
    uint32_t node[kStackDepth]; float entry[kStackDepth]; int sp = 0;
    void push(uint32_t n, float e) { if (sp < kStackDepth) { node[sp] = n; entry[sp] = e; ++sp; } }
    void pop(uint32_t& n, float& e) { --sp; n = node[sp]; e = entry[sp]; }
    bool empty() const { return sp == 0; }
};

} // namespace tfdm
} // namespace gfx
