// nrtdsm_build.h -- host-only set-up of an NRTDSM object (csrc/nrtdsm/nrtdsm.hip and tests/nrtdsm_host.cpp include it): the
// per-triangle records before their heights are known, and what gfx_nrtdsm_create / set_params refuse.  Parameters, height mips,
// the texture transform, findRoots and the tree builder are TFDM's (tfdm_build.h).
#pragma once
#include "../tfdm/tfdm_build.h"
#include "nrtdsm_core.hip.h"

namespace gfx {
namespace nrtdsm {

// One record: the vertices as given, the texture coordinates through the texture transform (double, stored as float, as
// tfdm::make_record does), the roots of the footprint with target level 0.  minHeight / amplitude stay 0 until prim_bounds().
inline PrismRecord make_record(const float pA[3], const float pB[3], const float pC[3], const float nA[3], const float nB[3], const float nC[3],
                               const float tA[2], const float tB[2], const float tC[2], const gfx_tfdm_params& g, int maxDepth) {
    PrismRecord r;
    std::memset(&r, 0, sizeof(r));
    double X[9];
    tfdm::texture_transform(g, X);
    const float* P[3] = { pA, pB, pC };
    const float* N[3] = { nA, nB, nC };
    const float* T[3] = { tA, tB, tC };
    tfdm::TriRecord roots;                 // find_roots reads tc and flipped, writes the root fields
    std::memset(&roots, 0, sizeof(roots));
    for (int v = 0; v < 3; ++v) {
        for (int k = 0; k < 3; ++k) { r.pos[3 * v + k] = P[v][k]; r.nrm[3 * v + k] = N[v][k]; }
        r.tc[2 * v] = static_cast<float>(X[0] * T[v][0] + X[1] * T[v][1] + X[2]);
        r.tc[2 * v + 1] = static_cast<float>(X[3] * T[v][0] + X[4] * T[v][1] + X[5]);
        roots.tc[2 * v] = r.tc[2 * v]; roots.tc[2 * v + 1] = r.tc[2 * v + 1];
    }
    const float area = cross2(v2(r.tc[2] - r.tc[0], r.tc[3] - r.tc[1]), v2(r.tc[4] - r.tc[0], r.tc[5] - r.tc[1]));
    if (area == 0.0f || !std::isfinite(area)) return r;
    r.flipped = area < 0.0f ? 1u : 0u;
    roots.flipped = r.flipped;
    tfdm::find_roots(roots, maxDepth, 0);
    for (float x : r.pos) if (!std::isfinite(x)) return r;
    for (float x : r.nrm) if (!std::isfinite(x)) return r;
    for (float x : r.tc) if (!std::isfinite(x)) return r;
    if (roots.rootLod >= kStackLevels) return r;
    r.rootMinX = roots.rootMinX; r.rootMinY = roots.rootMinY; r.rootMaxX = roots.rootMaxX; r.rootMaxY = roots.rootMaxY; r.rootLod = roots.rootLod;
    r.numRoots = roots.numRoots;
    return r;
}

// What the query cannot run; nullptr when the parameters are fine (the caller adds its own prefix and throws)
inline const char* refuse_params(const gfx_tfdm_params& g) {
    const float fields[] = { g.hOffset, g.hScale, g.hBias, g.texScale[0], g.texScale[1], g.texRotation, g.texOffset[0], g.texOffset[1] };
    for (float f : fields) if (!std::isfinite(f)) return "a parameter is not finite";
    if (!(g.texScale[0] > 0.0f) || !(g.texScale[1] > 0.0f)) return "texScale must be positive";
    if (g.targetMipLevel != 0u) return "targetMipLevel must be 0 (the reference's NRTDSM descends to the finest level only)";
    if (g.localIntersection != tfdm::kTwoTriangle) return "localIntersection must be the default, GFX_TFDM_TWO_TRIANGLE (NRTDSM has one local intersection, the micro-triangle cubic)";
    return nullptr;
}
// the plane solves clip h to [0, 1]: every map value of every level must lie there
inline bool heights_in_unit_range(const std::vector<float>& levels) {
    for (float h : levels) if (!(h >= 0.0f && h <= 1.0f)) return false;
    return true;
}
inline bool texel_coords_in_range(const PrismRecord& r, uint32_t size) {
    for (float c : r.tc) if (std::isfinite(c) && fabsf(c) * static_cast<float>(size) >= tfdm::kMaxTexelCoord) return false;
    return true;
}

} // namespace nrtdsm
} // namespace gfx
