// shell_build.h -- host-only set-up of a shell-mapped object (csrc/nrtdsm/shell.hip and tests/shell_host.cpp include it): the
// shell BVH over the shell mesh and what gfx_shell_create / set_geometry / set_params refuse.  The tree is tfdm::build_tree over
// the shell triangles' (u, v, h) boxes: a balanced binary tree of 32-byte nodes with one triangle per leaf, at most 20 deep.
// The per-triangle records are nrtdsm::make_record with maxDepth 0 (the tile roots); the parameters are TFDM's with size 1.
#pragma once
#include <string>
#include "nrtdsm_build.h"
#include "shell_core.hip.h"

namespace gfx {
namespace shell {

struct ShellBvh {
    std::vector<Node> nodes;
    std::vector<ShellTri> tris;       // the geometries behind one another, in the order given
};

// the longest path from `node` down to a leaf, in edges
inline int tree_depth(const std::vector<Node>& nodes) {
    struct Work { uint32_t node; int depth; };
    std::vector<Work> work{ { 0u, 0 } };
    int deepest = 0;
    while (!work.empty()) {
        const Work w = work.back();
        work.pop_back();
        deepest = std::max(deepest, w.depth);
        const Node& n = nodes[w.node];
        if (n.count == 0u) { work.push_back({ n.first, w.depth + 1 }); work.push_back({ n.first + 1u, w.depth + 1 }); }
    }
    return deepest;
}

// The shell BVH of the geometries, or why there is none (`out` is then untouched).  A flat mesh (every h equal, h = 0 included)
// is a decal and is accepted: its boxes have no height and the curve meets them in their one height plane.
inline const char* build_shell(const gfx_shell_geom* geoms, uint32_t numGeoms, ShellBvh& out) {
    if (!geoms || numGeoms == 0u) return "no shell geometry";
    if (numGeoms > kMaxGeoms) return "more than 8 shell geometries";
    uint64_t total = 0;
    for (uint32_t g = 0; g < numGeoms; ++g) {
        if (!geoms[g].positions || !geoms[g].triangles) return "a shell geometry has null positions or triangles";
        if (geoms[g].stride < 3u * sizeof(float)) return "a shell geometry's stride is smaller than three floats";
        total += geoms[g].numTriangles;
    }
    if (total == 0u) return "the shell mesh has no triangles";
    if (total > kMaxShellTriangles) return "more than 2^20 shell triangles";
    ShellBvh b;
    b.tris.reserve(static_cast<size_t>(total));
    std::vector<float> boxes;
    boxes.reserve(6 * static_cast<size_t>(total));
    for (uint32_t g = 0; g < numGeoms; ++g) {
        const uint8_t* base = reinterpret_cast<const uint8_t*>(geoms[g].positions);
        for (uint32_t t = 0; t < geoms[g].numTriangles; ++t) {
            ShellTri tri;
            std::memset(&tri, 0, sizeof(tri));
            float* dst[3] = { tri.a, tri.b, tri.c };
            for (int k = 0; k < 3; ++k) {
                const uint32_t vi = geoms[g].triangles[3 * t + k];
                if (vi >= geoms[g].numVertices) return "a shell triangle refers to a vertex that does not exist";
                std::memcpy(dst[k], base + static_cast<size_t>(geoms[g].stride) * vi, 3 * sizeof(float));
                for (int c = 0; c < 3; ++c) if (!std::isfinite(dst[k][c])) return "a shell vertex is not finite";
                if (!(dst[k][0] >= 0.0f && dst[k][0] <= 1.0f && dst[k][1] >= 0.0f && dst[k][1] <= 1.0f)) return "a shell vertex has u or v outside [0, 1] (the shell mesh lives in the unit tile)";
            }
            tri.geom = g;
            for (int c = 0; c < 3; ++c) boxes.push_back(std::min(tri.a[c], std::min(tri.b[c], tri.c[c])));
            for (int c = 0; c < 3; ++c) boxes.push_back(std::max(tri.a[c], std::max(tri.b[c], tri.c[c])));
            b.tris.push_back(tri);
        }
    }
    b.nodes = build_tree(boxes.data(), static_cast<uint32_t>(total));
    // trace and prim_bounds keep at most depth + 1 entries of the shell BVH at a time
    if (tree_depth(b.nodes) + 1 > kStackDepth) return "the shell BVH is deeper than the device stack holds";
    out = std::move(b);
    return nullptr;
}

// nullptr when the parameters are fine: NRTDSM's refusals
inline const char* refuse_params(const gfx_tfdm_params& g) {
    if (g.targetMipLevel != 0u) return "targetMipLevel must be 0 (a shell mesh has no levels)";
    if (g.localIntersection != 0u) return "localIntersection must be 0 (a shell mesh has one intersection, the shell triangle's cubic)";
    gfx_tfdm_params c = g;
    c.localIntersection = tfdm::kTwoTriangle;
    return nrtdsm::refuse_params(c);
}
inline Params make_shell_params(const gfx_tfdm_params& g) {
    gfx_tfdm_params c = g;
    c.localIntersection = tfdm::kTwoTriangle;
    return tfdm::make_params(c, 1u);
}
inline PrismRecord make_shell_record(const float pA[3], const float pB[3], const float pC[3], const float nA[3], const float nB[3], const float nC[3],
                                     const float tA[2], const float tB[2], const float tC[2], const gfx_tfdm_params& g) {
    return nrtdsm::make_record(pA, pB, pC, nA, nB, nC, tA, tB, tC, g, 0);
}
inline bool tile_coords_in_range(const PrismRecord& r) {
    for (float c : r.tc) if (std::isfinite(c) && fabsf(c) >= kMaxTileCoord) return false;
    return true;
}

} // namespace shell
} // namespace gfx
