// tfdm_update.h -- which texels an in-place change of a height map's level 0 makes dirty, and the level-ordered table the tree
// refit walks: the host arithmetic of gfx_tfdm_update_heights / gfx_nrtdsm_update_heights (tfdm_update.hip.h launches over these
// regions; tests/tfdm_update_host.cpp runs the same regions on the host).  Plain C++17, no device code.
//
// Heights.  Level l >= 1 is the 2 x 2 mean of level l - 1, so a changed rectangle [lo, hi) of level l - 1 changes
// H_l = [floor(lo / 2), ceil(hi / 2)) of level l, per axis.  H_l never wraps and never leaves the level.
//
// Pyramid.  A pyramid texel x of level l is made from the height texels x - 1 .. x + 1 of level l (the four corner samples of
// corner_height, repeat wrap) and, above level 0, from its four children.  Its dirty set P_l is therefore H_l grown by one texel
// on every side, wrapped modulo the level's width, united with P_(l-1) halved.  It is kept as one wrapped interval per axis
// (start < width, length <= width); where a union is not an interval the shorter covering interval is taken.  Covering too much
// costs time only (the same inputs give the same bits); covering too little is the bug this header can have.
#pragma once
#include <cstdint>
#include <vector>
#include "tfdm_core.hip.h"

namespace gfx {
namespace tfdm {

struct Span { uint32_t start, len; };             // texels start, start + 1, ... (len of them) modulo the axis' width

inline Span span(uint32_t start, uint32_t len) { Span s; s.start = start; s.len = len; return s; }

// [lo, hi) of one level -> the texels of the next coarser level whose 2 x 2 mean reads any of them
inline Span halve_heights(Span s) { return span(s.start / 2u, (s.start + s.len + 1u) / 2u - s.start / 2u); }

// a span of height texels that does not wrap (start + len <= width) -> the pyramid texels of the same level that read them
inline Span grow_wrapped(Span s, uint32_t width) {
    if (s.len + 2u >= width) return span(0u, width);
    return span((s.start + width - 1u) % width, s.len + 2u);
}

// a wrapped span of a level `width` wide -> the span of their parents, a level width / 2 wide
inline Span halve_wrapped(Span s, uint32_t width) {
    const uint32_t half = width / 2u;
    if (half == 0u) return span(0u, 1u);
    if (s.len >= width) return span(0u, half);
    const uint32_t first = s.start / 2u, last = (s.start + s.len - 1u) / 2u;      // not reduced: last may lie beyond the level
    const uint32_t len = last - first + 1u;
    return len >= half ? span(0u, half) : span(first % half, len);
}

// the shorter wrapped span that covers both
inline Span unite_wrapped(Span a, Span b, uint32_t width) {
    if (a.len >= width || b.len >= width) return span(0u, width);
    if (a.len == 0u) return b;
    if (b.len == 0u) return a;
    const uint32_t offB = (b.start + width - a.start) % width, offA = (a.start + width - b.start) % width;
    const uint32_t fromA = offB + b.len > a.len ? offB + b.len : a.len;        // starting at a.start
    const uint32_t fromB = offA + a.len > b.len ? offA + a.len : b.len;        // starting at b.start
    const Span r = fromA <= fromB ? span(a.start, fromA) : span(b.start, fromB);
    return r.len >= width ? span(0u, width) : r;
}

struct DirtyLevel { Span hx, hy, px, py; };         // heights (never wrapping) and pyramid (wrapped) of one level

// every level's dirty sets for a change of the level-0 rectangle (x0, y0, w, h), which lies inside the map
inline std::vector<DirtyLevel> dirty_levels(int maxDepth, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h) {
    std::vector<DirtyLevel> out(static_cast<size_t>(maxDepth) + 1u);
    for (int l = 0; l <= maxDepth; ++l) {
        const uint32_t width = 1u << (maxDepth - l);
        DirtyLevel& d = out[l];
        if (l == 0) { d.hx = span(x0, w); d.hy = span(y0, h); }
        else { d.hx = halve_heights(out[l - 1].hx); d.hy = halve_heights(out[l - 1].hy); }
        d.px = grow_wrapped(d.hx, width);
        d.py = grow_wrapped(d.hy, width);
        if (l > 0) {
            d.px = unite_wrapped(d.px, halve_wrapped(out[l - 1].px, 2u * width), width);
            d.py = unite_wrapped(d.py, halve_wrapped(out[l - 1].py, 2u * width), width);
        }
    }
    return out;
}

// ---------------------------------------------------------------- the refit's level table
// The nodes of a tree (tfdm_build.h build_tree) sorted by depth: `order` holds the node indices of depth 0, then of depth 1, ...;
// depth d is order[offset[d] .. offset[d + 1]).  A refit goes over the depths from the deepest to the root: a leaf takes its
// primitive's box, an inner node the union of its two children, which lie one depth further down.
constexpr int kMaxTreeLevels = 22;                  // a balanced tree over 2^20 leaves is 20 deep: 21 depths
struct LevelTable {
    std::vector<uint32_t> order;
    uint32_t offset[kMaxTreeLevels + 1];
    int numLevels = 0;
    uint32_t numLeaves = 0;
};

// false: the tree is deeper than kMaxTreeLevels or not a tree (build_tree makes neither)
inline bool make_level_table(const Node* nodes, uint32_t numNodes, LevelTable& t) {
    t.order.clear(); t.order.reserve(numNodes);
    t.numLevels = 0; t.numLeaves = 0;
    for (uint32_t& o : t.offset) o = 0u;
    if (numNodes == 0u) return false;
    t.order.push_back(0u);
    uint32_t begin = 0u;
    while (begin < t.order.size()) {
        if (t.numLevels == kMaxTreeLevels) return false;
        const uint32_t end = static_cast<uint32_t>(t.order.size());
        t.offset[t.numLevels++] = begin;
        for (uint32_t i = begin; i < end; ++i) {
            const Node& n = nodes[t.order[i]];
            if (n.count != 0u) { ++t.numLeaves; continue; }
            if (n.first >= numNodes - 1u || t.order.size() + 2u > numNodes) return false;
            t.order.push_back(n.first); t.order.push_back(n.first + 1u);
        }
        begin = end;
    }
    for (int d = t.numLevels; d <= kMaxTreeLevels; ++d) t.offset[d] = static_cast<uint32_t>(t.order.size());
    return t.order.size() == numNodes;
}

// One node of the refit, in the arithmetic of build_tree's loop (std::min / std::max as selects; the first child's value is kept
// on a tie).  `aabbs`: six floats per primitive.  A leaf whose primitive's box is empty (build_tree's test) keeps the box it has
// and the call returns false: in the one-node "nothing to hit" tree that is right, in any other tree the leaf's primitive was
// not empty when the tree was built, so the tree's shape is no longer the shape of a fresh build.
GFX_TFDM_FN bool box_is_empty(const float* b) { return !(b[0] <= b[3] && b[1] <= b[4] && b[2] <= b[5]); }
GFX_TFDM_FN float tree_min(float a, float b) { return b < a ? b : a; }
GFX_TFDM_FN float tree_max(float a, float b) { return a < b ? b : a; }
GFX_TFDM_FN bool refit_node(Node* nodes, uint32_t i, const float* aabbs) {
    Node n = nodes[i];
    if (n.count != 0u) {
        const float* b = aabbs + 6u * static_cast<size_t>(n.first);
        if (box_is_empty(b)) return false;
        for (int k = 0; k < 3; ++k) { n.lo[k] = b[k]; n.hi[k] = b[3 + k]; }
    }
    else {
        const Node a = nodes[n.first], c = nodes[n.first + 1u];
        for (int k = 0; k < 3; ++k) { n.lo[k] = tree_min(a.lo[k], c.lo[k]); n.hi[k] = tree_max(a.hi[k], c.hi[k]); }
    }
    nodes[i] = n;
    return true;
}

} // namespace tfdm
} // namespace gfx
