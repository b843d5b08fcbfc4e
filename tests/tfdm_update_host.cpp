// tfdm_update_host.cpp -- the host model of gfx_tfdm_update_heights behind a C interface (tests/tfdm_update_host.py compiles it
// into a directory the test provides; tools/tfdm_update_sanitize_main.cpp includes it under the sanitizers).  It runs the regions
// of gfxexp_amd/csrc/tfdm/tfdm_update.h with the core's own arithmetic: the height mips over H_l, the pyramid over P_l, prim_aabb
// for all triangles and the refit over a given node array -- what the device kernels of tfdm_update.hip.h do, texel for texel.
#include <cstdint>
#include <cstring>
#include <vector>
#include "tfdm/tfdm_build.h"
#include "tfdm/tfdm_update.h"

using namespace gfx::tfdm;

namespace {

// heights / pyramid: all levels behind one another.  counts (optional): per level the number of height and of pyramid texels written
void region_update(float* heights, F2* pyramid, uint32_t size, const float* src, uint32_t pitch, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t* counts) {
    const int maxDepth = floor_log2(size);
    const std::vector<DirtyLevel> dirty = dirty_levels(maxDepth, x0, y0, w, h);
    for (uint32_t j = 0; j < h; ++j)
        for (uint32_t i = 0; i < w; ++i) heights[static_cast<size_t>(y0 + j) * size + x0 + i] = src[static_cast<size_t>(j) * pitch + i];
    for (int l = 1; l <= maxDepth; ++l) {
        const DirtyLevel& d = dirty[l];
        const uint32_t lw = size >> l;
        const float* s = heights + level_offset(maxDepth, l - 1);
        float* dst = heights + level_offset(maxDepth, l);
        for (uint32_t y = d.hy.start; y < d.hy.start + d.hy.len; ++y)
            for (uint32_t x = d.hx.start; x < d.hx.start + d.hx.len; ++x) {
                const float a = s[(2 * y) * 2 * lw + 2 * x], b = s[(2 * y) * 2 * lw + 2 * x + 1];
                const float c = s[(2 * y + 1) * 2 * lw + 2 * x], e = s[(2 * y + 1) * 2 * lw + 2 * x + 1];
                dst[y * lw + x] = ((a + b) + (c + e)) * 0.25f;
            }
    }
    for (int l = 0; l <= maxDepth; ++l) {
        const DirtyLevel& d = dirty[l];
        const uint32_t lw = size >> l;
        for (uint32_t j = 0; j < d.py.len; ++j)
            for (uint32_t i = 0; i < d.px.len; ++i) {
                const int x = static_cast<int>((d.px.start + i) % lw), y = static_cast<int>((d.py.start + j) % lw);
                pyramid[level_offset(maxDepth, l) + static_cast<uint32_t>(y) * lw + static_cast<uint32_t>(x)] =
                    l == 0 ? texel_min_max(heights, maxDepth, 0, x, y) : pyramid_reduce(heights, pyramid, maxDepth, l, x, y);
            }
        if (counts) { counts[2 * l] = d.hx.len * d.hy.len; counts[2 * l + 1] = d.px.len * d.py.len; }
    }
}

void full_pyramid(const float* heights, uint32_t size, F2* out) {
    const int maxDepth = floor_log2(size);
    for (int l = 0; l <= maxDepth; ++l) {
        const int w = 1 << (maxDepth - l);
        for (int y = 0; y < w; ++y)
            for (int x = 0; x < w; ++x)
                out[level_offset(maxDepth, l) + static_cast<uint32_t>(y * w + x)] = l == 0 ? texel_min_max(heights, maxDepth, 0, x, y) : pyramid_reduce(heights, out, maxDepth, l, x, y);
    }
}

struct MapState { std::vector<float> heights; std::vector<F2> pyramid; };

MapState fresh_state(const float* map, uint32_t size) {
    MapState s;
    s.heights = make_levels(&map, 1u, size);
    s.pyramid.resize(s.heights.size());
    full_pyramid(s.heights.data(), size, s.pyramid.data());
    return s;
}

} // namespace

extern "C" {

// per level: hx.start, hx.len, hy.start, hy.len, px.start, px.len, py.start, py.len
void tfdm_update_host_dirty(uint32_t size, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t* out) {
    const std::vector<DirtyLevel> d = dirty_levels(floor_log2(size), x0, y0, w, h);
    for (size_t l = 0; l < d.size(); ++l) {
        const uint32_t v[8] = { d[l].hx.start, d[l].hx.len, d[l].hy.start, d[l].hy.len, d[l].px.start, d[l].px.len, d[l].py.start, d[l].py.len };
        std::memcpy(out + 8 * l, v, sizeof(v));
    }
}

void tfdm_update_host_region(float* heights, F2* pyramid, uint32_t size, const float* src, uint32_t pitch, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t* counts) {
    region_update(heights, pyramid, size, src, pitch, x0, y0, w, h, counts);
}

// The region update of the state of `oldMap` with the rectangle of `newMap` against make_levels + the full pyramid of the map that
// results (oldMap outside the rectangle, newMap inside).  0: the same bits at every level; otherwise 1 + the first level that
// differs (+ 100 where it is the pyramid that differs).
uint32_t tfdm_update_host_check_rect(uint32_t size, const float* oldMap, const float* newMap, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h) {
    MapState s = fresh_state(oldMap, size);
    region_update(s.heights.data(), s.pyramid.data(), size, newMap + static_cast<size_t>(y0) * size + x0, size, x0, y0, w, h, nullptr);
    std::vector<float> mixed(oldMap, oldMap + static_cast<size_t>(size) * size);
    for (uint32_t j = y0; j < y0 + h; ++j)
        for (uint32_t i = x0; i < x0 + w; ++i) mixed[static_cast<size_t>(j) * size + i] = newMap[static_cast<size_t>(j) * size + i];
    const MapState want = fresh_state(mixed.data(), size);
    const int maxDepth = floor_log2(size);
    for (int l = 0; l <= maxDepth; ++l) {
        const size_t off = level_offset(maxDepth, l), n = static_cast<size_t>(size >> l) * (size >> l);
        if (std::memcmp(s.heights.data() + off, want.heights.data() + off, sizeof(float) * n)) return 1u + static_cast<uint32_t>(l);
        if (std::memcmp(s.pyramid.data() + off, want.pyramid.data() + off, sizeof(F2) * n)) return 101u + static_cast<uint32_t>(l);
    }
    return 0u;
}

// ... over every rectangle of the map.  Returns how many rectangles differ; firstBad: x0, y0, w, h, code of the first one.
uint32_t tfdm_update_host_check_all(uint32_t size, const float* oldMap, const float* newMap, uint32_t* numRects, uint32_t* firstBad) {
    uint32_t bad = 0u, n = 0u;
    for (uint32_t y0 = 0; y0 < size; ++y0)
        for (uint32_t x0 = 0; x0 < size; ++x0)
            for (uint32_t h = 1; y0 + h <= size; ++h)
                for (uint32_t w = 1; x0 + w <= size; ++w) {
                    ++n;
                    const uint32_t code = tfdm_update_host_check_rect(size, oldMap, newMap, x0, y0, w, h);
                    if (code != 0u && bad++ == 0u) { firstBad[0] = x0; firstBad[1] = y0; firstBad[2] = w; firstBad[3] = h; firstBad[4] = code; }
                }
    *numRects = n;
    return bad;
}

// The refit over `nodes` in place (six floats per box): deepest depth first.  Returns the number of leaves whose primitive's box is
// empty (they keep their box), or -1 when the nodes are not a tree the level table takes.  depths (optional): the number of depths.
int tfdm_update_host_refit(Node* nodes, uint32_t numNodes, const float* aabbs, uint32_t* depths) {
    LevelTable t;
    if (!make_level_table(nodes, numNodes, t)) return -1;
    int emptyLeaves = 0;
    for (int d = t.numLevels - 1; d >= 0; --d)
        for (uint32_t i = t.offset[d]; i < t.offset[d + 1]; ++i)
            if (!refit_node(nodes, t.order[i], aabbs)) ++emptyLeaves;
    if (depths) *depths = static_cast<uint32_t>(t.numLevels);
    return emptyLeaves;
}

// The whole update of a TFDM object's state on the host: region update, prim_aabb for all triangles, refit.  Returns what
// tfdm_update_host_refit returns.
int tfdm_update_host_update(float* heights, F2* pyramid, uint32_t size, const float* src, uint32_t pitch, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                            const TriRecord* records, uint32_t numTriangles, const Params* p, float* aabbs, Node* nodes, uint32_t numNodes) {
    region_update(heights, pyramid, size, src, pitch, x0, y0, w, h, nullptr);
    for (uint32_t t = 0; t < numTriangles; ++t) {
        const Box b = prim_aabb(records[t], pyramid, *p);
        const float f[6] = { b.lo.x, b.lo.y, b.lo.z, b.hi.x, b.hi.y, b.hi.z };
        std::memcpy(aabbs + 6 * static_cast<size_t>(t), f, sizeof(f));
    }
    return tfdm_update_host_refit(nodes, numNodes, aabbs, nullptr);
}

}
