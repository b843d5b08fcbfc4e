// tfdm.hip -- tessellation-free displacement mapping on the device: the min-max pyramid, the per-triangle boxes and the ray
// query, around the arithmetic of tfdm_core.hip.h (which the host compiles too: tests/tfdm_host.cpp holds every result of
// these kernels against it bit for bit).
//
//   k_tfdm_minmax_first / k_tfdm_minmax_level   generateFirstMinMaxMipMap / generateMinMaxMipMap (tfdm_preprocess_kernels.cu:46-131),
//                                               launched level after level as tfdm_main.cpp:2492-2545 does
//   k_tfdm_prim_aabbs                           computeAABBs (:159-363)
//   k_tfdm_trace<ANY_HIT, BILINEAR>             the custom-primitive GAS + intersection program (tfdm_intersection_kernels.h): one
//                                               ray per lane through a binary tree over the per-triangle boxes, tfdm::intersect at
//                                               the leaves.  BILINEAR: the instantiation for an object of GFX_TFDM_BILINEAR; the
//                                               Newton loop is kept out of the other one, whose registers Box and TwoTriangle
//                                               users pay for
//
// Launch shape of k_tfdm_trace (cdna_hip_programming guidelines 5-7).  A lane's work is a data-dependent descent whose length
// differs by orders of magnitude between neighbouring rays, so the unit that retires together is chosen as small as the hardware
// allows: one wave per block, and a wave that is done frees its slot at once (GFX_TFDM_TRACE_BLOCK is the
// switch to time it against larger blocks).  The texel walk keeps no stack; the per-lane state
// that must be addressed dynamically is the base-tree stack alone, kept as one LDS column per lane ([depth][lane]: conflict-free,
// like bvh8.hip.h's LaneStack): 24 entries x 8 B x 64 lanes = 12 KB per wave.  Everything else is scalars the compiler keeps in
// registers: the record is read from memory where it is used instead of being copied into a per-lane array, and the core
// indexes no local array with a run-time index.  Register count, scratch and occupancy: DESIGN.md section 14.
#include <cstring>
#include "tfdm.h"
#include "tfdm_build.h"
#include "tfdm_lds_stack.hip.h"

namespace gfx {

using namespace tfdm;

namespace {

#ifndef GFX_TFDM_TRACE_BLOCK
#define GFX_TFDM_TRACE_BLOCK 64        // lanes per block of k_tfdm_trace, a multiple of 64
#endif
constexpr int kTraceBlock = GFX_TFDM_TRACE_BLOCK;

#include "tfdm_pyramid.hip.h"       // k_tfdm_minmax_first, k_tfdm_minmax_level
#include "tfdm_update.hip.h"        // k_tfdm_update_*, k_tfdm_refit_*, update_heights

__global__ void __launch_bounds__(64) k_tfdm_prim_aabbs(const TriRecord* __restrict__ records, const F2* __restrict__ pyramid, Params p, uint32_t numTriangles,
                                                        Box* __restrict__ aabbs) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= numTriangles) return;
    aabbs[i] = prim_aabb(records[i], pyramid, p);
}

using LdsStack = LdsColumnStack<kTraceBlock>;      // tfdm_lds_stack.hip.h

template <bool ANY_HIT, bool BILINEAR>
__global__ void __launch_bounds__(kTraceBlock) k_tfdm_trace(const Node* __restrict__ nodes, const TriRecord* __restrict__ records, const float* __restrict__ heights,
                                                            const F2* __restrict__ pyramid, Params p, const float4* __restrict__ rayOrgTmin,
                                                            const float4* __restrict__ rayDirTmax, uint32_t numRays, void* __restrict__ out,
                                                            unsigned long long* __restrict__ counters) {
    __shared__ uint2 s_stack[kStackDepth * kTraceBlock];
    const uint32_t i = blockIdx.x * kTraceBlock + threadIdx.x;
    const bool live = i < numRays;
    TraceStats ts;
    ts.aabbTests = 0u; ts.leafTests = 0u; ts.primTests = 0u;
    if (live) {
        const float4 o = rayOrgTmin[i], d = rayDirTmax[i];
        LdsStack stack;
        stack.col = s_stack + threadIdx.x;
        stack.sp = 0;
        Map map;
        map.heights = heights; map.pyramid = pyramid;
        TraceHit best;
        const bool hit = trace_ray_local<ANY_HIT, BILINEAR>(nodes, records, map, p, v3(o.x, o.y, o.z), v3(d.x, d.y, d.z), o.w, d.w, stack, best, ts);
        if (ANY_HIT) static_cast<uint32_t*>(out)[i] = hit ? 1u : 0u;
        else {
            float4* h = static_cast<float4*>(out) + 2u * i;
            h[0] = make_float4(best.t, best.bcB, best.bcC, b2f(best.prim));
            h[1] = make_float4(best.normal.x, best.normal.y, best.normal.z, b2f(best.frontFace));
        }
    }
    if (counters) {                      // per wave: every lane of a wave reaches this, whatever the block size
        const uint32_t a = wave_sum(ts.aabbTests), l = wave_sum(ts.leafTests), r = wave_sum(live ? 1u : 0u), t = wave_sum(ts.primTests);
        if ((threadIdx.x & 63u) == 0) { atomicAdd(counters + 0, a); atomicAdd(counters + 1, l); atomicAdd(counters + 2, r); atomicAdd(counters + 3, t); }
    }
}

void check_params(const gfx_tfdm_params& g, uint32_t size) {
    const int maxDepth = floor_log2(size);
    if (g.localIntersection != kBox && g.localIntersection != kTwoTriangle && g.localIntersection != kBilinear)
        throw HipError("gfx_tfdm: localIntersection must be GFX_TFDM_BOX, GFX_TFDM_TWO_TRIANGLE or GFX_TFDM_BILINEAR (the reference's BSpline is not built)");
    if (g.targetMipLevel > static_cast<uint32_t>(maxDepth)) throw HipError("gfx_tfdm: targetMipLevel lies beyond the pyramid (log2(size) is its last level)");
    const float fields[] = { g.hOffset, g.hScale, g.hBias, g.texScale[0], g.texScale[1], g.texRotation, g.texOffset[0], g.texOffset[1] };
    for (float f : fields) if (!std::isfinite(f)) throw HipError("gfx_tfdm: a parameter is not finite");
    if (!(g.texScale[0] > 0.0f) || !(g.texScale[1] > 0.0f)) throw HipError("gfx_tfdm: texScale must be positive");
}

// The records of every base triangle, or the refusal
std::vector<TriRecord> make_records(const TfdmObject& o, const gfx_tfdm_params& g, const Params& p) {
    std::vector<TriRecord> recs(o.numTriangles);
    for (uint32_t t = 0; t < o.numTriangles; ++t)
        recs[t] = make_record(&o.positions[9 * t], &o.positions[9 * t + 3], &o.positions[9 * t + 6], &o.normals[9 * t], &o.normals[9 * t + 3], &o.normals[9 * t + 6],
                              &o.texCoords[6 * t], &o.texCoords[6 * t + 2], &o.texCoords[6 * t + 4], g, p.maxDepth);
    // Texel indices are int32 and become float for the texel centres: beyond 2^24 texels from the origin the centres are inexact
    // (texels would be missed) and beyond 2^31 the walk's down() overflows and need not end.  Refused here, before anything runs.
    for (const TriRecord& r : recs)
        for (float c : r.tc)
            if (std::isfinite(c) && fabsf(c) * static_cast<float>(o.size) >= kMaxTexelCoord)
                throw HipError("gfx_tfdm: a texture coordinate (after the texture transform) times the map's size reaches 2^24; reduce texOffset modulo 1 or the scale");
    return recs;
}

void build_geometry(TfdmObject& o, hipStream_t stream, const gfx_tfdm_params& g) {
    const Params p = make_params(g, o.size);
    const std::vector<TriRecord> recs = make_records(o, g, p);
    o.root = rebuild(o, stream, recs.data(), g, p, [&](const DevBuf& records, const DevBuf& aabbs) {
        k_tfdm_prim_aabbs<<<(o.numTriangles + 63u) / 64u, 64, 0, stream>>>(records.as<TriRecord>(), o.pyramid.as<F2>(), p, o.numTriangles, aabbs.as<Box>());
    });
    ++o.generation;
    o.levelTableValid = false;
    o.lastChange = nullptr;
}

} // namespace

void tfdm_default_params(gfx_tfdm_params* out) {
    std::memset(out, 0, sizeof(*out));
    out->hScale = 1.0f;
    out->texScale[0] = out->texScale[1] = 1.0f;
    out->localIntersection = kTwoTriangle;
}

void tfdm_init(TfdmObject& o, hipStream_t stream, const void* vertices, uint32_t stride, uint32_t numVertices, const uint32_t* triangles, uint32_t numTriangles,
               const float* const* heightLevels, uint32_t numLevels, uint32_t size, const gfx_tfdm_params& g) {
    if (!vertices || !triangles || !heightLevels) throw HipError("gfx_tfdm_create: null vertices, triangles or height levels");
    check_base_mesh(o, stride, numVertices, numTriangles);
    check_height_map(o, heightLevels, numLevels, size);
    check_params(g, size);
    fill_mirror(o, vertices, stride, numVertices, triangles, numTriangles);
    o.size = size;
    o.ownMips = numLevels > 1u;
    upload_height_map(o, stream, make_levels(heightLevels, numLevels, size));
    build_geometry(o, stream, g);
}

void tfdm_set_params(TfdmObject& o, hipStream_t stream, const gfx_tfdm_params& g) {
    check_params(g, o.size);
    build_geometry(o, stream, g);
}

// The map changed in place: heights and pyramid over the dirty regions, every box again, the tree refitted (tfdm_update.hip.h).
// prim_aabb leaves a box empty by the record alone (no roots, or a footprint no texel centre test lets in) unless the map holds
// NaNs, so the tree's shape stays a fresh build's; where update_heights finds that it did not, the tree is made again.
void tfdm_update_heights(Context& ctx, TfdmObject& o, hipStream_t stream, const float* dSrc, uint32_t srcPitch, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h) {
    const bool refitted = update_heights(ctx, o, stream, dSrc, srcPitch, x0, y0, w, h, false, true, [&]() {
        k_tfdm_prim_aabbs<<<(o.numTriangles + 63u) / 64u, 64, 0, stream>>>(o.records.as<TriRecord>(), o.pyramid.as<F2>(), o.params, o.numTriangles, o.aabbs.as<Box>());
    }, o.root);
    if (refitted) ++o.generation;
    else build_geometry(o, stream, o.pub);
    o.lastChange = "gfx_tfdm_update_heights";
}

void tfdm_trace(TfdmObject& o, hipStream_t stream, int mode, const void* dRayOrgTmin, const void* dRayDirTmax, uint32_t numRays, void* dOut, void* dCounters) {
    const TraceArgs a = trace_args(o, mode, dRayOrgTmin, dRayDirTmax, numRays, dOut, dCounters, kTraceBlock);
    if (a.blocks == 0) return;
    auto launch = [&](auto kernel) {
        kernel<<<a.blocks, kTraceBlock, 0, stream>>>(o.nodes.as<Node>(), o.records.as<TriRecord>(), o.heights.as<float>(), o.pyramid.as<F2>(), o.params, a.org, a.dir, numRays, dOut,
                                                     a.counters);
    };
    const bool any = mode == GFX_TRACE_ANY;
    // (named in this order so that the instantiations without the Newton loop keep their place at the front of the code object)
    if (o.params.local != kBilinear) launch(any ? k_tfdm_trace<true, false> : k_tfdm_trace<false, false>);
    else launch(any ? k_tfdm_trace<true, true> : k_tfdm_trace<false, true>);
    GFX_HIP(hipGetLastError());
}

} // namespace gfx
