// nrtdsm.hip -- non-recursive traversal for displacement mapping on the device: the per-triangle heights and boxes and the ray
// query, around the arithmetic of nrtdsm_core.hip.h (which the host compiles too: tests/nrtdsm_host.cpp holds every result of
// these kernels against it bit for bit).  The height levels and the min-max pyramid are TFDM's, made by TFDM's kernels
// (tfdm/tfdm_pyramid.hip.h).
//
//   k_nrtdsm_prim               computeAABBs_generic<false> (nrtdsm_preprocess_kernels.cu:143-357): one triangle per lane; writes
//                               minHeight / amplitude into the triangle's record and its box
//   k_nrtdsm_trace<ANY_HIT>     the prism GAS + detailedSurface_generic (nrtdsm_intersection_kernels.h:1632-2220): one ray per lane
//                               through the binary tree over the per-triangle boxes, nrtdsm::intersect at the leaves
//
// Launch shape of k_nrtdsm_trace: that of k_tfdm_trace (tfdm.hip) for the same reason, a data-dependent
// descent whose length differs by orders of magnitude between neighbouring rays: one wave per block, the base-tree stack as one
// LDS column per lane (12 KB per wave), everything else in scalars.  The quadtree stack is three 64-bit words addressed by shifts;
// the 24 shared plane solves, the four children and the three roots are named scalars chosen by selects, so nothing is indexed at
// run time.  Registers, scratch and occupancy: DESIGN.md section 20.
#include <cstring>
#include "nrtdsm.h"
#include "nrtdsm_build.h"
#include "../tfdm/tfdm_lds_stack.hip.h"

namespace gfx {

using namespace tfdm;

namespace {

#include "../tfdm/tfdm_pyramid.hip.h"       // k_tfdm_minmax_first, k_tfdm_minmax_level
#include "../tfdm/tfdm_update.hip.h"        // k_tfdm_update_*, k_tfdm_refit_*, update_heights

constexpr int kTraceBlock = 64;             // one wave per block

__global__ void __launch_bounds__(64) k_nrtdsm_prim(nrtdsm::PrismRecord* __restrict__ records, const F2* __restrict__ pyramid, Params p, uint32_t numTriangles,
                                                    Box* __restrict__ aabbs) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= numTriangles) return;
    nrtdsm::PrismRecord r = records[i];
    aabbs[i] = nrtdsm::prim_bounds(r, pyramid, p);
    records[i] = r;
}

using LdsStack = LdsColumnStack<kTraceBlock>;

template <bool ANY_HIT>
__global__ void __launch_bounds__(kTraceBlock) k_nrtdsm_trace(const Node* __restrict__ nodes, const nrtdsm::PrismRecord* __restrict__ records,
                                                              const float* __restrict__ heights, const F2* __restrict__ pyramid, Params p,
                                                              const float4* __restrict__ rayOrgTmin, const float4* __restrict__ rayDirTmax, uint32_t numRays,
                                                              void* __restrict__ out, unsigned long long* __restrict__ counters) {
    __shared__ uint2 s_stack[kStackDepth * kTraceBlock];
    const uint32_t i = blockIdx.x * kTraceBlock + threadIdx.x;
    const bool live = i < numRays;
    nrtdsm::TraceStats ts;
    ts.aabbTests = 0u; ts.leafTests = 0u; ts.primTests = 0u; ts.maxIterations = 0u;
    if (live) {
        const float4 o = rayOrgTmin[i], d = rayDirTmax[i];
        LdsStack stack;
        stack.col = s_stack + threadIdx.x;
        stack.sp = 0;
        Map map;
        map.heights = heights; map.pyramid = pyramid;
        TraceHit best;
        const bool hit = nrtdsm::trace_ray<ANY_HIT>(nodes, records, map, p, v3(o.x, o.y, o.z), v3(d.x, d.y, d.z), o.w, d.w, stack, best, ts);
        if (ANY_HIT) static_cast<uint32_t*>(out)[i] = hit ? 1u : 0u;
        else {
            float4* h = static_cast<float4*>(out) + 2u * i;
            h[0] = make_float4(best.t, best.bcB, best.bcC, b2f(best.prim));
            h[1] = make_float4(best.normal.x, best.normal.y, best.normal.z, b2f(best.frontFace));
        }
    }
    if (counters) {                      // per wave
        const uint32_t a = wave_sum(ts.aabbTests), l = wave_sum(ts.leafTests), r = wave_sum(live ? 1u : 0u), t = wave_sum(ts.primTests);
        if ((threadIdx.x & 63u) == 0) { atomicAdd(counters + 0, a); atomicAdd(counters + 1, l); atomicAdd(counters + 2, r); atomicAdd(counters + 3, t); }
    }
}

void check_params(const gfx_tfdm_params& g) {
    if (const char* why = nrtdsm::refuse_params(g)) throw HipError(std::string("gfx_nrtdsm: ") + why);
}

// The records of every base triangle, or the refusal: needs no device work, so it runs before the first launch
std::vector<nrtdsm::PrismRecord> make_records(const NrtdsmObject& o, const gfx_tfdm_params& g, const Params& p) {
    if (!std::isfinite(p.baseHeight) || !std::isfinite(p.heightScale)) throw HipError("gfx_nrtdsm: the height offset or scale derived from the parameters is not finite");
    std::vector<nrtdsm::PrismRecord> recs(o.numTriangles);
    for (uint32_t t = 0; t < o.numTriangles; ++t) {
        recs[t] = nrtdsm::make_record(&o.positions[9 * t], &o.positions[9 * t + 3], &o.positions[9 * t + 6], &o.normals[9 * t], &o.normals[9 * t + 3], &o.normals[9 * t + 6],
                                      &o.texCoords[6 * t], &o.texCoords[6 * t + 2], &o.texCoords[6 * t + 4], g, p.maxDepth);
        for (float c : recs[t].tc) if (!std::isfinite(c)) throw HipError("gfx_nrtdsm: a texture coordinate (after the texture transform) is not finite");
        if (!nrtdsm::texel_coords_in_range(recs[t], o.size))
            throw HipError("gfx_nrtdsm: a texture coordinate (after the texture transform) times the map's size reaches 2^24; reduce texOffset modulo 1 or the scale");
    }
    return recs;
}

void build_geometry(NrtdsmObject& o, hipStream_t stream, const gfx_tfdm_params& g, const std::vector<nrtdsm::PrismRecord>& recs) {
    const Params p = make_params(g, o.size);
    o.root = rebuild(o, stream, recs.data(), g, p, [&](const DevBuf& records, const DevBuf& aabbs) {
        k_nrtdsm_prim<<<(o.numTriangles + 63u) / 64u, 64, 0, stream>>>(records.as<nrtdsm::PrismRecord>(), o.pyramid.as<F2>(), p, o.numTriangles, aabbs.as<Box>());
    });
    ++o.generation;
    o.levelTableValid = false;
    o.lastChange = nullptr;
}

} // namespace

void nrtdsm_init(NrtdsmObject& o, hipStream_t stream, const void* vertices, uint32_t stride, uint32_t numVertices, const uint32_t* triangles, uint32_t numTriangles,
                 const float* const* heightLevels, uint32_t numLevels, uint32_t size, const gfx_tfdm_params& g) {
    if (!vertices || !triangles || !heightLevels) throw HipError("gfx_nrtdsm_create: null vertices, triangles or height levels");
    check_base_mesh(o, stride, numVertices, numTriangles);
    check_height_map(o, heightLevels, numLevels, size);
    check_params(g);
    fill_mirror(o, vertices, stride, numVertices, triangles, numTriangles);
    const std::vector<float> levels = make_levels(heightLevels, numLevels, size);
    if (!nrtdsm::heights_in_unit_range(levels))
        throw HipError("gfx_nrtdsm_create: a height map value lies outside [0, 1] (the descent clips the map value to that range)");
    o.size = size;
    o.ownMips = numLevels > 1u;
    const std::vector<nrtdsm::PrismRecord> recs = make_records(o, g, make_params(g, size));      // every refusal comes before the first launch
    upload_height_map(o, stream, levels);
    build_geometry(o, stream, g, recs);
}

void nrtdsm_set_params(NrtdsmObject& o, hipStream_t stream, const gfx_tfdm_params& g) {
    check_params(g);
    build_geometry(o, stream, g, make_records(o, g, make_params(g, o.size)));
}

// The map changed in place (tfdm/tfdm_update.hip.h).  k_nrtdsm_prim runs again on the records it wrote before: minHeight and
// amplitude are outputs it never reads, and the one input it writes, numRoots = 0, it writes only where the two are not finite.
// With map values in [0, 1] that is decided by the record (no texel under the footprint) unless baseHeight + heightScale h can
// overflow; for such parameters the box of a primitive is empty or not by the heights, and the records and the tree are made
// again from the host's records instead, as set_params makes them.
void nrtdsm_update_heights(Context& ctx, NrtdsmObject& o, hipStream_t stream, const float* dSrc, uint32_t srcPitch, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h) {
    const bool byRecordAlone = std::fabs(static_cast<double>(o.params.baseHeight)) + std::fabs(static_cast<double>(o.params.heightScale)) < 1.0e38;
    const bool refitted = update_heights(ctx, o, stream, dSrc, srcPitch, x0, y0, w, h, true, byRecordAlone, [&]() {
        k_nrtdsm_prim<<<(o.numTriangles + 63u) / 64u, 64, 0, stream>>>(o.records.as<nrtdsm::PrismRecord>(), o.pyramid.as<F2>(), o.params, o.numTriangles, o.aabbs.as<Box>());
    }, o.root);
    if (refitted) ++o.generation;
    else build_geometry(o, stream, o.pub, make_records(o, o.pub, make_params(o.pub, o.size)));
    o.lastChange = "gfx_nrtdsm_update_heights";
}

void nrtdsm_trace(NrtdsmObject& o, hipStream_t stream, int mode, const void* dRayOrgTmin, const void* dRayDirTmax, uint32_t numRays, void* dOut, void* dCounters) {
    const TraceArgs a = trace_args(o, mode, dRayOrgTmin, dRayDirTmax, numRays, dOut, dCounters, kTraceBlock);
    if (a.blocks == 0) return;
    auto launch = [&](auto kernel) {
        kernel<<<a.blocks, kTraceBlock, 0, stream>>>(o.nodes.as<Node>(), o.records.as<nrtdsm::PrismRecord>(), o.heights.as<float>(), o.pyramid.as<F2>(), o.params, a.org, a.dir,
                                                     numRays, dOut, a.counters);
    };
    launch(mode == GFX_TRACE_ANY ? k_nrtdsm_trace<true> : k_nrtdsm_trace<false>);
    GFX_HIP(hipGetLastError());
}

} // namespace gfx
