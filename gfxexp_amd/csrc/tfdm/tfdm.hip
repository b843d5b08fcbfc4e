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

// records -> device, boxes on the device, boxes back, tree -> device; into fresh buffers, swapped in only when all of it worked
void build_geometry(TfdmObject& o, hipStream_t stream, const gfx_tfdm_params& g) {
    const Params p = make_params(g, o.size);
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
    DevBuf records, aabbs, nodes;
    try {
        records.reserve(sizeof(TriRecord) * o.numTriangles);
        aabbs.reserve(sizeof(Box) * o.numTriangles);
        GFX_HIP(hipMemcpyAsync(records.p, recs.data(), sizeof(TriRecord) * o.numTriangles, hipMemcpyHostToDevice, stream));
        k_tfdm_prim_aabbs<<<(o.numTriangles + 63u) / 64u, 64, 0, stream>>>(records.as<TriRecord>(), o.pyramid.as<F2>(), p, o.numTriangles, aabbs.as<Box>());
        GFX_HIP(hipGetLastError());
        std::vector<float> boxes(6 * static_cast<size_t>(o.numTriangles));
        GFX_HIP(hipMemcpyAsync(boxes.data(), aabbs.p, sizeof(Box) * o.numTriangles, hipMemcpyDeviceToHost, stream));
        GFX_HIP(hipStreamSynchronize(stream));       // also keeps `recs` alive until its copy is done
        const std::vector<Node> tree = build_tree(boxes.data(), o.numTriangles);
        nodes.reserve(sizeof(Node) * tree.size());
        GFX_HIP(hipMemcpy(nodes.p, tree.data(), sizeof(Node) * tree.size(), hipMemcpyHostToDevice));
        o.records.release(); o.aabbs.release(); o.nodes.release();
        o.records = records; o.aabbs = aabbs; o.nodes = nodes;
        o.numNodes = static_cast<uint32_t>(tree.size());
        o.root = tree[0];
        ++o.generation;
        o.pub = g;
        o.params = p;
    }
    catch (...) { records.release(); aabbs.release(); nodes.release(); throw; }
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
    if (stride < sizeof(gfx_vertex)) throw HipError("gfx_tfdm_create: the vertex stride is smaller than gfx_vertex");
    if (numTriangles == 0 || numVertices == 0) throw HipError("gfx_tfdm_create: the base mesh has no triangles");
    if (numTriangles > kMaxTriangles) throw HipError("gfx_tfdm_create: more than 2^20 base triangles");
    // tfdm_main.cpp:2236-2239: the height map must be square with a power-of-two size
    if (size == 0 || (size & (size - 1u)) != 0u) throw HipError("gfx_tfdm_create: the height map's size must be a power of two (and the map square)");
    if (size > (1u << kMaxDepth)) throw HipError("gfx_tfdm_create: height maps beyond 8192 x 8192 are not supported");
    const int maxDepth = floor_log2(size);
    if (numLevels != 1u && numLevels != static_cast<uint32_t>(maxDepth) + 1u)
        throw HipError("gfx_tfdm_create: numLevels must be 1 (the library makes the mips) or log2(size) + 1; a map that is not square has neither");
    for (uint32_t l = 0; l < numLevels; ++l) if (!heightLevels[l]) throw HipError("gfx_tfdm_create: a height level is null");
    check_params(g, size);
    for (uint32_t t = 0; t < 3u * numTriangles; ++t) if (triangles[t] >= numVertices) throw HipError("gfx_tfdm_create: a triangle refers to a vertex that does not exist");

    o.size = size; o.numTriangles = numTriangles;
    o.positions.resize(9 * static_cast<size_t>(numTriangles)); o.normals.resize(9 * static_cast<size_t>(numTriangles)); o.texCoords.resize(6 * static_cast<size_t>(numTriangles));
    for (uint32_t t = 0; t < 3u * numTriangles; ++t) {
        gfx_vertex v;
        std::memcpy(&v, static_cast<const uint8_t*>(vertices) + static_cast<size_t>(stride) * triangles[t], sizeof(v));
        for (int k = 0; k < 3; ++k) { o.positions[3 * t + k] = v.position[k]; o.normals[3 * t + k] = v.normal[k]; }
        o.texCoords[2 * t] = v.texCoord[0]; o.texCoords[2 * t + 1] = v.texCoord[1];
    }
    const std::vector<float> levels = make_levels(heightLevels, numLevels, size);
    o.heights.reserve(sizeof(float) * levels.size());
    o.pyramid.reserve(sizeof(F2) * levels.size());
    GFX_HIP(hipMemcpyAsync(o.heights.p, levels.data(), sizeof(float) * levels.size(), hipMemcpyHostToDevice, stream));
    const uint32_t b0 = (size + 15u) / 16u;
    k_tfdm_minmax_first<<<dim3(b0, b0), 256, 0, stream>>>(o.heights.as<float>(), o.pyramid.as<F2>(), maxDepth);
    GFX_HIP(hipGetLastError());
    for (int l = 1; l <= maxDepth; ++l) {
        const uint32_t b = ((size >> l) + 15u) / 16u;
        k_tfdm_minmax_level<<<dim3(b, b), 256, 0, stream>>>(o.heights.as<float>(), o.pyramid.as<F2>(), maxDepth, l);
        GFX_HIP(hipGetLastError());
    }
    GFX_HIP(hipStreamSynchronize(stream));           // `levels` goes out of scope
    build_geometry(o, stream, g);
}

void tfdm_set_params(TfdmObject& o, hipStream_t stream, const gfx_tfdm_params& g) {
    check_params(g, o.size);
    build_geometry(o, stream, g);
}

void tfdm_release(TfdmObject& o) {
    o.heights.release(); o.pyramid.release(); o.records.release(); o.aabbs.release(); o.nodes.release();
}

void tfdm_trace(TfdmObject& o, hipStream_t stream, int mode, const void* dRayOrgTmin, const void* dRayDirTmax, uint32_t numRays, void* dOut, void* dCounters) {
    if (mode != GFX_TRACE_CLOSEST && mode != GFX_TRACE_ANY) throw HipError("gfx_tfdm_trace: unknown mode");
    if (numRays == 0) return;
    if (!dRayOrgTmin || !dRayDirTmax || !dOut) throw HipError("gfx_tfdm_trace: null ray or output buffer");
    // rays are read as float4 and a closest hit is written as two float4; an any-hit answer is one uint32
    const uintptr_t outMask = mode == GFX_TRACE_ANY ? 3u : 15u;
    if ((reinterpret_cast<uintptr_t>(dRayOrgTmin) & 15u) || (reinterpret_cast<uintptr_t>(dRayDirTmax) & 15u) || (reinterpret_cast<uintptr_t>(dOut) & outMask))
        throw HipError("gfx_tfdm_trace: the ray buffers and a closest-hit output must be 16-byte aligned (an any-hit output 4-byte)");
    if (reinterpret_cast<uintptr_t>(dCounters) & 7u) throw HipError("gfx_tfdm_trace: the counters must be 8-byte aligned");
    const uint32_t blocks = (numRays + kTraceBlock - 1u) / kTraceBlock;
    const float4* org = static_cast<const float4*>(dRayOrgTmin);
    const float4* dir = static_cast<const float4*>(dRayDirTmax);
    unsigned long long* cnt = static_cast<unsigned long long*>(dCounters);
    auto launch = [&](auto kernel) {
        kernel<<<blocks, kTraceBlock, 0, stream>>>(o.nodes.as<Node>(), o.records.as<TriRecord>(), o.heights.as<float>(), o.pyramid.as<F2>(), o.params, org, dir, numRays, dOut, cnt);
    };
    const bool any = mode == GFX_TRACE_ANY;
    // (named in this order so that the instantiations without the Newton loop keep their place at the front of the code object)
    if (o.params.local != kBilinear) launch(any ? k_tfdm_trace<true, false> : k_tfdm_trace<false, false>);
    else launch(any ? k_tfdm_trace<true, true> : k_tfdm_trace<false, true>);
    GFX_HIP(hipGetLastError());
}

size_t tfdm_size(const TfdmObject& o, int what, uint32_t level) {
    const int maxDepth = o.params.maxDepth;
    switch (what) {
    case -1: return o.heights.bytes + o.pyramid.bytes + o.records.bytes + o.aabbs.bytes + o.nodes.bytes;
    case GFX_TFDM_READ_PYRAMID:
    case GFX_TFDM_READ_HEIGHTS: {
        if (level > static_cast<uint32_t>(maxDepth)) throw HipError("gfx_tfdm_read: no such level");
        const size_t w = o.size >> level;
        return w * w * (what == GFX_TFDM_READ_PYRAMID ? sizeof(F2) : sizeof(float));
    }
    case GFX_TFDM_READ_AABBS: return sizeof(Box) * o.numTriangles;
    case GFX_TFDM_READ_RECORDS: return sizeof(TriRecord) * o.numTriangles;
    case GFX_TFDM_READ_NODES: return sizeof(Node) * o.numNodes;
    default: throw HipError("gfx_tfdm_read: unknown item");
    }
}

void tfdm_read(TfdmObject& o, int what, uint32_t level, void* hostOut, size_t bytes) {
    if (what < 0) throw HipError("gfx_tfdm_read: unknown item");
    const size_t need = tfdm_size(o, what, level);
    if (!hostOut || bytes != need) throw HipError("gfx_tfdm_read: the buffer must have exactly the item's size (gfx_tfdm_size)");
    const void* src = nullptr;
    switch (what) {
    case GFX_TFDM_READ_PYRAMID: src = o.pyramid.as<F2>() + level_offset(o.params.maxDepth, static_cast<int>(level)); break;
    case GFX_TFDM_READ_HEIGHTS: src = o.heights.as<float>() + level_offset(o.params.maxDepth, static_cast<int>(level)); break;
    case GFX_TFDM_READ_AABBS: src = o.aabbs.p; break;
    case GFX_TFDM_READ_RECORDS: src = o.records.p; break;
    default: src = o.nodes.p; break;
    }
    GFX_HIP(hipDeviceSynchronize());
    GFX_HIP(hipMemcpy(hostOut, src, bytes, hipMemcpyDeviceToHost));
}

} // namespace gfx
