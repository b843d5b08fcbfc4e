// shell.hip -- shell mapping on the device: the per-triangle heights and boxes and the ray query, around the arithmetic of
// shell_core.hip.h (which the host compiles too: tests/shell_host.cpp holds every result of these kernels against it bit for bit).
//
//   k_shell_prim                computeAABBs_generic<true> (nrtdsm_preprocess_kernels.cu:143-357): one base triangle per lane; the
//                               heights of the shell mesh over its footprint go into its record, the prism's box into `aabbs`
//   k_shell_trace<ANY_HIT>      the prism GAS + detailedSurface_generic<., true> (nrtdsm_intersection_kernels.h:1632-2220): one ray
//                               per lane through the binary tree over the per-triangle boxes, shell::intersect at the leaves
//
// Launch shape: that of k_nrtdsm_trace, one wave per block.  Two LDS columns per lane: the base-tree stack and the shell-BVH stack
// (12 KB each per wave); the quadtree over tiles is three 64-bit words addressed by shifts; everything else is in scalars and
// nothing is indexed at run time.  Registers, scratch and occupancy: DESIGN.md section 21.
#include <cstring>
#include "shell.h"
#include "shell_build.h"
#include "../tfdm/tfdm_lds_stack.hip.h"

namespace gfx {

using namespace tfdm;

namespace {

constexpr int kTraceBlock = 64;             // one wave per block
using LdsStack = LdsColumnStack<kTraceBlock>;

__global__ void __launch_bounds__(kTraceBlock) k_shell_prim(nrtdsm::PrismRecord* __restrict__ records, const Node* __restrict__ shellNodes,
                                                            const shell::ShellTri* __restrict__ shellTris, Params p, uint32_t numTriangles, Box* __restrict__ aabbs) {
    __shared__ uint2 s_stack[kStackDepth * kTraceBlock];
    const uint32_t i = blockIdx.x * kTraceBlock + threadIdx.x;
    if (i >= numTriangles) return;
    LdsStack stack;
    stack.col = s_stack + threadIdx.x;
    stack.sp = 0;
    shell::ShellMap map;
    map.nodes = shellNodes; map.tris = shellTris;
    nrtdsm::PrismRecord r = records[i];
    aabbs[i] = shell::prim_bounds(r, map, p, stack);
    records[i] = r;
}

template <bool ANY_HIT>
__global__ void __launch_bounds__(kTraceBlock) k_shell_trace(const Node* __restrict__ nodes, const nrtdsm::PrismRecord* __restrict__ records,
                                                             const Node* __restrict__ shellNodes, const shell::ShellTri* __restrict__ shellTris, Params p,
                                                             const float4* __restrict__ rayOrgTmin, const float4* __restrict__ rayDirTmax, uint32_t numRays,
                                                             void* __restrict__ out, unsigned long long* __restrict__ counters) {
    __shared__ uint2 s_stack[kStackDepth * kTraceBlock];
    __shared__ uint2 s_shellStack[kStackDepth * kTraceBlock];
    const uint32_t i = blockIdx.x * kTraceBlock + threadIdx.x;
    const bool live = i < numRays;
    nrtdsm::TraceStats ts;
    ts.aabbTests = 0u; ts.leafTests = 0u; ts.primTests = 0u; ts.maxIterations = 0u;
    if (live) {
        const float4 o = rayOrgTmin[i], d = rayDirTmax[i];
        LdsStack stack, shellStack;
        stack.col = s_stack + threadIdx.x;
        stack.sp = 0;
        shellStack.col = s_shellStack + threadIdx.x;
        shellStack.sp = 0;
        shell::ShellMap map;
        map.nodes = shellNodes; map.tris = shellTris;
        shell::TraceShellHit best;
        const bool hit = shell::trace_ray<ANY_HIT>(nodes, records, map, p, v3(o.x, o.y, o.z), v3(d.x, d.y, d.z), o.w, d.w, stack, shellStack, best, ts);
        if (ANY_HIT) static_cast<uint32_t*>(out)[i] = hit ? 1u : 0u;
        else {
            float4* h = static_cast<float4*>(out) + 3u * i;
            h[0] = make_float4(best.t, best.bcB, best.bcC, b2f(best.prim));
            h[1] = make_float4(best.normal.x, best.normal.y, best.normal.z, b2f(best.frontFace));
            h[2] = make_float4(b2f(best.tri), b2f(best.geom), b2f(static_cast<uint32_t>(best.tileX)), b2f(static_cast<uint32_t>(best.tileY)));
        }
    }
    if (counters) {                      // per wave
        const uint32_t a = wave_sum(ts.aabbTests), l = wave_sum(ts.leafTests), r = wave_sum(live ? 1u : 0u), t = wave_sum(ts.primTests);
        if ((threadIdx.x & 63u) == 0) { atomicAdd(counters + 0, a); atomicAdd(counters + 1, l); atomicAdd(counters + 2, r); atomicAdd(counters + 3, t); }
    }
}

void check_params(const gfx_tfdm_params& g) {
    if (const char* why = shell::refuse_params(g)) throw HipError(std::string("gfx_shell: ") + why);
}

// The records of every base triangle, or the refusal: needs no device work, so it runs before the first launch
std::vector<nrtdsm::PrismRecord> make_records(const ShellObject& o, const gfx_tfdm_params& g, const Params& p) {
    if (!std::isfinite(p.baseHeight) || !std::isfinite(p.heightScale)) throw HipError("gfx_shell: the height offset or scale derived from the parameters is not finite");
    std::vector<nrtdsm::PrismRecord> recs(o.numTriangles);
    for (uint32_t t = 0; t < o.numTriangles; ++t) {
        recs[t] = shell::make_shell_record(&o.positions[9 * t], &o.positions[9 * t + 3], &o.positions[9 * t + 6], &o.normals[9 * t], &o.normals[9 * t + 3], &o.normals[9 * t + 6],
                                           &o.texCoords[6 * t], &o.texCoords[6 * t + 2], &o.texCoords[6 * t + 4], g);
        for (float c : recs[t].tc) if (!std::isfinite(c)) throw HipError("gfx_shell: a texture coordinate (after the texture transform) is not finite");
        if (!shell::tile_coords_in_range(recs[t]))
            throw HipError("gfx_shell: a texture coordinate (after the texture transform) reaches 2^22 tiles; reduce texOffset modulo 1 or the scale");
    }
    return recs;
}

struct ShellDev { DevBuf nodes, tris; uint32_t numNodes = 0, numTris = 0, numGeoms = 0; };

// `fresh`: a new shell BVH that takes the place of the object's own together with the new records, boxes and tree (null: the
// object's own is used)
void build_geometry(ShellObject& o, hipStream_t stream, const gfx_tfdm_params& g, const std::vector<nrtdsm::PrismRecord>& recs, ShellDev* fresh) {
    const Params p = shell::make_shell_params(g);
    const DevBuf& sn = fresh ? fresh->nodes : o.shellNodes;
    const DevBuf& st = fresh ? fresh->tris : o.shellTris;
    o.root = rebuild(o, stream, recs.data(), g, p, [&](const DevBuf& records, const DevBuf& aabbs) {
        k_shell_prim<<<(o.numTriangles + 63u) / 64u, kTraceBlock, 0, stream>>>(records.as<nrtdsm::PrismRecord>(), sn.as<Node>(), st.as<shell::ShellTri>(), p, o.numTriangles, aabbs.as<Box>());
    });
    if (fresh) {
        o.shellNodes.release(); o.shellTris.release();
        o.shellNodes = fresh->nodes; o.shellTris = fresh->tris;
        o.numShellNodes = fresh->numNodes; o.numShellTriangles = fresh->numTris;
        o.numGeoms = fresh->numGeoms;
        fresh->nodes = DevBuf(); fresh->tris = DevBuf();
    }
    ++o.generation;
}

// the shell BVH of the geometries on the device, or the refusal
void upload_shell(const char* who, hipStream_t stream, const gfx_shell_geom* geoms, uint32_t numGeoms, ShellDev& dev) {
    shell::ShellBvh bvh;
    if (const char* why = shell::build_shell(geoms, numGeoms, bvh)) throw HipError(std::string(who) + ": " + why);
    dev.nodes.reserve(sizeof(Node) * bvh.nodes.size());
    dev.tris.reserve(sizeof(shell::ShellTri) * bvh.tris.size());
    GFX_HIP(hipMemcpyAsync(dev.nodes.p, bvh.nodes.data(), sizeof(Node) * bvh.nodes.size(), hipMemcpyHostToDevice, stream));
    GFX_HIP(hipMemcpyAsync(dev.tris.p, bvh.tris.data(), sizeof(shell::ShellTri) * bvh.tris.size(), hipMemcpyHostToDevice, stream));
    GFX_HIP(hipStreamSynchronize(stream));           // `bvh` goes out of scope
    dev.numNodes = static_cast<uint32_t>(bvh.nodes.size());
    dev.numTris = static_cast<uint32_t>(bvh.tris.size());
    dev.numGeoms = numGeoms;
}

} // namespace

void shell_init(ShellObject& o, hipStream_t stream, const void* vertices, uint32_t stride, uint32_t numVertices, const uint32_t* triangles, uint32_t numTriangles,
                const gfx_shell_geom* geoms, uint32_t numGeoms, const gfx_tfdm_params& g) {
    if (!vertices || !triangles) throw HipError("gfx_shell_create: null vertices or triangles");
    check_base_mesh(o, stride, numVertices, numTriangles);
    check_params(g);
    fill_mirror(o, vertices, stride, numVertices, triangles, numTriangles);
    const std::vector<nrtdsm::PrismRecord> recs = make_records(o, g, shell::make_shell_params(g));      // every refusal comes before the first launch
    ShellDev dev;
    try {
        upload_shell("gfx_shell_create", stream, geoms, numGeoms, dev);
        build_geometry(o, stream, g, recs, &dev);
    }
    catch (...) { dev.nodes.release(); dev.tris.release(); throw; }
}

void shell_set_params(ShellObject& o, hipStream_t stream, const gfx_tfdm_params& g) {
    check_params(g);
    build_geometry(o, stream, g, make_records(o, g, shell::make_shell_params(g)), nullptr);
    o.lastChange = "gfx_shell_set_params";
}

void shell_set_geometry(ShellObject& o, hipStream_t stream, const gfx_shell_geom* geoms, uint32_t numGeoms) {
    ShellDev dev;
    try {
        upload_shell("gfx_shell_set_geometry", stream, geoms, numGeoms, dev);
        build_geometry(o, stream, o.pub, make_records(o, o.pub, shell::make_shell_params(o.pub)), &dev);
        o.lastChange = "gfx_shell_set_geometry";
    }
    catch (...) { dev.nodes.release(); dev.tris.release(); throw; }
}

void shell_trace(ShellObject& o, hipStream_t stream, int mode, const void* dRayOrgTmin, const void* dRayDirTmax, uint32_t numRays, void* dOut, void* dCounters) {
    const TraceArgs a = trace_args(o, mode, dRayOrgTmin, dRayDirTmax, numRays, dOut, dCounters, kTraceBlock);
    if (a.blocks == 0) return;
    auto launch = [&](auto kernel) {
        kernel<<<a.blocks, kTraceBlock, 0, stream>>>(o.nodes.as<Node>(), o.records.as<nrtdsm::PrismRecord>(), o.shellNodes.as<Node>(), o.shellTris.as<shell::ShellTri>(), o.params,
                                                     a.org, a.dir, numRays, dOut, a.counters);
    };
    launch(mode == GFX_TRACE_ANY ? k_shell_trace<true> : k_shell_trace<false>);
    GFX_HIP(hipGetLastError());
}

} // namespace gfx
