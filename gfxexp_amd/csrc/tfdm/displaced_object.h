// displaced_object.h -- the host layer the three displaced-surface ray queries share (tfdm.hip, nrtdsm/nrtdsm.hip,
// nrtdsm/shell.hip): the object every one of them keeps, the checks of a base mesh, of a height map and of a trace call, the
// rebuild of records, boxes and tree into fresh buffers, and size / read of what an object owns.  What is left in the three
// files is what differs: the kernels, check_params, make_records (the refusals of a query) and the order of a create.
//
// `name` is the query's prefix in the ABI ("gfx_tfdm", "gfx_nrtdsm", "gfx_shell"): every message of this layer begins with it
// and the call it belongs to, as include/gfxexp.h documents them.  (The upload of a height map launches the pyramid kernels
// and so lives beside them, in tfdm_pyramid.hip.h.)
#pragma once
#include "../internal.h"
#include "tfdm_build.h"
#include "tfdm_update.h"

namespace gfx {

struct DisplacedObject {
    const char* const name;             // "gfx_tfdm", "gfx_nrtdsm", "gfx_shell"
    const size_t recordBytes;           // of one element of `records`
    int device = 0;
    uint32_t numTriangles = 0, numNodes = 0;
    gfx_tfdm_params pub;                // as the caller gave them
    tfdm::Params params;                // derived (tfdm_build.h make_params, shell_build.h make_shell_params)
    // host mirror of the base mesh: the records are made again when the parameters (or a shell's mesh) change
    std::vector<float> positions, normals, texCoords;   // 9 / 9 / 6 floats per triangle, vertex order A B C
    DevBuf records, aabbs, nodes;       // record[numTriangles], Box[numTriangles], Node[numNodes]
    DisplacedObject(const char* n, size_t r) : name(n), recordBytes(r) {}
};

// ... displaced by a height map (TFDM, NRTDSM)
struct HeightMapObject : DisplacedObject {
    uint32_t size = 0;
    DevBuf heights, pyramid;            // all levels behind one another (tfdm::level_offset)
    bool ownMips = false;               // created with every level supplied: the coarser levels are not means of the finer ones
    const char* lastChange = nullptr;   // the call that made this generation, when it is not set_params: a stale member's message names it
    // what *_update_heights needs (tfdm_update.hip.h), allocated at the first update: an object that is never updated owns none of it
    DevBuf updateFlags, levelOrder;     // eight flag words; the tree's node indices sorted by depth (tfdm_update.h LevelTable)
    void* updateHost = nullptr;         // pinned: the flag words and the root node as they come back
    tfdm::LevelTable levelTable;        // offsets of `levelOrder`; made from the tree at the first update of a generation
    bool levelTableValid = false;       // false again whenever `nodes` becomes a new tree (create, set_params)
    uint32_t numNonEmpty = 0;           // primitives whose box is not empty, counted when the table was made
    using DisplacedObject::DisplacedObject;
};

inline void displaced_release(DisplacedObject& o) { o.records.release(); o.aabbs.release(); o.nodes.release(); }
inline void displaced_release(HeightMapObject& o) {
    o.heights.release(); o.pyramid.release(); o.updateFlags.release(); o.levelOrder.release();
    if (o.updateHost) (void)hipHostFree(o.updateHost);
    o.updateHost = nullptr;
    displaced_release(static_cast<DisplacedObject&>(o));
}

// ---- create: the base mesh.  The null check of a create names what that query takes and stays with it; check_base_mesh follows
// it, fill_mirror comes after the query's own checks (height map, parameters).
inline void check_base_mesh(const DisplacedObject& o, uint32_t stride, uint32_t numVertices, uint32_t numTriangles) {
    const std::string who = std::string(o.name) + "_create: ";
    if (stride < sizeof(gfx_vertex)) throw HipError(who + "the vertex stride is smaller than gfx_vertex");
    if (numTriangles == 0 || numVertices == 0) throw HipError(who + "the base mesh has no triangles");
    if (numTriangles > tfdm::kMaxTriangles) throw HipError(who + "more than 2^20 base triangles");
}

inline void fill_mirror(DisplacedObject& o, const void* vertices, uint32_t stride, uint32_t numVertices, const uint32_t* triangles, uint32_t numTriangles) {
    for (uint32_t t = 0; t < 3u * numTriangles; ++t)
        if (triangles[t] >= numVertices) throw HipError(std::string(o.name) + "_create: a triangle refers to a vertex that does not exist");
    o.numTriangles = numTriangles;
    o.positions.resize(9 * static_cast<size_t>(numTriangles)); o.normals.resize(9 * static_cast<size_t>(numTriangles)); o.texCoords.resize(6 * static_cast<size_t>(numTriangles));
    for (uint32_t t = 0; t < 3u * numTriangles; ++t) {
        gfx_vertex v;
        std::memcpy(&v, static_cast<const uint8_t*>(vertices) + static_cast<size_t>(stride) * triangles[t], sizeof(v));
        for (int k = 0; k < 3; ++k) { o.positions[3 * t + k] = v.position[k]; o.normals[3 * t + k] = v.normal[k]; }
        o.texCoords[2 * t] = v.texCoord[0]; o.texCoords[2 * t + 1] = v.texCoord[1];
    }
}

// ---- create: the height map.  tfdm_main.cpp:2236-2239: it must be square with a power-of-two size
inline void check_height_map(const HeightMapObject& o, const float* const* heightLevels, uint32_t numLevels, uint32_t size) {
    const std::string who = std::string(o.name) + "_create: ";
    if (size == 0 || (size & (size - 1u)) != 0u) throw HipError(who + "the height map's size must be a power of two (and the map square)");
    if (size > (1u << tfdm::kMaxDepth)) throw HipError(who + "height maps beyond 8192 x 8192 are not supported");
    if (numLevels != 1u && numLevels != static_cast<uint32_t>(tfdm::floor_log2(size)) + 1u)
        throw HipError(who + "numLevels must be 1 (the library makes the mips) or log2(size) + 1; a map that is not square has neither");
    for (uint32_t l = 0; l < numLevels; ++l) if (!heightLevels[l]) throw HipError(who + "a height level is null");
}

// ---- create, set_params, set_geometry: `recs` (numTriangles records of o.recordBytes) -> device, `launchPrim(records, aabbs)`
// makes the boxes on the device, boxes back, tree -> device; into fresh buffers, swapped in only when all of it worked, so a call
// that fails leaves the object as it was.  Returns the root of the new tree; what a query adds to the swap (TFDM's root and
// generation, a shell's fresh BVH) follows the call and cannot fail.
template <typename LaunchPrim>
tfdm::Node rebuild(DisplacedObject& o, hipStream_t stream, const void* recs, const gfx_tfdm_params& g, const tfdm::Params& p, LaunchPrim launchPrim) {
    DevBuf records, aabbs, nodes;
    try {
        records.reserve(o.recordBytes * o.numTriangles);
        aabbs.reserve(sizeof(tfdm::Box) * o.numTriangles);
        GFX_HIP(hipMemcpyAsync(records.p, recs, o.recordBytes * o.numTriangles, hipMemcpyHostToDevice, stream));
        launchPrim(records, aabbs);
        GFX_HIP(hipGetLastError());
        std::vector<float> boxes(6 * static_cast<size_t>(o.numTriangles));
        GFX_HIP(hipMemcpyAsync(boxes.data(), aabbs.p, sizeof(tfdm::Box) * o.numTriangles, hipMemcpyDeviceToHost, stream));
        GFX_HIP(hipStreamSynchronize(stream));       // also keeps `recs` alive until its copy is done
        const std::vector<tfdm::Node> tree = tfdm::build_tree(boxes.data(), o.numTriangles);
        nodes.reserve(sizeof(tfdm::Node) * tree.size());
        GFX_HIP(hipMemcpy(nodes.p, tree.data(), sizeof(tfdm::Node) * tree.size(), hipMemcpyHostToDevice));
        displaced_release(o);
        o.records = records; o.aabbs = aabbs; o.nodes = nodes;
        o.numNodes = static_cast<uint32_t>(tree.size());
        o.pub = g;
        o.params = p;
        return tree[0];
    }
    catch (...) { records.release(); aabbs.release(); nodes.release(); throw; }
}

// ---- trace: the checks every query makes of its arguments.  blocks == 0: there are no rays and nothing to launch.
struct TraceArgs { uint32_t blocks; const float4* org; const float4* dir; unsigned long long* counters; };

inline TraceArgs trace_args(const DisplacedObject& o, int mode, const void* dRayOrgTmin, const void* dRayDirTmax, uint32_t numRays, void* dOut, void* dCounters,
                            uint32_t block) {
    const std::string who = std::string(o.name) + "_trace: ";
    if (mode != GFX_TRACE_CLOSEST && mode != GFX_TRACE_ANY) throw HipError(who + "unknown mode");
    if (numRays == 0) return TraceArgs{ 0u, nullptr, nullptr, nullptr };
    if (!dRayOrgTmin || !dRayDirTmax || !dOut) throw HipError(who + "null ray or output buffer");
    // rays are read as float4 and a closest hit is written as float4s; an any-hit answer is one uint32
    const uintptr_t outMask = mode == GFX_TRACE_ANY ? 3u : 15u;
    if ((reinterpret_cast<uintptr_t>(dRayOrgTmin) & 15u) || (reinterpret_cast<uintptr_t>(dRayDirTmax) & 15u) || (reinterpret_cast<uintptr_t>(dOut) & outMask))
        throw HipError(who + "the ray buffers and a closest-hit output must be 16-byte aligned (an any-hit output 4-byte)");
    if (reinterpret_cast<uintptr_t>(dCounters) & 7u) throw HipError(who + "the counters must be 8-byte aligned");
    return TraceArgs{ (numRays + block - 1u) / block, static_cast<const float4*>(dRayOrgTmin), static_cast<const float4*>(dRayDirTmax),
                      static_cast<unsigned long long*>(dCounters) };
}

// ---- size / read.  `what`: GFX_TFDM_READ_* (a shell adds its two items on top, shell.hip); -1: every device byte of the object
inline size_t displaced_size(const DisplacedObject& o, int what) {
    switch (what) {
    case -1: return o.records.bytes + o.aabbs.bytes + o.nodes.bytes;
    case GFX_TFDM_READ_AABBS: return sizeof(tfdm::Box) * o.numTriangles;
    case GFX_TFDM_READ_RECORDS: return o.recordBytes * o.numTriangles;
    case GFX_TFDM_READ_NODES: return sizeof(tfdm::Node) * o.numNodes;
    default: throw HipError(std::string(o.name) + "_read: unknown item");
    }
}

inline size_t displaced_size(const HeightMapObject& o, int what, uint32_t level) {
    const DisplacedObject& base = o;
    switch (what) {
    case -1: return o.heights.bytes + o.pyramid.bytes + o.updateFlags.bytes + o.levelOrder.bytes + displaced_size(base, -1);
    case GFX_TFDM_READ_PYRAMID:
    case GFX_TFDM_READ_HEIGHTS: {
        if (level > static_cast<uint32_t>(o.params.maxDepth)) throw HipError(std::string(o.name) + "_read: no such level");
        const size_t w = o.size >> level;
        return w * w * (what == GFX_TFDM_READ_PYRAMID ? sizeof(tfdm::F2) : sizeof(float));
    }
    default: return displaced_size(base, what);
    }
}

inline const void* displaced_item(const DisplacedObject& o, int what) {
    return what == GFX_TFDM_READ_AABBS ? o.aabbs.p : what == GFX_TFDM_READ_RECORDS ? o.records.p : o.nodes.p;
}

// `need`: the item's size, which the caller asks for first (an unknown item or level is refused there); `src`: where it lies
inline void read_item(const DisplacedObject& o, size_t need, const void* src, void* hostOut, size_t bytes) {
    if (!hostOut || bytes != need) throw HipError(std::string(o.name) + "_read: the buffer must have exactly the item's size (" + o.name + "_size)");
    GFX_HIP(hipDeviceSynchronize());
    GFX_HIP(hipMemcpy(hostOut, src, bytes, hipMemcpyDeviceToHost));
}

inline void displaced_read(const HeightMapObject& o, int what, uint32_t level, void* hostOut, size_t bytes) {
    if (what < 0) throw HipError(std::string(o.name) + "_read: unknown item");
    const size_t need = displaced_size(o, what, level);
    const void* src = displaced_item(o, what);
    if (what == GFX_TFDM_READ_PYRAMID) src = o.pyramid.as<tfdm::F2>() + tfdm::level_offset(o.params.maxDepth, static_cast<int>(level));
    if (what == GFX_TFDM_READ_HEIGHTS) src = o.heights.as<float>() + tfdm::level_offset(o.params.maxDepth, static_cast<int>(level));
    read_item(o, need, src, hostOut, bytes);
}

} // namespace gfx
