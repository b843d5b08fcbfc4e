// tfdm.h -- host-side state of a displaced object (tfdm.hip) behind gfx_tfdm_*.
#pragma once
#include "../internal.h"
#include "tfdm_core.hip.h"

namespace gfx {

struct TfdmObject {
    int device = 0;
    uint32_t size = 0, numTriangles = 0, numNodes = 0;
    gfx_tfdm_params pub;                // as the caller gave them
    tfdm::Params params;                // derived (tfdm_build.h make_params)
    // host mirror of the base mesh: the records are made again when the parameters change
    std::vector<float> positions, normals, texCoords;   // 9 / 9 / 6 floats per triangle, vertex order A B C
    DevBuf heights, pyramid;            // all levels behind one another (tfdm::level_offset)
    DevBuf records, aabbs, nodes;       // TriRecord[numTriangles], Box[numTriangles], Node[numNodes]
    tfdm::Node root;                    // nodes[0] on the host: an instance's world box is made from it (tfdm_instance.hip.h)
    uint64_t generation = 0;            // bumped whenever records / aabbs / nodes become new buffers (create, set_params): an instance
                                        // record that holds the old pointers is stale (tfdm_set.hip)
};

void tfdm_default_params(gfx_tfdm_params* out);
void tfdm_init(TfdmObject& o, hipStream_t stream, const void* vertices, uint32_t stride, uint32_t numVertices, const uint32_t* triangles, uint32_t numTriangles,
               const float* const* heightLevels, uint32_t numLevels, uint32_t size, const gfx_tfdm_params& params);
void tfdm_set_params(TfdmObject& o, hipStream_t stream, const gfx_tfdm_params& params);
void tfdm_release(TfdmObject& o);
void tfdm_trace(TfdmObject& o, hipStream_t stream, int mode, const void* dRayOrgTmin, const void* dRayDirTmax, uint32_t numRays, void* dOut, void* dCounters);
size_t tfdm_size(const TfdmObject& o, int what, uint32_t level);
void tfdm_read(TfdmObject& o, int what, uint32_t level, void* hostOut, size_t bytes);

} // namespace gfx
