// nrtdsm.h -- host-side state of an NRTDSM object (nrtdsm.hip) behind gfx_nrtdsm_*.
#pragma once
#include "../internal.h"
#include "nrtdsm_core.hip.h"

namespace gfx {

struct NrtdsmObject {
    int device = 0;
    uint32_t size = 0, numTriangles = 0, numNodes = 0;
    gfx_tfdm_params pub;                // as the caller gave them
    tfdm::Params params;                // derived (tfdm_build.h make_params)
    // host mirror of the base mesh: the records are made again when the parameters change
    std::vector<float> positions, normals, texCoords;   // 9 / 9 / 6 floats per triangle, vertex order A B C
    DevBuf heights, pyramid;            // all levels behind one another (tfdm::level_offset)
    DevBuf records, aabbs, nodes;       // PrismRecord[numTriangles], Box[numTriangles], Node[numNodes]
};

void nrtdsm_init(NrtdsmObject& o, hipStream_t stream, const void* vertices, uint32_t stride, uint32_t numVertices, const uint32_t* triangles, uint32_t numTriangles,
                 const float* const* heightLevels, uint32_t numLevels, uint32_t size, const gfx_tfdm_params& params);
void nrtdsm_set_params(NrtdsmObject& o, hipStream_t stream, const gfx_tfdm_params& params);
void nrtdsm_release(NrtdsmObject& o);
void nrtdsm_trace(NrtdsmObject& o, hipStream_t stream, int mode, const void* dRayOrgTmin, const void* dRayDirTmax, uint32_t numRays, void* dOut, void* dCounters);
size_t nrtdsm_size(const NrtdsmObject& o, int what, uint32_t level);
void nrtdsm_read(NrtdsmObject& o, int what, uint32_t level, void* hostOut, size_t bytes);

} // namespace gfx
