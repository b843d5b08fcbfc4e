// nrtdsm.h -- host-side state of an NRTDSM object (nrtdsm.hip) behind gfx_nrtdsm_*; release, size and read are displaced_object.h's.
#pragma once
#include "../tfdm/displaced_object.h"
#include "nrtdsm_core.hip.h"

namespace gfx {

struct NrtdsmObject : HeightMapObject {
    tfdm::Node root;                    // nodes[0] on the host and the generation of the buffers, as TfdmObject keeps them: what a
    uint64_t generation = 0;            // member of an instance set needs (tfdm/tfdm_set.hip)
    NrtdsmObject() : HeightMapObject("gfx_nrtdsm", sizeof(nrtdsm::PrismRecord)) {}
};

void nrtdsm_init(NrtdsmObject& o, hipStream_t stream, const void* vertices, uint32_t stride, uint32_t numVertices, const uint32_t* triangles, uint32_t numTriangles,
                 const float* const* heightLevels, uint32_t numLevels, uint32_t size, const gfx_tfdm_params& params);
void nrtdsm_set_params(NrtdsmObject& o, hipStream_t stream, const gfx_tfdm_params& params);
void nrtdsm_update_heights(Context& ctx, NrtdsmObject& o, hipStream_t stream, const float* dSrc, uint32_t srcPitch, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h);
void nrtdsm_trace(NrtdsmObject& o, hipStream_t stream, int mode, const void* dRayOrgTmin, const void* dRayDirTmax, uint32_t numRays, void* dOut, void* dCounters);

} // namespace gfx
