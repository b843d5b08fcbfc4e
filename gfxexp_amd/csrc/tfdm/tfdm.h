// tfdm.h -- host-side state of a displaced object (tfdm.hip) behind gfx_tfdm_*; release, size and read are displaced_object.h's.
#pragma once
#include "displaced_object.h"

namespace gfx {

struct TfdmObject : HeightMapObject {
    tfdm::Node root;                    // nodes[0] on the host: an instance's world box is made from it (tfdm_instance.hip.h)
    uint64_t generation = 0;            // bumped whenever records / aabbs / nodes become new buffers (create, set_params) or new contents
                                        // (update_heights): an instance record that holds the old pointers or the old box is stale (tfdm_set.hip)
    TfdmObject() : HeightMapObject("gfx_tfdm", sizeof(tfdm::TriRecord)) {}
};

void tfdm_default_params(gfx_tfdm_params* out);
void tfdm_init(TfdmObject& o, hipStream_t stream, const void* vertices, uint32_t stride, uint32_t numVertices, const uint32_t* triangles, uint32_t numTriangles,
               const float* const* heightLevels, uint32_t numLevels, uint32_t size, const gfx_tfdm_params& params);
void tfdm_set_params(TfdmObject& o, hipStream_t stream, const gfx_tfdm_params& params);
void tfdm_update_heights(Context& ctx, TfdmObject& o, hipStream_t stream, const float* dSrc, uint32_t srcPitch, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h);
void tfdm_trace(TfdmObject& o, hipStream_t stream, int mode, const void* dRayOrgTmin, const void* dRayDirTmax, uint32_t numRays, void* dOut, void* dCounters);

} // namespace gfx
