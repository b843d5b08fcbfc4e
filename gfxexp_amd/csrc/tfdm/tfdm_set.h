// tfdm_set.h -- host-side state of a set of displaced instances and the scene-level ray query (tfdm_set.hip) behind
// gfx_tfdm_set_* and gfx_trace_scene.
#pragma once
#include "tfdm.h"
#include "tfdm_instance.hip.h"

namespace gfx {

struct TfdmSet {
    int device = 0;
    struct Member {
        TfdmObject* obj;            // not owned: objects outlive the set
        float objToWorld[12];
        uint32_t userId;
        uint64_t generation;        // the object's generation the committed record was made from
    };
    std::vector<Member> members;
    bool dirty = false;             // an add or a transform since the last commit
    std::vector<tfdm::InstanceRecord> host;   // the committed table
    DevBuf table;                   // InstanceRecord[members]
    DevBuf plain;                   // gfx_hit[numRays] of the plain phase of a closest-hit query; grows on demand
};

uint32_t tfdm_set_add(TfdmSet& s, TfdmObject* obj, const float objToWorld[12], uint32_t userId);
void tfdm_set_transform(TfdmSet& s, uint32_t index, const float objToWorld[12]);
void tfdm_set_commit(TfdmSet& s, hipStream_t stream);
void tfdm_set_read(TfdmSet& s, void* hostOut, size_t bytes);
void tfdm_set_release(TfdmSet& s);
// set == nullptr: no displaced instances; accel == nullptr: no plain geometry.  `fallbackPlain`: the plain-phase buffer of a
// closest-hit query without a set (the context's).
void trace_scene(Context& ctx, hipStream_t stream, const DevAccel* accel, TfdmSet* set, DevBuf& fallbackPlain, int mode, const void* dRayOrgTmin,
                 const void* dRayDirTmax, uint32_t numRays, void* dOut, void* dCounters);

} // namespace gfx
