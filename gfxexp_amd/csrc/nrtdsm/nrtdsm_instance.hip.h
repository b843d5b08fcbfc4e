// nrtdsm_instance.hip.h -- NRTDSM objects as instances of a scene, beside TFDM ones: the arithmetic shared by
// k_scene_instances_mixed (tfdm/tfdm_set.hip), the host side of the instance set and the tests (tests/scene_nrtdsm_host.cpp).
// tfdm/tfdm_instance.hip.h has the record, the ray transform, the normal matrix, the world box and the merge rule; this header adds
// the kind of a record and the step of the merge rule that runs nrtdsm::trace_ray.
//
// The kind of an instance is the word of InstanceRecord that tfdm_instance.hip.h calls pad0: 0 (what make_instance leaves there)
// is a TFDM member, 1 an NRTDSM member.  The four pointers and the Params mean the same for both; only `records` differs, which
// is nrtdsm::PrismRecord[] behind a record of kind 1.
//
// The merge rule across kinds is the rule of tfdm_instance.hip.h unchanged: nrtdsm::trace_ray accepts only t < tmax as
// tfdm::trace_ray does, so walking the members in index order, whatever their kind, with tmax = the best distance so far gives
// the closest hit, the plain hit on equal distance, then the lower member index.
//
// Under the math contract of tfdm_core.hip.h: plain C++17, no contraction; hipcc and g++ compile it to the same bits.  The
// object-space direction is not renormalised: nrtdsm::trace_ray divides by |dir|^2 where it needs a length (recSq).
#pragma once
#include "../tfdm/tfdm_instance.hip.h"
#include "nrtdsm_core.hip.h"

namespace gfx {
namespace nrtdsm {

constexpr uint32_t kKindTfdm = GFX_INSTANCE_TFDM, kKindNrtdsm = GFX_INSTANCE_NRTDSM;
GFX_TFDM_FN uint32_t instance_kind(const InstanceRecord& r) { return r.pad0; }

// One step of the merge rule for a record of kind 1, as tfdm::scene_instance_local is for kind 0: instance `index` against the
// world ray, accepted only where closer than `best`.  kAny: returns at the first hit and leaves `best` alone.  `stack` is emptied
// first.
template <bool kAny, class Stack>
GFX_TFDM_FN bool scene_instance_nrtdsm(const InstanceRecord& r, uint32_t index, V3 org, V3 dir, float tmin, Stack& stack, SceneHit& best, TraceStats& ts) {
    V3 objOrg, objDir;
    to_object_ray(r, org, dir, objOrg, objDir);
    Map map;
    map.heights = r.heights; map.pyramid = r.pyramid;
    TraceHit h;
    stack.sp = 0;
    if (!trace_ray<kAny>(r.nodes, reinterpret_cast<const PrismRecord*>(r.records), map, r.params, objOrg, objDir, tmin, best.dist, stack, h, ts)) return false;
    if (!kAny) {
        best.dist = h.t; best.bcB = h.bcB; best.bcC = h.bcC; best.index = h.prim;
        best.normal = normal_to_world(r, h.normal);
        best.where = (index << 1) | h.frontFace;
    }
    return true;
}

// ---------------------------------------------------------------- host
// ... with the step chosen by the record's kind (k_scene_instances_mixed names its own).  The counters of both kinds go into one
// nrtdsm::TraceStats (maxIterations stays what the NRTDSM members made it).
template <bool kAny, class Stack>
inline bool scene_instance_any_kind(const InstanceRecord& r, uint32_t index, V3 org, V3 dir, float tmin, Stack& stack, SceneHit& best, TraceStats& ts) {
    if (instance_kind(r) == kKindNrtdsm) return scene_instance_nrtdsm<kAny>(r, index, org, dir, tmin, stack, best, ts);
    tfdm::TraceStats t;
    t.aabbTests = 0u; t.leafTests = 0u; t.primTests = 0u;
    const bool hit = tfdm::scene_instance<kAny>(r, index, org, dir, tmin, stack, best, t);
    ts.aabbTests += t.aabbTests; ts.leafTests += t.leafTests; ts.primTests += t.primTests;
    return hit;
}

// make_instance for a member of either kind: the record of tfdm_instance.hip.h with the kind in its pad0 word
inline const char* make_instance_of_kind(uint32_t kind, const float objToWorld[12], const Node& root, const Node* nodes, const void* records, const float* heights,
                                         const F2* pyramid, const Params& params, uint32_t userId, InstanceRecord& out) {
    const char* err = make_instance(objToWorld, root, nodes, static_cast<const TriRecord*>(records), heights, pyramid, params, userId, out);
    if (!err) out.pad0 = kind;
    return err;
}

} // namespace nrtdsm
} // namespace gfx
