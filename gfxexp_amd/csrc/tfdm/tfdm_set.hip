// tfdm_set.hip -- plain and displaced instances in one ray query (gfx_trace_scene): what one optixTrace on an instance AS of
// triangle GASes and custom-primitive GASes does in the reference (tfdm/tfdm_main.cpp:2620-2640).  Two phases on one stream:
//
//   plain phase      the scene BVH8 through the persistent k_trace (trace_launch), unchanged: its refill keeps the lanes of a
//                    wave busy, which a one-wave block beside a TFDM descent could not
//   instance phase   k_scene_instances<ANY_HIT, BILINEAR>: one ray per lane, one wave per block (the launch shape of k_tfdm_trace and for
//                    its reason, tfdm.hip).  A lane starts from the plain result and walks the instance table in index order; the
//                    record is read through the wave-uniform loop index, so the matrices, Params and pointers live in scalar
//                    registers.  A lane whose ray passes the instance's padded world box takes the ray to object space and runs
//                    tfdm::trace_ray with tmax = its best distance so far (tfdm_instance.hip.h: that is the merge rule); an
//                    instance no lane of the wave enters is skipped by ballot.  BILINEAR: the instantiation that can run a member of
//                    GFX_TFDM_BILINEAR (its mode is read through the same wave-uniform record); launched only for a set that has
//                    one, so a set of Box and TwoTriangle members runs the code it ran before that mode existed.
//   ... mixed        k_scene_instances_mixed<ANY_HIT, BILINEAR>: the same phase for a set that has an NRTDSM member (gfx_tfdm_set_add_nrtdsm).
//                    Same launch shape, same walk over all members in index order; after the box test and the ballot skip a lane
//                    branches on the record's kind word, which is wave-uniform like the rest of the record, to tfdm::trace_ray or
//                    nrtdsm::trace_ray (nrtdsm/nrtdsm_instance.hip.h).  One walk, not one per kind: a later phase accepts only
//                    t < tmax, so on equal distance a higher-index member of the first phase would beat a lower-index one of the
//                    second.  Launched only for a set with such a member: a set of TFDM members launches what it always did.
//   ... shell        k_scene_instances_shell<ANY_HIT, BILINEAR>: the same phase for a set that has a shell member (gfx_tfdm_set_add_shell),
//                    whatever else it holds.  The mixed walk with a third wave-uniform branch, to shell::trace_ray
//                    (nrtdsm/shell_instance.hip.h), a second LDS column per lane for the shell BVH's stack (24 KB per block, as
//                    k_shell_trace), the world ray and the merged hit parked in LDS during a descent (6 KB more) and, for
//                    gfx_trace_scene_ex, a third float4 per closest hit: the shell triangle, its geometry and the tile of the
//                    winning shell member, zeros for any other winner.  Launched only for a set with such a member: every other
//                    set launches what it always did.
//
// Register count, scratch and occupancy: DESIGN.md sections 15, 18, 22 and 23.
#include <algorithm>
#include <cstring>
#include <limits>
#include "tfdm_set.h"
#include "tfdm_lds_stack.hip.h"
#include "../nrtdsm/displaced_kinds.hip.h"

namespace gfx {

using namespace tfdm;

namespace {

constexpr int kSceneBlock = 64;
using SceneStack = LdsColumnStack<kSceneBlock>;

template <bool ANY_HIT, bool BILINEAR>
__global__ void __launch_bounds__(kSceneBlock) k_scene_instances(const InstanceRecord* __restrict__ table, uint32_t numInstances, const float4* __restrict__ rayOrgTmin,
                                                                 const float4* __restrict__ rayDirTmax, uint32_t numRays, const uint32_t* __restrict__ numRaysPtr, const void* plain,
                                                                 void* out, unsigned long long* __restrict__ counters) {
    __shared__ uint2 s_stack[kStackDepth * kSceneBlock];
    if (numRaysPtr) {                            // a device-side count: the launch covers the queue capacity
        const uint32_t count = *numRaysPtr;
        numRays = count < numRays ? count : numRays;
        if (blockIdx.x * kSceneBlock >= numRays) return;
    }
    const uint32_t i = blockIdx.x * kSceneBlock + threadIdx.x;
    const bool live = i < numRays;
    TraceStats ts;
    ts.aabbTests = 0u; ts.leafTests = 0u; ts.primTests = 0u;
    uint32_t boxTests = 0u, traversals = 0u;
    V3 org = v3(0.0f, 0.0f, 0.0f), dir = v3(0.0f, 0.0f, 1.0f);
    float tmin = 0.0f;
    SceneHit best = scene_miss(0.0f);
    bool occluded = false;
    if (live) {
        const float4 o = rayOrgTmin[i], d = rayDirTmax[i];
        org = v3(o.x, o.y, o.z); dir = v3(d.x, d.y, d.z); tmin = o.w;
        best = scene_miss(d.w);
        if (plain) {
            if (ANY_HIT) occluded = static_cast<const uint32_t*>(plain)[i] != 0u;
            else {
                const float4 h = static_cast<const float4*>(plain)[i];          // a gfx_hit
                best = scene_start(d.w, h.x, h.y, h.z, f2b(h.w));
            }
        }
    }
    const V3 inv = v3(1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z);
    SceneStack stack;
    stack.col = s_stack + threadIdx.x;
    stack.sp = 0;
    // the lane still looks for a hit; a shadow-ray slot without a ray (tmax = -1, zero direction: restir_common.hip.h emit_ray_at_slot)
    // enters no instance and keeps the 0 k_trace wrote
    bool open = live && !occluded && (!ANY_HIT || best.dist > tmin);
    for (uint32_t k = 0; k < numInstances; ++k) {
        const InstanceRecord& r = table[k];
        bool enter = false;
        if (open) { ++boxTests; enter = world_box_hit(r, org, inv, tmin, best.dist); }
        if (__ballot(enter) == 0ull) continue;
        if (enter) {
            ++traversals;
            if (scene_instance_local<ANY_HIT, BILINEAR>(r, k, org, dir, tmin, stack, best, ts) && ANY_HIT) { occluded = true; open = false; }
        }
    }
    if (live) {
        if (ANY_HIT) static_cast<uint32_t*>(out)[i] = occluded ? 1u : 0u;
        else {
            float4* h = static_cast<float4*>(out) + 2u * i;
            h[0] = make_float4(best.dist, best.bcB, best.bcC, b2f(best.index));
            h[1] = make_float4(best.normal.x, best.normal.y, best.normal.z, b2f(best.where));
        }
    }
    if (counters) {                      // per wave, one atomic each
        const uint32_t a = wave_sum(ts.aabbTests), l = wave_sum(ts.leafTests), n = wave_sum(live ? 1u : 0u), t = wave_sum(ts.primTests);
        const uint32_t b = wave_sum(boxTests), v = wave_sum(traversals);
        if ((threadIdx.x & 63u) == 0) {
            atomicAdd(counters + 0, a); atomicAdd(counters + 1, l); atomicAdd(counters + 2, n); atomicAdd(counters + 3, t);
            atomicAdd(counters + 4, b); atomicAdd(counters + 5, v);
        }
    }
}

// The instance phase over members of both kinds.  k_scene_instances above stays as it is for sets without an NRTDSM member, so
// their instruction stream does not change; this is its text with the branch on the kind and the second set of counters.
template <bool ANY_HIT, bool BILINEAR>
__global__ void __launch_bounds__(kSceneBlock) k_scene_instances_mixed(const InstanceRecord* __restrict__ table, uint32_t numInstances, const float4* __restrict__ rayOrgTmin,
                                                                       const float4* __restrict__ rayDirTmax, uint32_t numRays, const uint32_t* __restrict__ numRaysPtr,
                                                                       const void* plain, void* out, unsigned long long* __restrict__ counters) {
    __shared__ uint2 s_stack[kStackDepth * kSceneBlock];
    if (numRaysPtr) {                            // a device-side count: the launch covers the queue capacity
        const uint32_t count = *numRaysPtr;
        numRays = count < numRays ? count : numRays;
        if (blockIdx.x * kSceneBlock >= numRays) return;
    }
    const uint32_t i = blockIdx.x * kSceneBlock + threadIdx.x;
    const bool live = i < numRays;
    TraceStats ts;                               // of the TFDM members
    ts.aabbTests = 0u; ts.leafTests = 0u; ts.primTests = 0u;
    nrtdsm::TraceStats ns;                       // of the NRTDSM members
    ns.aabbTests = 0u; ns.leafTests = 0u; ns.primTests = 0u; ns.maxIterations = 0u;
    uint32_t boxTests = 0u, traversals = 0u;
    V3 org = v3(0.0f, 0.0f, 0.0f), dir = v3(0.0f, 0.0f, 1.0f);
    float tmin = 0.0f;
    SceneHit best = scene_miss(0.0f);
    bool occluded = false;
    if (live) {
        const float4 o = rayOrgTmin[i], d = rayDirTmax[i];
        org = v3(o.x, o.y, o.z); dir = v3(d.x, d.y, d.z); tmin = o.w;
        best = scene_miss(d.w);
        if (plain) {
            if (ANY_HIT) occluded = static_cast<const uint32_t*>(plain)[i] != 0u;
            else {
                const float4 h = static_cast<const float4*>(plain)[i];          // a gfx_hit
                best = scene_start(d.w, h.x, h.y, h.z, f2b(h.w));
            }
        }
    }
    const V3 inv = v3(1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z);
    SceneStack stack;
    stack.col = s_stack + threadIdx.x;
    stack.sp = 0;
    bool open = live && !occluded && (!ANY_HIT || best.dist > tmin);       // as k_scene_instances
    for (uint32_t k = 0; k < numInstances; ++k) {
        const InstanceRecord& r = table[k];
        bool enter = false;
        if (open) { ++boxTests; enter = world_box_hit(r, org, inv, tmin, best.dist); }
        if (__ballot(enter) == 0ull) continue;
        if (enter) {
            ++traversals;
            bool hit;
            if (nrtdsm::instance_kind(r) == nrtdsm::kKindNrtdsm) hit = nrtdsm::scene_instance_nrtdsm<ANY_HIT>(r, k, org, dir, tmin, stack, best, ns);
            else hit = scene_instance_local<ANY_HIT, BILINEAR>(r, k, org, dir, tmin, stack, best, ts);
            if (hit && ANY_HIT) { occluded = true; open = false; }
        }
    }
    if (live) {
        if (ANY_HIT) static_cast<uint32_t*>(out)[i] = occluded ? 1u : 0u;
        else {
            float4* h = static_cast<float4*>(out) + 2u * i;
            h[0] = make_float4(best.dist, best.bcB, best.bcC, b2f(best.index));
            h[1] = make_float4(best.normal.x, best.normal.y, best.normal.z, b2f(best.where));
        }
    }
    if (counters) {                      // per wave, one atomic each; [0..3] sum over both kinds
        const uint32_t a = wave_sum(ts.aabbTests + ns.aabbTests), l = wave_sum(ts.leafTests + ns.leafTests), n = wave_sum(live ? 1u : 0u);
        const uint32_t t = wave_sum(ts.primTests + ns.primTests), b = wave_sum(boxTests), v = wave_sum(traversals);
        if ((threadIdx.x & 63u) == 0) {
            atomicAdd(counters + 0, a); atomicAdd(counters + 1, l); atomicAdd(counters + 2, n); atomicAdd(counters + 3, t);
            atomicAdd(counters + 4, b); atomicAdd(counters + 5, v);
        }
    }
}

// The instance phase over members of all three kinds, for a set that has a shell member.  The two kernels above stay as they are,
// so sets without one run the instruction stream they ran; this is k_scene_instances_mixed's walk with the third branch and the
// second LDS column (the shell BVH's stack; the first serves the base tree of whichever kind runs, only one runs at a time:
// 24 KB per block, as k_shell_trace has).
//
// Registers.  shell::trace_ray alone needs 232 VGPRs (k_shell_trace<false>), so what the walk keeps across a
// descent has to be small for two waves per SIMD.  Nothing but the best distance, the two stacks' pointers and the counters is:
//   * the world ray and its reciprocal lie in LDS (s_lane, three float4 per lane) and are read back per member, for the box test
//     and for to_object_ray;
//   * the merged hit lies there too (three more float4: bcB, bcC, index, where / the normal / the shell part).  A step works on a
//     hit of its own that starts as a miss at the best distance; where it finds something the lane overwrites its LDS entry,
//     and a hit of another kind clears the shell part that way;
//   * all kinds count into one nrtdsm::TraceStats (a TFDM step through a TraceStats of its own, added afterwards).
// That is 6 KB more LDS, 30 KB per block: five blocks per CU by LDS, where the registers of the plain form allow four.
// amdgpu_waves_per_eu(2, 2) holds the allocation at 256 registers; without it the closest-hit variants take 257 and 258 and
// lose the second wave (section 23 has the table, and what the plain form costs).
// `shellPart` (closest only, optional): one float4 per ray, zero unless the winning hit is a shell member's.
constexpr int kLaneOrg = 0, kLaneDir = 1, kLaneInv = 2, kLaneHit = 3, kLaneNormal = 4, kLanePart = 5, kLaneSlots = 6;

template <bool ANY_HIT, bool BILINEAR>
__global__ void __launch_bounds__(kSceneBlock) __attribute__((amdgpu_waves_per_eu(2, 2)))
k_scene_instances_shell(const InstanceRecord* __restrict__ table, uint32_t numInstances, const float4* __restrict__ rayOrgTmin, const float4* __restrict__ rayDirTmax,
                        uint32_t numRays, const uint32_t* __restrict__ numRaysPtr, const void* plain, void* out, unsigned long long* __restrict__ counters,
                        float4* __restrict__ shellPart) {
    __shared__ uint2 s_stack[kStackDepth * kSceneBlock];
    __shared__ uint2 s_shellStack[kStackDepth * kSceneBlock];
    __shared__ float4 s_lane[kLaneSlots * kSceneBlock];          // [slot][lane]: a lane reads and writes only its own column
    if (numRaysPtr) {                            // a device-side count: the launch covers the queue capacity
        const uint32_t count = *numRaysPtr;
        numRays = count < numRays ? count : numRays;
        if (blockIdx.x * kSceneBlock >= numRays) return;
    }
    const uint32_t i = blockIdx.x * kSceneBlock + threadIdx.x;
    const bool live = i < numRays;
    nrtdsm::TraceStats ns;                       // of all members
    ns.aabbTests = 0u; ns.leafTests = 0u; ns.primTests = 0u; ns.maxIterations = 0u;
    uint32_t boxTests = 0u, traversals = 0u;
    float4* const mine = s_lane + threadIdx.x;
    float bestDist = 0.0f;
    bool occluded = false, open;
    {
        V3 org = v3(0.0f, 0.0f, 0.0f), dir = v3(0.0f, 0.0f, 1.0f);
        float tmin = 0.0f;
        SceneHit best = scene_miss(0.0f);
        if (live) {
            const float4 o = rayOrgTmin[i], d = rayDirTmax[i];
            org = v3(o.x, o.y, o.z); dir = v3(d.x, d.y, d.z); tmin = o.w;
            best = scene_miss(d.w);
            if (plain) {
                if (ANY_HIT) occluded = static_cast<const uint32_t*>(plain)[i] != 0u;
                else {
                    const float4 h = static_cast<const float4*>(plain)[i];          // a gfx_hit
                    best = scene_start(d.w, h.x, h.y, h.z, f2b(h.w));
                }
            }
        }
        bestDist = best.dist;
        open = live && !occluded && (!ANY_HIT || best.dist > tmin);       // as k_scene_instances
        mine[kLaneOrg * kSceneBlock] = make_float4(org.x, org.y, org.z, tmin);
        mine[kLaneDir * kSceneBlock] = make_float4(dir.x, dir.y, dir.z, 0.0f);
        mine[kLaneInv * kSceneBlock] = make_float4(1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z, 0.0f);
        if (!ANY_HIT) {
            mine[kLaneHit * kSceneBlock] = make_float4(best.bcB, best.bcC, b2f(best.index), b2f(best.where));
            mine[kLaneNormal * kSceneBlock] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            mine[kLanePart * kSceneBlock] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
    SceneStack stack, shellStack;
    stack.col = s_stack + threadIdx.x;
    stack.sp = 0;
    shellStack.col = s_shellStack + threadIdx.x;
    shellStack.sp = 0;
    for (uint32_t k = 0; k < numInstances; ++k) {
        const InstanceRecord& r = table[k];
        bool enter = false;
        if (open) {
            const float4 o = mine[kLaneOrg * kSceneBlock], iv = mine[kLaneInv * kSceneBlock];
            ++boxTests;
            enter = world_box_hit(r, v3(o.x, o.y, o.z), v3(iv.x, iv.y, iv.z), o.w, bestDist);
        }
        if (__ballot(enter) == 0ull) continue;
        if (enter) {
            const float4 o = mine[kLaneOrg * kSceneBlock], d = mine[kLaneDir * kSceneBlock];
            const V3 org = v3(o.x, o.y, o.z), dir = v3(d.x, d.y, d.z);
            ++traversals;
            const uint32_t kind = nrtdsm::instance_kind(r);
            SceneHit h = scene_miss(bestDist);                  // the step's own: a step accepts only what is closer than h.dist
            shell::ShellPart hp = shell::shell_part_none();
            bool hit;
            if (kind == shell::kKindShell) hit = shell::scene_instance_shell<ANY_HIT>(r, k, org, dir, o.w, stack, shellStack, h, hp, ns);
            else if (kind == nrtdsm::kKindNrtdsm) hit = nrtdsm::scene_instance_nrtdsm<ANY_HIT>(r, k, org, dir, o.w, stack, h, ns);
            else {
                TraceStats ts;
                ts.aabbTests = 0u; ts.leafTests = 0u; ts.primTests = 0u;
                hit = scene_instance_local<ANY_HIT, BILINEAR>(r, k, org, dir, o.w, stack, h, ts);
                ns.aabbTests += ts.aabbTests; ns.leafTests += ts.leafTests; ns.primTests += ts.primTests;
            }
            if (hit) {
                if (ANY_HIT) { occluded = true; open = false; }
                else {
                    bestDist = h.dist;
                    mine[kLaneHit * kSceneBlock] = make_float4(h.bcB, h.bcC, b2f(h.index), b2f(h.where));
                    mine[kLaneNormal * kSceneBlock] = make_float4(h.normal.x, h.normal.y, h.normal.z, 0.0f);
                    // zeros where the winner is no shell member
                    mine[kLanePart * kSceneBlock] = make_float4(b2f(hp.shellTriangle), b2f(hp.shellGeom), b2f(static_cast<uint32_t>(hp.tileX)), b2f(static_cast<uint32_t>(hp.tileY)));
                }
            }
        }
    }
    if (live) {
        if (ANY_HIT) static_cast<uint32_t*>(out)[i] = occluded ? 1u : 0u;
        else {
            float4* h = static_cast<float4*>(out) + 2u * i;
            const float4 a = mine[kLaneHit * kSceneBlock], n = mine[kLaneNormal * kSceneBlock];
            h[0] = make_float4(bestDist, a.x, a.y, a.z);
            h[1] = make_float4(n.x, n.y, n.z, a.w);
            if (shellPart) shellPart[i] = mine[kLanePart * kSceneBlock];
        }
    }
    if (counters) {                      // per wave, one atomic each; [0..3] sum over all kinds
        const uint32_t a = wave_sum(ns.aabbTests), l = wave_sum(ns.leafTests), n = wave_sum(live ? 1u : 0u);
        const uint32_t t = wave_sum(ns.primTests), b = wave_sum(boxTests), v = wave_sum(traversals);
        if ((threadIdx.x & 63u) == 0) {
            atomicAdd(counters + 0, a); atomicAdd(counters + 1, l); atomicAdd(counters + 2, n); atomicAdd(counters + 3, t);
            atomicAdd(counters + 4, b); atomicAdd(counters + 5, v);
        }
    }
}

void check_member(const TfdmSet& s, const DisplacedObject* obj) {
    if (!obj) throw HipError("gfx_tfdm_set: null object");
    if (obj->device != s.device) throw HipError("gfx_tfdm_set: the object belongs to another device");
}

uint32_t add_member(TfdmSet& s, DisplacedObject* obj, uint32_t kind, const float objToWorld[12], uint32_t userId, const char* who) {
    check_member(s, obj);
    if (!objToWorld) throw HipError(std::string(who) + ": null transform");
    if (s.members.size() >= kMaxInstances) throw HipError(std::string(who) + ": a set holds at most 1024 instances");
    TfdmSet::Member m;
    m.obj = obj; m.kind = kind; m.userId = userId; m.generation = 0;
    std::memcpy(m.objToWorld, objToWorld, sizeof(m.objToWorld));
    std::memcpy(m.prevObjToWorld, objToWorld, sizeof(m.prevObjToWorld));
    s.members.push_back(m);
    s.dirty = true;
    return static_cast<uint32_t>(s.members.size() - 1);
}

// root and generation live in the three derived objects; the kind says which one `obj` is
bool is_nrtdsm(const TfdmSet::Member& m) { return m.kind == GFX_INSTANCE_NRTDSM; }
bool is_shell(const TfdmSet::Member& m) { return m.kind == GFX_INSTANCE_SHELL; }
uint64_t generation_of(const TfdmSet::Member& m) {
    if (is_shell(m)) return static_cast<const ShellObject*>(m.obj)->generation;
    return is_nrtdsm(m) ? static_cast<const NrtdsmObject*>(m.obj)->generation : static_cast<const TfdmObject*>(m.obj)->generation;
}
const Node& root_of(const TfdmSet::Member& m) {
    if (is_shell(m)) return static_cast<const ShellObject*>(m.obj)->root;
    return is_nrtdsm(m) ? static_cast<const NrtdsmObject*>(m.obj)->root : static_cast<const TfdmObject*>(m.obj)->root;
}
// the call after which a member's object has buffers the committed record does not know
const char* stale_call_of(const TfdmSet::Member& m) {
    if (is_shell(m)) return static_cast<const ShellObject*>(m.obj)->lastChange;
    if (const char* call = static_cast<const HeightMapObject*>(m.obj)->lastChange) return call;
    return is_nrtdsm(m) ? "gfx_nrtdsm_set_params" : "gfx_tfdm_set_params";
}
bool has_nrtdsm(const TfdmSet& s) {
    for (const TfdmSet::Member& m : s.members) if (is_nrtdsm(m)) return true;
    return false;
}
bool has_shell(const TfdmSet& s) {
    for (const TfdmSet::Member& m : s.members) if (is_shell(m)) return true;
    return false;
}
const char* const kNotRendered = "the set has an NRTDSM instance; NRTDSM instances are traced (gfx_trace_scene) but not rendered through this binding "
                                 "(gfx_scene_bind_displaced_kinds renders them)";
const char* const kShellNotRendered = "the set has a shell instance; shell instances are traced (gfx_trace_scene) but not rendered through this binding "
                                      "(gfx_scene_bind_displaced_kinds renders them)";
// a set that is traced but cannot be bound by gfx_scene_bind_displaced / _passes: the message, or null
const char* not_rendered(const TfdmSet& s) { return has_nrtdsm(s) ? kNotRendered : has_shell(s) ? kShellNotRendered : nullptr; }

// What gfx_scene_bind_displaced_kinds asks of member `m` beyond its geometry, at the bind and again at every launch (the shell
// object's geometry and the materials may have changed in between): the refusal without the member's index, or empty.
std::string kinds_member_refusal(const Context& ctx, const TfdmSet::Member& m, const gfx_displaced_member& d) {
    if (!is_shell(m)) {
        if (d.numShellMaterials != 0u)
            return "numShellMaterials is " + std::to_string(d.numShellMaterials) + " for a member that is not a shell member (it must be 0)";
        return std::string();
    }
    const uint32_t numGeoms = static_cast<const ShellObject*>(m.obj)->numGeoms;
    if (d.numShellMaterials != numGeoms)
        return std::to_string(d.numShellMaterials) + " shell materials for a shell object of " + std::to_string(numGeoms) + " shell geometries (shell geometry count mismatch)";
    if (d.geomInstSlot >= (1u << tfdm::kGeomSlotBits))
        return "geometry slot " + std::to_string(d.geomInstSlot) + " of a shell member must be below 2^28 (the G-buffer keeps the shell geometry in the upper four bits)";
    for (uint32_t g = 0; g < numGeoms; ++g) {
        const uint32_t slot = d.shellMatSlots[g];
        if (slot >= ctx.materials.size()) return "unknown material slot " + std::to_string(slot) + " for shell geometry " + std::to_string(g);
        if (ctx.materials[slot].hasEmittance)
            return "the material of shell geometry " + std::to_string(g) + " (slot " + std::to_string(slot) + ") has emittance; displaced emitters are not supported";
    }
    return std::string();
}

// the checks both bind calls make of the geometry member k is shaded with
void check_bound_geometry(const Context& ctx, const TfdmSet& set, uint32_t k, uint32_t geomSlot, const std::string& who) {
    if (geomSlot >= ctx.geoms.size()) throw HipError(who + "unknown geometry slot " + std::to_string(geomSlot));
    const HostGeom& g = ctx.geoms[geomSlot];
    if (g.triangles.size() / 3 != set.members[k].obj->numTriangles)
        throw HipError(who + "geometry slot " + std::to_string(geomSlot) + " has " + std::to_string(g.triangles.size() / 3) + " triangles, the displaced object " +
                       std::to_string(set.members[k].obj->numTriangles) + " (triangle count mismatch)");
    if (g.materialSlot < ctx.materials.size() && ctx.materials[g.materialSlot].hasEmittance)
        throw HipError(who + "the material of geometry slot " + std::to_string(geomSlot) + " has emittance; displaced emitters are not supported");
}

void unbind(DisplacedBinding& b) { b.set = nullptr; b.geomSlots.clear(); b.passMask = 0u; b.kinds = false; b.members.clear(); }

} // namespace

uint32_t tfdm_set_add(TfdmSet& s, TfdmObject* obj, const float objToWorld[12], uint32_t userId) {
    return add_member(s, obj, GFX_INSTANCE_TFDM, objToWorld, userId, "gfx_tfdm_set_add");
}

uint32_t tfdm_set_add_nrtdsm(TfdmSet& s, NrtdsmObject* obj, const float objToWorld[12], uint32_t userId) {
    return add_member(s, obj, GFX_INSTANCE_NRTDSM, objToWorld, userId, "gfx_tfdm_set_add_nrtdsm");
}

uint32_t tfdm_set_add_shell(TfdmSet& s, ShellObject* obj, const float objToWorld[12], uint32_t userId) {
    return add_member(s, obj, GFX_INSTANCE_SHELL, objToWorld, userId, "gfx_tfdm_set_add_shell");
}

void tfdm_set_transform(TfdmSet& s, uint32_t index, const float objToWorld[12]) {
    if (index >= s.members.size()) throw HipError("gfx_tfdm_set_transform: no such instance");
    if (!objToWorld) throw HipError("gfx_tfdm_set_transform: null transform");
    std::memcpy(s.members[index].objToWorld, objToWorld, sizeof(s.members[index].objToWorld));
    std::memcpy(s.members[index].prevObjToWorld, objToWorld, sizeof(s.members[index].prevObjToWorld));      // a teleport: no motion
    s.dirty = true;
}

// InstanceController::update for a displaced instance, as gfx_instance_set_transform is for a plain one.
void tfdm_set_move(TfdmSet& s, uint32_t index, const float objToWorld[12]) {
    if (index >= s.members.size()) throw HipError("gfx_tfdm_set_move: no such instance");
    if (!objToWorld) throw HipError("gfx_tfdm_set_move: null transform");
    TfdmSet::Member& m = s.members[index];
    std::memcpy(m.prevObjToWorld, m.objToWorld, sizeof(m.prevObjToWorld));
    std::memcpy(m.objToWorld, objToWorld, sizeof(m.objToWorld));
    s.dirty = true;
}

// The records and the motion table are derived into fresh tables and swapped in only when every one of them worked.
void tfdm_set_commit(TfdmSet& s, hipStream_t stream) {
    std::vector<InstanceRecord> recs(s.members.size());
    std::vector<float> motion(12 * s.members.size());
    for (size_t k = 0; k < s.members.size(); ++k) {
        const TfdmSet::Member& m = s.members[k];
        const char* err;
        if (is_shell(m)) {
            const ShellObject& o = *static_cast<const ShellObject*>(m.obj);
            err = shell::make_shell_instance(m.objToWorld, o.root, o.nodes.as<Node>(), o.records.as<nrtdsm::PrismRecord>(), o.shellNodes.as<Node>(),
                                             o.shellTris.as<shell::ShellTri>(), o.params, m.userId, recs[k]);
        }
        else {
            const HeightMapObject& o = *static_cast<const HeightMapObject*>(m.obj);
            err = nrtdsm::make_instance_of_kind(m.kind, m.objToWorld, root_of(m), o.nodes.as<Node>(), o.records.p, o.heights.as<float>(), o.pyramid.as<F2>(), o.params,
                                                m.userId, recs[k]);
        }
        if (!err) err = make_cur_to_prev(m.prevObjToWorld, m.objToWorld, motion.data() + 12 * k);
        if (err) throw HipError("gfx_tfdm_set_commit: instance " + std::to_string(k) + ": " + err);
    }
    if (!recs.empty()) {
        s.table.reserve(sizeof(InstanceRecord) * recs.size());
        s.motion.reserve(sizeof(float) * motion.size());
        GFX_HIP(hipMemcpyAsync(s.table.p, recs.data(), sizeof(InstanceRecord) * recs.size(), hipMemcpyHostToDevice, stream));
        GFX_HIP(hipMemcpyAsync(s.motion.p, motion.data(), sizeof(float) * motion.size(), hipMemcpyHostToDevice, stream));
        GFX_HIP(hipStreamSynchronize(stream));       // `recs` and `motion` are pageable memory
    }
    s.host.swap(recs);
    s.hostMotion.swap(motion);
    s.anyBilinear = false;
    s.anyNrtdsm = false;
    s.anyShell = false;
    for (const InstanceRecord& r : s.host) {
        s.anyBilinear = s.anyBilinear || r.params.local == kBilinear;
        s.anyNrtdsm = s.anyNrtdsm || nrtdsm::instance_kind(r) == nrtdsm::kKindNrtdsm;
        s.anyShell = s.anyShell || nrtdsm::instance_kind(r) == shell::kKindShell;
    }
    for (TfdmSet::Member& m : s.members) m.generation = generation_of(m);
    s.dirty = false;
}

void tfdm_set_read(TfdmSet& s, void* hostOut, size_t bytes) {
    if (s.dirty) throw HipError("gfx_tfdm_set_read: the set has an add or a transform that is not committed");
    const size_t need = sizeof(InstanceRecord) * s.host.size();
    if (bytes != need || (need && !hostOut)) throw HipError("gfx_tfdm_set_read: the buffer must hold exactly 192 bytes per instance");
    if (!need) return;
    GFX_HIP(hipDeviceSynchronize());
    GFX_HIP(hipMemcpy(hostOut, s.table.p, need, hipMemcpyDeviceToHost));
}

void tfdm_set_bounds(const TfdmSet& s, float lo[3], float hi[3]) {
    if (s.dirty) throw HipError("gfx_tfdm_set_bounds: the set has an add, a transform or a move that is not committed");
    if (!lo || !hi) throw HipError("gfx_tfdm_set_bounds: null output");
    for (int k = 0; k < 3; ++k) { lo[k] = std::numeric_limits<float>::infinity(); hi[k] = -std::numeric_limits<float>::infinity(); }
    for (const InstanceRecord& r : s.host)
        for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], r.boxLo[k]); hi[k] = std::max(hi[k], r.boxHi[k]); }
}

void tfdm_set_read_motion(TfdmSet& s, void* hostOut, size_t bytes) {
    if (s.dirty) throw HipError("gfx_tfdm_set_read_motion: the set has an add, a transform or a move that is not committed");
    const size_t need = sizeof(float) * s.hostMotion.size();
    if (bytes != need || (need && !hostOut)) throw HipError("gfx_tfdm_set_read_motion: the buffer must hold exactly 48 bytes per instance");
    if (!need) return;
    GFX_HIP(hipDeviceSynchronize());
    GFX_HIP(hipMemcpy(hostOut, s.motion.p, need, hipMemcpyDeviceToHost));
}

void tfdm_set_release(TfdmSet& s) { s.table.release(); s.motion.release(); s.plain.release(); }

void trace_scene_check_set(const TfdmSet& set, int device, const char* who) {
    const std::string w(who);
    if (set.device != device) throw HipError(w + ": the instance set belongs to another device");
    if (set.dirty) throw HipError(w + ": the instance set has an add or a transform that is not committed (gfx_tfdm_set_commit)");
    for (size_t k = 0; k < set.members.size(); ++k)
        if (set.members[k].generation != generation_of(set.members[k]))
            throw HipError(w + ": instance " + std::to_string(k) + "'s object had " + stale_call_of(set.members[k]) +
                           " after the set was committed; commit the set again");
}

void trace_scene_launch(Context& ctx, hipStream_t stream, const SceneTrace& s) {
    if (s.numRays == 0) return;
    const bool any = s.mode == GFX_TRACE_ANY;
    const uint32_t numInstances = s.set ? static_cast<uint32_t>(s.set->host.size()) : 0u;
    // Plain phase.  An any-hit answer has the output's own format: k_trace writes it in place and the instance phase goes over
    // it.  A closest hit is a 16-byte gfx_hit that the instance phase widens, so it goes through a buffer.
    const void* plain = nullptr;
    if (s.accel) {
        void* dst = any ? s.out : s.plainHits;
        TraceLaunch t;
        t.accel = *s.accel;
        t.rayOrgTmin = s.rayOrgTmin; t.rayDirTmax = s.rayDirTmax;
        t.numRays = s.numRays; t.numRaysPtr = s.numRaysPtr; t.out = dst; t.mode = s.mode;
        t.spill = s.spill; t.counters = s.counters;
        t.zeroWords[0] = s.zeroWords[0]; t.zeroWords[1] = s.zeroWords[1];
        t.hintFromOut = s.hintFromOut;
        trace_launch(ctx, stream, t);
        plain = dst;
        if (any && numInstances == 0 && !s.statCounters) return;
    }
    else {
        // no plain phase to zero the queue heads a path tracer hands over: stream order does
        for (uint32_t* w : s.zeroWords) if (w) GFX_HIP(hipMemsetAsync(w, 0, sizeof(uint32_t), stream));
    }
    const uint32_t blocks = (s.numRays + kSceneBlock - 1u) / kSceneBlock;
    const InstanceRecord* table = numInstances ? s.set->table.as<InstanceRecord>() : nullptr;
    unsigned long long* cnt = static_cast<unsigned long long*>(s.statCounters);
    ScopedKernelTimer timer(ctx, stream, "k_scene_instances");
    auto launch = [&](auto kernel) {
        kernel<<<blocks, kSceneBlock, 0, stream>>>(table, numInstances, s.rayOrgTmin, s.rayDirTmax, s.numRays, s.numRaysPtr, plain, s.out, cnt);
    };
    const bool shellPhase = numInstances && s.set->anyShell;
    // the side record of a closest hit is all zeros where no shell member can win: the kernels of such a set do not know it
    if (s.shellPart && !any && !shellPhase) GFX_HIP(hipMemsetAsync(s.shellPart, 0, sizeof(gfx_scene_shell_part) * static_cast<size_t>(s.numRays), stream));
    if (shellPhase) {
        auto launchShell = [&](auto kernel) {
            kernel<<<blocks, kSceneBlock, 0, stream>>>(table, numInstances, s.rayOrgTmin, s.rayDirTmax, s.numRays, s.numRaysPtr, plain, s.out, cnt,
                                                       any ? nullptr : static_cast<float4*>(s.shellPart));
        };
        if (!s.set->anyBilinear) launchShell(any ? k_scene_instances_shell<true, false> : k_scene_instances_shell<false, false>);
        else launchShell(any ? k_scene_instances_shell<true, true> : k_scene_instances_shell<false, true>);
    }
    else if (numInstances && s.set->anyNrtdsm) {
        if (!s.set->anyBilinear) launch(any ? k_scene_instances_mixed<true, false> : k_scene_instances_mixed<false, false>);
        else launch(any ? k_scene_instances_mixed<true, true> : k_scene_instances_mixed<false, true>);
    }
    else if (!(numInstances && s.set->anyBilinear)) launch(any ? k_scene_instances<true, false> : k_scene_instances<false, false>);
    else launch(any ? k_scene_instances<true, true> : k_scene_instances<false, true>);
    GFX_HIP(hipGetLastError());
}

void displaced_bind(Context& ctx, TfdmSet* set, const uint32_t* geomSlots, uint32_t n, uint32_t passMask) {
    DisplacedBinding& b = ctx.displaced;
    if (passMask & ~(GFX_DISPLACED_GBUFFER_PT | GFX_DISPLACED_RESTIR | GFX_DISPLACED_REGIR))
        throw HipError("gfx_scene_bind_displaced_passes: unknown bit in the pass mask " + std::to_string(passMask));
    if (!set) { unbind(b); return; }
    if (set->device != ctx.device) throw HipError("gfx_scene_bind_displaced: the instance set belongs to another device");
    if (const char* why = not_rendered(*set)) throw HipError(std::string("gfx_scene_bind_displaced: ") + why);
    if (n != set->members.size())
        throw HipError("gfx_scene_bind_displaced: " + std::to_string(n) + " geometry slots for a set of " + std::to_string(set->members.size()) + " instances");
    if (n && !geomSlots) throw HipError("gfx_scene_bind_displaced: null geometry slots");
    for (uint32_t k = 0; k < n; ++k) {
        check_bound_geometry(ctx, *set, k, geomSlots[k], "gfx_scene_bind_displaced: instance " + std::to_string(k) + ": ");
    }
    // (a reserve() that has to grow frees the old table with hipFree, which waits for the passes that read it)
    std::vector<uint32_t> slots(geomSlots, geomSlots + n);
    b.dGeomSlots.reserve(std::max<size_t>(sizeof(uint32_t) * n, 16));
    if (n) GFX_HIP(hipMemcpy(b.dGeomSlots.p, slots.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice));
    b.geomSlots.swap(slots);
    b.set = set;
    b.passMask = passMask | GFX_DISPLACED_GBUFFER_PT;
    b.kinds = false;
    b.members.clear();
}

// The binding of displaced_bind with one more table, and without its refusal of NRTDSM and shell members.  Every check comes before
// the first change of the binding: a refused call leaves the binding as it was.
void displaced_bind_kinds(Context& ctx, TfdmSet* set, const gfx_displaced_member* members, uint32_t n, uint32_t passMask) {
    DisplacedBinding& b = ctx.displaced;
    const std::string me = "gfx_scene_bind_displaced_kinds: ";
    if (passMask & ~(GFX_DISPLACED_GBUFFER_PT | GFX_DISPLACED_RESTIR | GFX_DISPLACED_REGIR)) throw HipError(me + "unknown bit in the pass mask " + std::to_string(passMask));
    if (!set) { unbind(b); return; }
    if (set->device != ctx.device) throw HipError(me + "the instance set belongs to another device");
    if (n != set->members.size())
        throw HipError(me + std::to_string(n) + " members for a set of " + std::to_string(set->members.size()) + " instances");
    if (n && !members) throw HipError(me + "null members");
    std::vector<uint32_t> slots(n), mats(static_cast<size_t>(tfdm::kShellMatsPerMember) * n, 0u);
    for (uint32_t k = 0; k < n; ++k) {
        const std::string who = me + "instance " + std::to_string(k) + ": ";
        const std::string why = kinds_member_refusal(ctx, set->members[k], members[k]);       // first: a shell member's slot >= 2^28 is named as such
        if (!why.empty()) throw HipError(who + why);
        check_bound_geometry(ctx, *set, k, members[k].geomInstSlot, who);
        slots[k] = members[k].geomInstSlot;
        for (uint32_t g = 0; g < members[k].numShellMaterials; ++g) mats[tfdm::kShellMatsPerMember * k + g] = members[k].shellMatSlots[g];
    }
    b.dGeomSlots.reserve(std::max<size_t>(sizeof(uint32_t) * n, 16));
    b.dShellMats.reserve(std::max<size_t>(sizeof(uint32_t) * mats.size(), 16));
    if (n) {
        GFX_HIP(hipMemcpy(b.dGeomSlots.p, slots.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice));
        GFX_HIP(hipMemcpy(b.dShellMats.p, mats.data(), sizeof(uint32_t) * mats.size(), hipMemcpyHostToDevice));
    }
    b.geomSlots.swap(slots);
    b.members.assign(members, members + n);
    b.set = set;
    b.passMask = passMask | GFX_DISPLACED_GBUFFER_PT;
    b.kinds = true;
}

void displaced_check(Context& ctx, const char* who) {
    const DisplacedBinding& b = ctx.displaced;
    trace_scene_check_set(*b.set, ctx.device, who);
    if (!b.kinds) if (const char* why = not_rendered(*b.set)) throw HipError(std::string(who) + ": " + why);      // a member added after the bind
    if (b.geomSlots.size() != b.set->members.size())
        throw HipError(std::string(who) + ": the bound instance set has grown since gfx_scene_bind_displaced; bind it again");
    for (size_t k = 0; k < b.geomSlots.size(); ++k) {
        if (b.geomSlots[k] >= ctx.hGeomInsts.size())
            throw HipError(std::string(who) + ": the geometry of displaced instance " + std::to_string(k) + " is not on the device yet (gfx_accel_build uploads the scene)");
        const uint32_t m = ctx.geoms[b.geomSlots[k]].materialSlot;
        if (m < ctx.materials.size() && ctx.materials[m].hasEmittance)
            throw HipError(std::string(who) + ": the material of displaced instance " + std::to_string(k) + " has emittance; displaced emitters are not supported");
        if (b.kinds) {       // gfx_shell_set_geometry (with a new commit) and gfx_material_set may have run since the bind
            const std::string why = kinds_member_refusal(ctx, b.set->members[k], b.members[k]);
            if (!why.empty()) throw HipError(std::string(who) + ": displaced instance " + std::to_string(k) + ": " + why + "; bind the set again");
        }
    }
}

bool displaced_shell_render(const Context& ctx) { return ctx.displaced.set && ctx.displaced.kinds && ctx.displaced.set->anyShell; }

DisplacedShellArgs displaced_shell_args(const Context& ctx, const void* shellPart) {
    DisplacedShellArgs e;
    e.shellPart = static_cast<const float4*>(shellPart);
    e.shellMats = ctx.displaced.dShellMats.as<uint32_t>();
    return e;
}

DisplacedArgs displaced_args(const Context& ctx, const void* hits) {
    DisplacedArgs d;
    d.hits = static_cast<const float4*>(hits);
    d.table = ctx.displaced.set->table.as<InstanceRecord>();
    d.geomSlots = ctx.displaced.dGeomSlots.as<uint32_t>();
    d.motion = ctx.displaced.set->motion.as<float4>();
    return d;
}

void trace_scene(Context& ctx, hipStream_t stream, const DevAccel* accel, TfdmSet* set, DevBuf& fallbackPlain, int mode, const void* dRayOrgTmin,
                 const void* dRayDirTmax, uint32_t numRays, void* dOut, void* dCounters, void* dShellPart) {
    if (mode != GFX_TRACE_CLOSEST && mode != GFX_TRACE_ANY) throw HipError("gfx_trace_scene: unknown mode");
    if (set) trace_scene_check_set(*set, ctx.device, "gfx_trace_scene");
    if (numRays == 0) return;
    if (!dRayOrgTmin || !dRayDirTmax || !dOut) throw HipError("gfx_trace_scene: null ray or output buffer");
    // rays are read as float4 and a closest hit is written as two float4; an any-hit answer is one uint32
    const bool any = mode == GFX_TRACE_ANY;
    const uintptr_t outMask = any ? 3u : 15u;
    if ((reinterpret_cast<uintptr_t>(dRayOrgTmin) & 15u) || (reinterpret_cast<uintptr_t>(dRayDirTmax) & 15u) || (reinterpret_cast<uintptr_t>(dOut) & outMask))
        throw HipError("gfx_trace_scene: the ray buffers and a closest-hit output must be 16-byte aligned (an any-hit output 4-byte)");
    if (reinterpret_cast<uintptr_t>(dCounters) & 7u) throw HipError("gfx_trace_scene: the counters must be 8-byte aligned");
    if (!any && (reinterpret_cast<uintptr_t>(dShellPart) & 15u)) throw HipError("gfx_trace_scene_ex: the shell part must be 16-byte aligned");
    SceneTrace s;
    s.accel = accel; s.set = set; s.mode = mode;
    s.rayOrgTmin = static_cast<const float4*>(dRayOrgTmin); s.rayDirTmax = static_cast<const float4*>(dRayDirTmax);
    s.numRays = numRays; s.out = dOut; s.statCounters = dCounters;
    s.shellPart = any ? nullptr : dShellPart;
    if (accel && !any) {
        DevBuf& buf = set ? set->plain : fallbackPlain;
        buf.reserve(sizeof(gfx_hit) * static_cast<size_t>(numRays));
        s.plainHits = buf.p;
    }
    trace_scene_launch(ctx, stream, s);
}

} // namespace gfx
