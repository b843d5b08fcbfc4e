// tfdm_set.h -- host-side state of a set of displaced instances and the scene-level ray query (tfdm_set.hip) behind
// gfx_tfdm_set_* and gfx_trace_scene.
#pragma once
#include "tfdm.h"
#include "../nrtdsm/nrtdsm.h"
#include "../nrtdsm/shell.h"
#include "../nrtdsm/shell_instance.hip.h"

namespace gfx {

struct TfdmSet {
    int device = 0;
    struct Member {
        DisplacedObject* obj;       // not owned: objects outlive the set.  A TfdmObject, an NrtdsmObject or a ShellObject, by `kind`
        uint32_t kind;              // GFX_INSTANCE_TFDM / _NRTDSM / _SHELL: the kind word of the member's record (nrtdsm_instance.hip.h)
        float objToWorld[12];
        float prevObjToWorld[12];   // where the instance was: the transform tfdm_set_move replaced (add and tfdm_set_transform: objToWorld)
        uint32_t userId;
        uint64_t generation;        // the object's generation the committed record was made from
    };
    std::vector<Member> members;
    bool dirty = false;             // an add, a transform or a move since the last commit
    std::vector<tfdm::InstanceRecord> host;   // the committed table
    std::vector<float> hostMotion;  // the committed motion table: curToPrev[12] per member (tfdm_instance.hip.h make_cur_to_prev)
    bool anyBilinear = false;       // ... has a member of GFX_TFDM_BILINEAR: the instance phase launches the instantiation that can run it
    bool anyNrtdsm = false;         // ... has an NRTDSM member: the instance phase is k_scene_instances_mixed
    bool anyShell = false;          // ... has a shell member: the instance phase is k_scene_instances_shell, whatever else the set holds
    DevBuf table;                   // InstanceRecord[members]
    DevBuf motion;                  // float4[3 * members], the motion table: committed together with `table`
    DevBuf plain;                   // gfx_hit[numRays] of the plain phase of a closest-hit query; grows on demand
};

uint32_t tfdm_set_add(TfdmSet& s, TfdmObject* obj, const float objToWorld[12], uint32_t userId);
uint32_t tfdm_set_add_nrtdsm(TfdmSet& s, NrtdsmObject* obj, const float objToWorld[12], uint32_t userId);   // indices count all kinds
uint32_t tfdm_set_add_shell(TfdmSet& s, ShellObject* obj, const float objToWorld[12], uint32_t userId);
void tfdm_set_transform(TfdmSet& s, uint32_t index, const float objToWorld[12]);   // the teleport: prev <- cur <- objToWorld
void tfdm_set_move(TfdmSet& s, uint32_t index, const float objToWorld[12]);        // prev <- cur, cur <- objToWorld
void tfdm_set_commit(TfdmSet& s, hipStream_t stream);
void tfdm_set_read(TfdmSet& s, void* hostOut, size_t bytes);
void tfdm_set_read_motion(TfdmSet& s, void* hostOut, size_t bytes);
void tfdm_set_bounds(const TfdmSet& s, float lo[3], float hi[3]);   // union of the committed records' world boxes (host table)
void tfdm_set_release(TfdmSet& s);
// The scene query as the passes launch it (restir.hip, pathtrace.hip).  The ray count may be a device word (numRaysPtr; numRays is
// then the queue capacity: k_scene_instances launches over it and the waves beyond the count leave at once), as TraceLaunch's is for
// k_trace, so a bounce loop needs no host read-back.  spill / counters / zeroWords / hintFromOut go to the plain phase's TraceLaunch
// unchanged.  plainHits: gfx_hit[numRays] the plain phase of a closest-hit query writes and the instance phase widens -- the caller's,
// so that two queries in flight on two streams never share one.
struct SceneTrace {
    const DevAccel* accel = nullptr;
    TfdmSet* set = nullptr;
    int mode = 0;
    const float4* rayOrgTmin = nullptr; const float4* rayDirTmax = nullptr;
    uint32_t numRays = 0; const uint32_t* numRaysPtr = nullptr;
    void* out = nullptr;
    void* plainHits = nullptr;
    void* statCounters = nullptr;       // u64[8] of gfx_trace_scene, optional
    void* shellPart = nullptr;          // gfx_scene_shell_part[numRays] of gfx_trace_scene_ex, optional: closest hits of a set with a shell member
    DevBuf* spill = nullptr; DevBuf* counters = nullptr;
    uint32_t* zeroWords[2] = { nullptr, nullptr };
    bool hintFromOut = false;           // plainHits still holds the previous launch's plain hits for the same rays
};
void trace_scene_launch(Context& ctx, hipStream_t stream, const SceneTrace& t);
void trace_scene_check_set(const TfdmSet& set, int device, const char* who);   // throws: foreign device, uncommitted change, stale member

// what the set-bound passes read of a displaced hit: gfx_scene_hit[] as two float4 per entry, the committed instance table, the
// geometry each instance is shaded with (Context::displaced) and the committed motion table (three float4 per instance: the rows
// of curToPrev; only the G-buffer pass reads it)
struct DisplacedArgs { const float4* hits; const tfdm::InstanceRecord* table; const uint32_t* geomSlots; const float4* motion; };

// gfx_scene_bind_displaced_passes (set == nullptr: unbind; passMask: GFX_DISPLACED_*, the G-buffer pass and the path tracer are
// always in it) and the check every set-bound launch repeats: the set as gfx_trace_scene wants it, and no bound geometry's material
// emitting (a material may have been set after the bind).
void displaced_bind(Context& ctx, TfdmSet* set, const uint32_t* geomSlots, uint32_t n, uint32_t passMask);
void displaced_check(Context& ctx, const char* who);
DisplacedArgs displaced_args(const Context& ctx, const void* hits);
// gfx_scene_bind_displaced_kinds: the binding that renders NRTDSM and shell members too.  displaced_check
// knows which of the two calls made the binding.  The shell-aware siblings of the three set-bound kernels take, next to
// DisplacedArgs, the shell part of every hit (one 16-byte gfx_scene_shell_part beside each gfx_scene_hit) and the material table;
// they run only while displaced_shell_render(ctx): a kinds binding whose committed set has a shell member.
void displaced_bind_kinds(Context& ctx, TfdmSet* set, const gfx_displaced_member* members, uint32_t n, uint32_t passMask);
struct DisplacedShellArgs { const float4* shellPart; const uint32_t* shellMats; };
bool displaced_shell_render(const Context& ctx);
DisplacedShellArgs displaced_shell_args(const Context& ctx, const void* shellPart);
void restir_primary_rays(Context& ctx, hipStream_t stream, uint32_t width, uint32_t height, void* dRayOrgTmin, void* dRayDirTmax);   // restir.hip
// gfx_restir_last_rays: the queue and the occlusion words of the last ray pass that ran in its three-kernel form (restir.hip)
void restir_last_rays(Context& ctx, hipStream_t stream, void* dRayOrgTmin, void* dRayDirTmax, void* dOccluded, uint32_t capacity, uint32_t* count);
// gfx_pt_last_nee_rays: the same for the last any-hit pass of a path tracer's wavefront form, with the owning pixels (pathtrace.hip)
void pt_last_nee_rays(Context& ctx, hipStream_t stream, void* dRayOrgTmin, void* dRayDirTmax, void* dOccluded, void* dOwnerPixel, uint32_t capacity, uint32_t* count);

// set == nullptr: no displaced instances; accel == nullptr: no plain geometry.  `fallbackPlain`: the plain-phase buffer of a
// closest-hit query without a set (the context's).
void trace_scene(Context& ctx, hipStream_t stream, const DevAccel* accel, TfdmSet* set, DevBuf& fallbackPlain, int mode, const void* dRayOrgTmin,
                 const void* dRayDirTmax, uint32_t numRays, void* dOut, void* dCounters, void* dShellPart = nullptr);

} // namespace gfx
