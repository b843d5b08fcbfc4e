// shell_instance.hip.h -- shell-mapped objects as instances of a scene, beside TFDM and NRTDSM ones: the arithmetic shared by
// k_scene_instances_shell (tfdm/tfdm_set.hip), the host side of the instance set and the tests (tests/scene_shell_host.cpp).
// tfdm/tfdm_instance.hip.h has the record, the ray transform, the normal matrix, the world box and the merge rule;
// nrtdsm_instance.hip.h the kind of a record and the NRTDSM step; this header adds the third kind and the step of the merge rule
// that runs shell::trace_ray.
//
// A shell object owns four device arrays and a Params, so it fits the 192-byte InstanceRecord as it is.  Behind a record of kind
// 2 (GFX_INSTANCE_SHELL) the fields carry
//     nodes    the base tree over the per-triangle prism boxes (tfdm::Node[]), as for the other kinds
//     records  nrtdsm::PrismRecord[], the prisms with their tile roots (as behind a record of kind 1)
//     heights  the shell BVH's nodes, tfdm::Node[]     (shell::ShellMap::nodes; there is no height map)
//     pyramid  the shell triangles, shell::ShellTri[]  (shell::ShellMap::tris;  there is no min-max pyramid)
//     params   shell_build.h make_shell_params
// The two repurposed pointers keep their declared types in the record and are cast back here, shell_map(); nothing else reads
// them behind a record of kind 2.
//
// A shell hit has 16 bytes that no other kind has: the shell triangle, its geometry and the tile.  gfx_scene_hit stays 32 bytes;
// those words go to a side record, ShellPart (gfx_scene_shell_part), that is all zeros unless the winning hit is a shell member's.
// A step that accepts a hit of another kind, or the plain phase, leaves it zero: shell_part_none() is what the walk starts from
// and what scene_instance_any_kind puts back when a later member of another kind wins.
//
// The merge rule across kinds is the rule of tfdm_instance.hip.h unchanged: shell::trace_ray accepts only t < tmax and does not
// renormalise the direction (it divides by |dir|^2 where it needs a length), so walking the members in index order, whatever
// their kind, with tmax = the best distance so far gives the closest hit, the plain hit on equal distance, then the lower index.
//
// Under the math contract of tfdm_core.hip.h: plain C++17, no contraction; hipcc and g++ compile it to the same bits.
#pragma once
#include "nrtdsm_instance.hip.h"
#include "shell_core.hip.h"

namespace gfx {
namespace shell {

constexpr uint32_t kKindShell = GFX_INSTANCE_SHELL;

// what only a shell hit has (gfx_scene_shell_part)
struct ShellPart { uint32_t shellTriangle, shellGeom; int32_t tileX, tileY; };
static_assert(sizeof(ShellPart) == 16, "ShellPart is one 16-byte store");

GFX_TFDM_FN ShellPart shell_part_none() {
    ShellPart p;
    p.shellTriangle = 0u; p.shellGeom = 0u; p.tileX = 0; p.tileY = 0;
    return p;
}

GFX_TFDM_FN ShellMap shell_map(const InstanceRecord& r) {
    ShellMap map;
    map.nodes = reinterpret_cast<const Node*>(r.heights);
    map.tris = reinterpret_cast<const ShellTri*>(r.pyramid);
    return map;
}

// One step of the merge rule for a record of kind 2, as nrtdsm::scene_instance_nrtdsm is for kind 1: instance `index` against
// the world ray, accepted only where closer than `best`.  kAny: returns at the first hit and leaves `best` and `part` alone.
// Both stacks are emptied first.
template <bool kAny, class Stack>
GFX_TFDM_FN bool scene_instance_shell(const InstanceRecord& r, uint32_t index, V3 org, V3 dir, float tmin, Stack& stack, Stack& shellStack, SceneHit& best,
                                      ShellPart& part, TraceStats& ts) {
    V3 objOrg, objDir;
    to_object_ray(r, org, dir, objOrg, objDir);
    stack.sp = 0;
    shellStack.sp = 0;
    const ShellMap map = shell_map(r);
    TraceShellHit h;
    if (!trace_ray<kAny>(r.nodes, reinterpret_cast<const PrismRecord*>(r.records), map, r.params, objOrg, objDir, tmin, best.dist, stack, shellStack, h, ts)) return false;
    if (!kAny) {
        best.dist = h.t; best.bcB = h.bcB; best.bcC = h.bcC; best.index = h.prim;
        best.normal = normal_to_world(r, h.normal);
        best.where = (index << 1) | h.frontFace;
        part.shellTriangle = h.tri; part.shellGeom = h.geom; part.tileX = h.tileX; part.tileY = h.tileY;
    }
    return true;
}

// ---------------------------------------------------------------- host
// ... with the step chosen by the record's kind, over all three (k_scene_instances_shell names its own).  The counters of all
// kinds go into one nrtdsm::TraceStats.  A closest hit of another kind clears `part`.
template <bool kAny, class Stack>
inline bool scene_instance_any_kind(const InstanceRecord& r, uint32_t index, V3 org, V3 dir, float tmin, Stack& stack, Stack& shellStack, SceneHit& best, ShellPart& part,
                                    TraceStats& ts) {
    if (nrtdsm::instance_kind(r) == kKindShell) return scene_instance_shell<kAny>(r, index, org, dir, tmin, stack, shellStack, best, part, ts);
    const bool hit = nrtdsm::scene_instance_any_kind<kAny>(r, index, org, dir, tmin, stack, best, ts);
    if (hit && !kAny) part = shell_part_none();
    return hit;
}

// make_instance_of_kind for a shell member: the record of tfdm_instance.hip.h with kind 2 and the shell BVH behind the two
// height-map pointers
inline const char* make_shell_instance(const float objToWorld[12], const Node& root, const Node* nodes, const PrismRecord* records, const Node* shellNodes,
                                       const ShellTri* shellTris, const Params& params, uint32_t userId, InstanceRecord& out) {
    return nrtdsm::make_instance_of_kind(kKindShell, objToWorld, root, nodes, records, reinterpret_cast<const float*>(shellNodes), reinterpret_cast<const F2*>(shellTris),
                                         params, userId, out);
}

} // namespace shell
} // namespace gfx
