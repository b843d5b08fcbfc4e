// scene_shell_host.cpp -- the host compilation of gfxexp_amd/csrc/nrtdsm/shell_instance.hip.h behind a C interface
// (tests/scene_shell_host.py compiles it into a directory the test provides), next to tests/scene_nrtdsm_host.cpp for
// nrtdsm_instance.hip.h.  The same text hipcc compiles for k_scene_instances_shell, so the GPU tests compare with it bit for bit.
// Ray transform, normal matrix and world-box test are tfdm_instance.hip.h's and stay behind tests/scene_trace_host.cpp.
#include <cstdint>
#include <cstring>
#include "nrtdsm/shell_instance.hip.h"

using namespace gfx::tfdm;
namespace nr = gfx::nrtdsm;
namespace sh = gfx::shell;

extern "C" {

uint32_t scene_shell_host_sizeof(int what) {
    return what == 0 ? sizeof(InstanceRecord) : what == 1 ? sizeof(gfx_scene_hit) : what == 2 ? sizeof(gfx_hit) : sizeof(gfx_scene_shell_part);
}
uint32_t scene_shell_host_kind(int which) { return which == 2 ? sh::kKindShell : which == 1 ? nr::kKindNrtdsm : nr::kKindTfdm; }

// kind: 0 a TFDM member, 1 an NRTDSM member, 2 a shell member.  ptrs: nodes, records, and heights, pyramid (kinds 0 and 1) or shell
// nodes, shell triangles (kind 2), as 64-bit values (host arrays to trace on the host, device addresses to compare a device
// table).  Returns 0, or 1 with the message in `err`.
int scene_shell_host_make_instance(uint32_t kind, const float objToWorld[12], const Node* root, const uint64_t ptrs[4], const Params* p, uint32_t userId,
                                   InstanceRecord* out, char* err, uint32_t errBytes) {
    const char* e;
    if (kind == sh::kKindShell)
        e = sh::make_shell_instance(objToWorld, *root, reinterpret_cast<const Node*>(ptrs[0]), reinterpret_cast<const nr::PrismRecord*>(ptrs[1]),
                                    reinterpret_cast<const Node*>(ptrs[2]), reinterpret_cast<const sh::ShellTri*>(ptrs[3]), *p, userId, *out);
    else
        e = nr::make_instance_of_kind(kind, objToWorld, *root, reinterpret_cast<const Node*>(ptrs[0]), reinterpret_cast<const void*>(ptrs[1]),
                                      reinterpret_cast<const float*>(ptrs[2]), reinterpret_cast<const F2*>(ptrs[3]), *p, userId, *out);
    if (!e) return 0;
    if (err && errBytes) { std::strncpy(err, e, errBytes - 1); err[errBytes - 1] = 0; }
    return 1;
}

// The instance phase of gfx_trace_scene_ex over three kinds, one ray after the other: all members in index order, each by its kind,
// tmax = the best distance so far.  Arguments as scene_host_trace of tests/scene_trace_host.cpp; shellPart (optional, mode 0):
// gfx_scene_shell_part[n].
void scene_shell_host_trace(const InstanceRecord* table, uint32_t numInstances, const void* plain, int mode, const float* orgTmin, const float* dirTmax, uint32_t n,
                            void* out, gfx_scene_shell_part* shellPart, uint64_t* counters, int cull) {
    for (uint32_t i = 0; i < n; ++i) {
        const V3 org = v3(orgTmin[4 * i], orgTmin[4 * i + 1], orgTmin[4 * i + 2]), dir = v3(dirTmax[4 * i], dirTmax[4 * i + 1], dirTmax[4 * i + 2]);
        const float tmin = orgTmin[4 * i + 3], tmax = dirTmax[4 * i + 3];
        const V3 inv = v3(1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z);
        SceneHit best = scene_miss(tmax);
        sh::ShellPart part = sh::shell_part_none();
        bool occluded = false;
        if (plain) {
            if (mode == 1) occluded = static_cast<const uint32_t*>(plain)[i] != 0u;
            else { const gfx_hit& h = static_cast<const gfx_hit*>(plain)[i]; best = scene_start(tmax, h.dist, h.bcB, h.bcC, h.triIndex); }
        }
        nr::TraceStats ts;
        ts.aabbTests = ts.leafTests = ts.primTests = ts.maxIterations = 0u;
        uint64_t boxTests = 0, traversals = 0;
        HostStack stack, shellStack;
        // an any-hit lane of the kernel is open only with tmax > tmin (tfdm_set.hip): a slot without a ray enters nothing
        const bool open = mode != 1 || best.dist > tmin;
        for (uint32_t k = 0; k < numInstances && open && !occluded; ++k) {
            ++boxTests;
            if (cull && !world_box_hit(table[k], org, inv, tmin, best.dist)) continue;
            ++traversals;
            const bool hit = mode == 1 ? sh::scene_instance_any_kind<true>(table[k], k, org, dir, tmin, stack, shellStack, best, part, ts)
                                       : sh::scene_instance_any_kind<false>(table[k], k, org, dir, tmin, stack, shellStack, best, part, ts);
            if (mode == 1 && hit) occluded = true;
        }
        if (mode == 1) static_cast<uint32_t*>(out)[i] = occluded ? 1u : 0u;
        else {
            gfx_scene_hit h;
            h.dist = best.dist; h.bcB = best.bcB; h.bcC = best.bcC; h.index = best.index;
            h.normal[0] = best.normal.x; h.normal[1] = best.normal.y; h.normal[2] = best.normal.z; h.where = best.where;
            static_cast<gfx_scene_hit*>(out)[i] = h;
            if (shellPart) {
                gfx_scene_shell_part s;
                s.shellTriangle = part.shellTriangle; s.shellGeom = part.shellGeom; s.tile[0] = part.tileX; s.tile[1] = part.tileY;
                shellPart[i] = s;
            }
        }
        if (counters) {
            counters[0] += ts.aabbTests; counters[1] += ts.leafTests; counters[2] += 1u; counters[3] += ts.primTests;
            counters[4] += boxTests; counters[5] += traversals;
        }
    }
}

} // extern "C"
