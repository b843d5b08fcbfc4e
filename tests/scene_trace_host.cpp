// scene_trace_host.cpp -- the host compilation of gfxexp_amd/csrc/tfdm/tfdm_instance.hip.h behind a C interface
// (tests/scene_trace_host.py compiles it into a directory the test provides), next to tests/tfdm_host.cpp for the core.  The same
// text hipcc compiles for k_scene_instances, so the GPU tests compare with it bit for bit.
#include <cstdint>
#include <cstring>
#include "tfdm/tfdm_instance.hip.h"

using namespace gfx::tfdm;

extern "C" {

uint32_t scene_host_sizeof(int what) { return what == 0 ? sizeof(InstanceRecord) : what == 1 ? sizeof(gfx_scene_hit) : sizeof(gfx_hit); }

// ptrs: nodes, records, heights, pyramid as 64-bit values (host arrays to trace on the host, device addresses to compare a
// device table).  Returns 0, or 1 with the message in `err`.
int scene_host_make_instance(const float objToWorld[12], const Node* root, const uint64_t ptrs[4], const Params* p, uint32_t userId, InstanceRecord* out,
                             char* err, uint32_t errBytes) {
    const char* e = make_instance(objToWorld, *root, reinterpret_cast<const Node*>(ptrs[0]), reinterpret_cast<const TriRecord*>(ptrs[1]),
                                  reinterpret_cast<const float*>(ptrs[2]), reinterpret_cast<const F2*>(ptrs[3]), *p, userId, *out);
    if (!e) return 0;
    if (err && errBytes) { std::strncpy(err, e, errBytes - 1); err[errBytes - 1] = 0; }
    return 1;
}

// (origin | tmin, direction | tmax) -> the same layout in object space; tmin and tmax pass through
void scene_host_to_object_rays(const InstanceRecord* r, const float* orgTmin, const float* dirTmax, uint32_t n, float* objOrgTmin, float* objDirTmax) {
    for (uint32_t i = 0; i < n; ++i) {
        V3 o, d;
        to_object_ray(*r, v3(orgTmin[4 * i], orgTmin[4 * i + 1], orgTmin[4 * i + 2]), v3(dirTmax[4 * i], dirTmax[4 * i + 1], dirTmax[4 * i + 2]), o, d);
        objOrgTmin[4 * i] = o.x; objOrgTmin[4 * i + 1] = o.y; objOrgTmin[4 * i + 2] = o.z; objOrgTmin[4 * i + 3] = orgTmin[4 * i + 3];
        objDirTmax[4 * i] = d.x; objDirTmax[4 * i + 1] = d.y; objDirTmax[4 * i + 2] = d.z; objDirTmax[4 * i + 3] = dirTmax[4 * i + 3];
    }
}

void scene_host_normals_to_world(const InstanceRecord* r, const float* normals, uint32_t n, float* out) {
    for (uint32_t i = 0; i < n; ++i) {
        const V3 w = normal_to_world(*r, v3(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]));
        out[3 * i] = w.x; out[3 * i + 1] = w.y; out[3 * i + 2] = w.z;
    }
}

void scene_host_world_box_hits(const InstanceRecord* r, const float* orgTmin, const float* dirTmax, uint32_t n, uint8_t* out) {
    for (uint32_t i = 0; i < n; ++i) {
        const V3 inv = v3(1.0f / dirTmax[4 * i], 1.0f / dirTmax[4 * i + 1], 1.0f / dirTmax[4 * i + 2]);
        out[i] = world_box_hit(*r, v3(orgTmin[4 * i], orgTmin[4 * i + 1], orgTmin[4 * i + 2]), inv, orgTmin[4 * i + 3], dirTmax[4 * i + 3]) ? 1 : 0;
    }
}

// The instance phase of gfx_trace_scene, one ray after the other.  `plain` (optional): what the plain phase found, gfx_hit[n]
// (mode 0) or uint32[n] (mode 1).  mode 0: out = gfx_scene_hit[n]; mode 1: uint32[n].  cull = 0: every instance is traversed
// whatever its world box says.  counters (optional): u64[8], added to.
void scene_host_trace(const InstanceRecord* table, uint32_t numInstances, const void* plain, int mode, const float* orgTmin, const float* dirTmax, uint32_t n,
                      void* out, uint64_t* counters, int cull) {
    for (uint32_t i = 0; i < n; ++i) {
        const V3 org = v3(orgTmin[4 * i], orgTmin[4 * i + 1], orgTmin[4 * i + 2]), dir = v3(dirTmax[4 * i], dirTmax[4 * i + 1], dirTmax[4 * i + 2]);
        const float tmin = orgTmin[4 * i + 3], tmax = dirTmax[4 * i + 3];
        const V3 inv = v3(1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z);
        SceneHit best = scene_miss(tmax);
        bool occluded = false;
        if (plain) {
            if (mode == 1) occluded = static_cast<const uint32_t*>(plain)[i] != 0u;
            else { const gfx_hit& h = static_cast<const gfx_hit*>(plain)[i]; best = scene_start(tmax, h.dist, h.bcB, h.bcC, h.triIndex); }
        }
        TraceStats ts;
        ts.aabbTests = ts.leafTests = ts.primTests = 0u;
        uint64_t boxTests = 0, traversals = 0;
        HostStack stack;
        for (uint32_t k = 0; k < numInstances && !occluded; ++k) {
            ++boxTests;
            if (cull && !world_box_hit(table[k], org, inv, tmin, best.dist)) continue;
            ++traversals;
            const bool hit = mode == 1 ? scene_instance<true>(table[k], k, org, dir, tmin, stack, best, ts) : scene_instance<false>(table[k], k, org, dir, tmin, stack, best, ts);
            if (mode == 1 && hit) occluded = true;
        }
        if (mode == 1) static_cast<uint32_t*>(out)[i] = occluded ? 1u : 0u;
        else {
            gfx_scene_hit h;
            h.dist = best.dist; h.bcB = best.bcB; h.bcC = best.bcC; h.index = best.index;
            h.normal[0] = best.normal.x; h.normal[1] = best.normal.y; h.normal[2] = best.normal.z; h.where = best.where;
            static_cast<gfx_scene_hit*>(out)[i] = h;
        }
        if (counters) {
            counters[0] += ts.aabbTests; counters[1] += ts.leafTests; counters[2] += 1u; counters[3] += ts.primTests;
            counters[4] += boxTests; counters[5] += traversals;
        }
    }
}

} // extern "C"
