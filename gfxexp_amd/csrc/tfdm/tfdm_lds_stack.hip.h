// tfdm_lds_stack.hip.h -- device-only pieces that k_tfdm_trace (tfdm.hip) and k_scene_instances (tfdm_set.hip) share: the
// base-tree stack of tfdm::trace_ray as one LDS column per lane, and the per-wave sum of a counter.
#pragma once
#include <hip/hip_runtime.h>
#include "tfdm_core.hip.h"

namespace gfx {

// [depth][lane] over a block of BLOCK lanes: conflict-free, like bvh8.hip.h's LaneStack.  push() beyond kStackDepth would drop the
// entry; tfdm_core.hip.h asserts that the deepest tree build_tree makes fits
template <int BLOCK>
struct LdsColumnStack {
    uint2* col; int sp;
    __device__ __forceinline__ void push(uint32_t n, float e) { if (sp < tfdm::kStackDepth) { col[sp * BLOCK] = make_uint2(n, tfdm::f2b(e)); ++sp; } }
    __device__ __forceinline__ void pop(uint32_t& n, float& e) { --sp; const uint2 v = col[sp * BLOCK]; n = v.x; e = tfdm::b2f(v.y); }
    __device__ __forceinline__ bool empty() const { return sp == 0; }
};

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

} // namespace gfx
