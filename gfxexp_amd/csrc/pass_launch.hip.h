// pass_launch.hip.h -- the launch plumbing the pass sequencers share (restir_launch, pathtrace_launch): one kernel under its timer,
// one cost-ordered launch, one ray queue traced through the BVH8 or -- when a displaced set is in play -- the scene query.
#pragma once
#include "internal.h"
#include "restir_common.hip.h"
#include "tfdm/tfdm_set.h"

namespace gfx {

// One kernel launch on `stream` with the launch error checked ...
template <typename K, typename... Args>
inline void launch_checked(hipStream_t stream, K kernel, dim3 grid, dim3 block, const Args&... args) {
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, args...);
    GFX_HIP(hipGetLastError());
}
// ... and under the timer `name` (gfx_timing_collect).
template <typename K, typename... Args>
inline void launch_timed(Context& ctx, hipStream_t stream, const char* name, K kernel, dim3 grid, dim3 block, const Args&... args) {
    ScopedKernelTimer timer(ctx, stream, name);
    launch_checked(stream, kernel, grid, block, args...);
}

// A launch whose blocks start in the cost order of the launch before it (block_order_begin / _end, restir.hip).  `which`: the
// Context::blockOrders slot; `key`: the launch shape the order belongs to.  px.order is set for the launch; `launch(cost)` makes it
// (launch_timed with the kernel's arguments, `cost` among them: null when the launch takes no part).
template <typename Launch>
inline void launch_cost_ordered(Context& ctx, hipStream_t stream, int which, uint32_t blocks, uint64_t key, uint32_t minBlocks, PixelGrid& px, Launch launch) {
    const uint32_t* order = nullptr;
    uint32_t* cost = nullptr;
    block_order_begin(ctx, stream, which, blocks, key, minBlocks, order, cost);
    px.order = order;
    launch(cost);
    block_order_end(ctx, stream, which, blocks, cost);
}

// One ray queue traced: `q` describes it as a scene query would be (tfdm/tfdm_set.h SceneTrace; numRays: the count, or with numRaysPtr the
// queue's capacity; accel and set are filled in here).  Through the scene query over the bound set when `scene` -- the caller's own
// condition for "the set is in play" -- else through trace_launch, which has no use for plainHits and shellPart.
inline void trace_ray_queue(Context& ctx, hipStream_t stream, const DevAccel& accel, bool scene, SceneTrace q) {
    if (scene) {
        q.accel = &accel; q.set = ctx.displaced.set;
        trace_scene_launch(ctx, stream, q);
        return;
    }
    TraceLaunch t;
    t.accel = accel; t.rayOrgTmin = q.rayOrgTmin; t.rayDirTmax = q.rayDirTmax;
    t.numRays = q.numRaysPtr ? 0u : q.numRays; t.numRaysPtr = q.numRaysPtr;     // (k_trace reads the count from the device and needs no capacity)
    t.out = q.out; t.mode = q.mode;
    t.spill = q.spill; t.counters = q.counters;
    t.zeroWords[0] = q.zeroWords[0]; t.zeroWords[1] = q.zeroWords[1];
    t.hintFromOut = q.hintFromOut;
    trace_launch(ctx, stream, t);
}

} // namespace gfx
