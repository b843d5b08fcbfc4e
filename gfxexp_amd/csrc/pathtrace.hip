// pathtrace.hip -- the baseline unidirectional path tracer as a wavefront pipeline.
//
// The reference runs one OptiX ray-generation megakernel per pixel that loops over path vertices,
// tracing a shadow ray (NEE) and an extension ray per vertex inline
// (path_tracing/gpu_kernels/optix_pathtracing_kernels.cu:18-341).  Here a frame is
//
//   k_pt_first                     first-hit shading from the G-buffer: NEE ray + extension ray
//   repeat for pathLength = 2..max(2, maxPathLength):
//     trace any   (NEE queue)      -> k_pt_apply_nee   contribution += alpha * NEE  (if unoccluded)
//     trace closest (ext queue)    -> k_pt_bounce      closest-hit / miss program of that vertex
//   k_pt_finish                    running mean into the beauty buffer
//
// Both ray queues are dense (ballot/popcount compaction, one atomic per wave) and shrink every
// bounce; every launch covers the queue capacity and reads the live count from the device, so the
// whole frame is enqueued without a host sync.  Per-path arithmetic, RNG draw order and the order
// of the floating-point adds into `contribution` are those of the reference, so the beauty buffer
// and the RNG states match the CPU restatement (oracle/orc_pathtrace.h) bit for bit.
//
// ReGIR (regir/gpu_kernels/build_cell_reservoirs.cu, regir/gpu_kernels/optix_pathtracing_kernels.cu)
// reuses the same pipeline with REGIR = true: NEE resamples the light-slot reservoirs of the grid cell
// under the shading point, Russian roulette moves to the loop head, and three small kernels maintain
// the grid: k_regir_build<temporal>, k_regir_update_last_access.
//
// One translation unit, cut by concern: regir.hip.h (PtArgs, ReGIR), pt_vertex.hip.h (one path vertex),
// pt_scene.hip.h (a bound displaced set), nrc_render.hip.h (NRC); here the baseline and one-kernel tracers and the host sequencing.
#include <cstring>
#include "pt_vertex.hip.h"
#include "regir.hip.h"
#include "pt_scene.hip.h"
#include "nrc_render.hip.h"
#include "pass_launch.hip.h"

namespace gfx {

// pathTrace_rayGen_generic up to the path extension loop, through the queues: the first vertex of every pixel of the band
template <bool REGIR>
__global__ __launch_bounds__(kPtBlock) void k_pt_first(PtArgs a) {
    const PixelId px = pixel_of_thread(a.px);
    const size_t p = px.p;
    PtPath path;
    const bool surface = pt_first_vertex<REGIR>(a, px, path);
    if (surface) static_cast<uint64_t*>(a.s.rngBuffer)[p] = path.rng.state;
    if (px.valid) {
        a.state[2 * p] = make_float4(path.alpha.x, path.alpha.y, path.alpha.z, path.dirPDensity);
        a.state[2 * p + 1] = make_float4(path.contribution.x, path.contribution.y, path.contribution.z, 0.0f);
    }
    push_vertex(a, static_cast<uint32_t>(p), path.pos, path.o);
}

// The visibility factor of performDirectLighting<.., true> applied after the any-hit trace:
// contribution += alpha * NEE  (optix_pathtracing_kernels.cu:136-137, :279-280)
__global__ __launch_bounds__(kPtBlock) void k_pt_apply_nee(PtArgs a) {
    const uint32_t i = blockIdx.x * kPtBlock + threadIdx.x;
    if (i >= *a.neeCount) return;
    const float4 pend = a.neePending[i];
    const uint32_t pixel = f2bits(pend.w);
    f3 add(pend.x, pend.y, pend.z);
    if (a.occluded[i]) {
        add = add * 0.0f;                     // alpha * RGB(0): zero unless the throughput is not finite
        if (a.neeTrainIdx) {                  // NRC: the record's initial target is the SHADOWED estimate
            const uint32_t t = a.neeTrainIdx[i];
            if (t != 0x007FFFFFu) {
                float* tgt = static_cast<float*>(a.nrc.trainTargetBuffer[0]) + 3ull * t;
                tgt[0] = 0.0f; tgt[1] = 0.0f; tgt[2] = 0.0f;
            }
        }
    }
    float4* c = a.state + 2ull * pixel + 1;
    const float4 cur = *c;
    *c = make_float4(cur.x + add.x, cur.y + add.y, cur.z + add.z, 0.0f);
}

// One extension-queue entry: what its ray found and the vertex it reached (pt_next_vertex), the path's state back to its pixel
template <bool REGIR>
__global__ __launch_bounds__(kPtBlock) void k_pt_bounce(PtArgs a) {
    const uint32_t i = blockIdx.x * kPtBlock + threadIdx.x;
    const uint32_t count = *a.extCountIn;
    PtPath path;
    path.alpha = f3(0.0f); path.contribution = f3(0.0f); path.dirPDensity = 0.0f; path.rng.state = 0;
    uint32_t pixel = 0;
    gfx_hit h; h.dist = 0.0f; h.bcB = 0.0f; h.bcC = 0.0f; h.triIndex = GFX_INVALID_SLOT;
    f3 rayOrg(0.0f), rayDir(0.0f);
    const bool active = i < count;
    if (active) {
        pixel = a.extOwnerIn[i];
        h = a.hits[i];
        const float4 ro4 = a.extOrgIn[i], rd4 = a.extDirIn[i];
        rayOrg = f3(ro4.x, ro4.y, ro4.z); rayDir = f3(rd4.x, rd4.y, rd4.z);
        const float4 s0 = a.state[2ull * pixel], s1 = a.state[2ull * pixel + 1];
        path.alpha = f3(s0.x, s0.y, s0.z);
        path.dirPDensity = s0.w;
        path.contribution = f3(s1.x, s1.y, s1.z);
    }
    const uint32_t what = pt_next_vertex<REGIR>(a, active, h, rayOrg, rayDir, static_cast<const uint64_t*>(a.s.rngBuffer) + pixel, path);
    if (what & kPtHitSurface) {
        static_cast<uint64_t*>(a.s.rngBuffer)[pixel] = path.rng.state;
        a.state[2ull * pixel] = make_float4(path.alpha.x, path.alpha.y, path.alpha.z, path.dirPDensity);
    }
    if (what & (kPtHitSurface | kPtMissAdded)) a.state[2ull * pixel + 1] = make_float4(path.contribution.x, path.contribution.y, path.contribution.z, 0.0f);
    push_vertex(a, pixel, path.pos, path.o);
}

// running mean (optix_pathtracing_kernels.cu:203-208)
__global__ __launch_bounds__(kPtBlock) void k_pt_finish(PtArgs a) {
    const PixelId px = pixel_of_thread(a.px);
    if (!px.valid) return;
    const size_t p = px.p;
    const float4 c = a.state[2 * p + 1];
    const f3 contribution(c.x, c.y, c.z);
    float4* beauty = static_cast<float4*>(a.s.beautyAccumBuffer) + p;
    f3 prev(0.0f);
    if (a.f.numAccumFrames > 0) { const float4 b = *beauty; prev = f3(b.x, b.y, b.z); }
    const float curWeight = 1.0f / (1 + a.f.numAccumFrames);
    const f3 result = (1 - curWeight) * prev + curWeight * contribution;
    *beauty = make_float4(result.x, result.y, result.z, 1.0f);
}

// The whole path of a pixel in ONE kernel, for small launches (trace_local.hip.h): first vertex, then per further vertex the NEE ray
// (any hit), its visibility applied, the extension ray (closest hit), the next vertex -- what k_pt_first, the two k_trace launches,
// k_pt_apply_nee, k_pt_bounce and k_pt_finish do through queues, here in the registers of the pixel's lane, in the same order per pixel
// (so the same sums).  A 512 x 512 frame is one round of waves; its wavefront form is ~20 launches of which most last as long as their
// slowest wave.  A lane whose path has ended idles until its wave's longest path has (no compaction: that is the price, and why large
// launches keep the wavefront form).
template <bool REGIR>
__global__ __launch_bounds__(kPtBlock) void k_pt_fused(PtArgs a, DevAccel accel, uint2* spill, int spillCap, uint32_t maxPathLength, uint32_t* __restrict__ blockCost,
                                                       unsigned long long* __restrict__ diag) {
    __shared__ uint2 ldsStack[kLdsStackDepth * kPtBlock];
    __shared__ __attribute__((aligned(16))) uint4 fetchBuf[(kPtBlock / 64) * 256];
    const int tid = threadIdx.x, lane = tid & 63;
    uint4* waveBuf = fetchBuf + 256 * __builtin_amdgcn_readfirstlane(tid >> 6);
    uint2* stackLds = ldsStack + tid;
    uint2* stackSpill = spill + (static_cast<size_t>(blockIdx.x) * kPtBlock + tid) * spillCap;
    const PixelId px = pixel_of_thread(a.px);                   // (a.px.order: the blocks whose paths took most steps one frame ago start first)
    uint32_t steps = 0, totalSteps = 0;
    uint32_t diagIterations = 0, diagLanes = 0;                 // "pt_diag": bounce iterations of the wave, lanes that held a ray in them
    PtPath path;
    bool rngMoved = pt_first_vertex<REGIR>(a, px, path);       // a.pathLength = 1 (set by the host)
    for (uint32_t pathLength = 2;; ++pathLength) {
        if (diag) { ++diagIterations; diagLanes += static_cast<uint32_t>(__popcll(__ballot(path.o.wantNee || path.o.wantExt))); }
        const RayHit shadow = trace_wave_local<true>(accel, path.o.wantNee, path.o.neeFromOrg ? path.o.neeOrg : path.pos, path.o.neeDir, 0.0f, path.o.neeTmax,
                                                     stackLds, kPtBlock, stackSpill, spillCap, waveBuf, lane, 0xFFFFFFFFu, &steps);
        totalSteps += steps;
        if (path.o.wantNee) {                                   // k_pt_apply_nee
            f3 add = path.o.pending;
            if (shadow.tri != GFX_INVALID_SLOT) add = add * 0.0f;
            path.contribution = path.contribution + add;
        }
        if (REGIR && pathLength >= maxPathLength) break;
        if (__ballot(path.o.wantExt) == 0ull) break;            // no path of the wave goes on: nothing further can be added
        const bool extend = path.o.wantExt;
        const f3 rayOrg = path.pos, rayDir = path.o.extDir;
        const RayHit hit = trace_wave_local<false>(accel, extend, rayOrg, rayDir, 0.0f, 3.402823466e+38f, stackLds, kPtBlock, stackSpill, spillCap, waveBuf, lane, 0xFFFFFFFFu, &steps);
        totalSteps += steps;
        gfx_hit h; h.dist = hit.t; h.bcB = hit.bcB; h.bcC = hit.bcC; h.triIndex = hit.tri;
        const bool lastVertex = pathLength >= maxPathLength;     // what the host sets per bounce launch in the wavefront form
        if (pt_next_vertex<REGIR>(a, extend, h, rayOrg, rayDir, nullptr, path, lastVertex ? 1 : 0, pathLength + 1 >= maxPathLength ? 1 : 0) & kPtHitSurface) rngMoved = true;
        if (!REGIR && lastVertex) break;
    }
    if (blockCost && lane == 0) atomicMax(blockCost + launch_block(a.px), totalSteps >> 1);    // (<= 255 after the sort's clamp: 510 steps)
    if (diag && lane == 0) { atomicAdd(diag, diagIterations); atomicAdd(diag + 1, diagLanes); atomicAdd(diag + 2, totalSteps); atomicAdd(diag + 3, 1ull); }
    if (!px.valid) return;
    const size_t p = px.p;
    if (rngMoved) static_cast<uint64_t*>(a.s.rngBuffer)[p] = path.rng.state;
    float4* beauty = static_cast<float4*>(a.s.beautyAccumBuffer) + p;          // k_pt_finish
    f3 prev(0.0f);
    if (a.f.numAccumFrames > 0) { const float4 bb = *beauty; prev = f3(bb.x, bb.y, bb.z); }
    const float curWeight = 1.0f / (1 + a.f.numAccumFrames);
    const f3 result = (1 - curWeight) * prev + curWeight * path.contribution;
    *beauty = make_float4(result.x, result.y, result.z, 1.0f);
}

// k_pt_fused with path regeneration.  In k_pt_fused a lane whose path has ended idles until the longest path of its wave has: 0.30
// lanes per instruction on the 512 x 512 bunny frame (profiles/r05_pmc_config1.json: most pixels miss or end after one or two vertices,
// a few run to the length limit).  Here the launch is the waves the GPU holds at once, and a lane whose path has ended writes its pixel
// and draws the next launch slot from a ticket counter (one wave-aggregated atomic per refill), takes that pixel's first vertex from
// the G-buffer and joins the wave's next trace: the wave keeps full lanes until the ticket runs out.  A pixel's path is the same
// sequence of operations on the same RNG stream whichever lane runs it and whenever: the frame is bit-identical to k_pt_fused's.
// Baseline path tracer only (the ReGIR tracer merges its cell-access atomics across lanes that are at the same vertex).
__global__ __launch_bounds__(kPtBlock) void k_pt_regen(PtArgs a, DevAccel accel, uint2* spill, int spillCap, uint32_t maxPathLength,
                                                       uint32_t* __restrict__ ticket, uint32_t numSlots, int minRefill, unsigned long long* __restrict__ diag) {
    __shared__ uint2 ldsStack[kLdsStackDepth * kPtBlock];
    __shared__ __attribute__((aligned(16))) uint4 fetchBuf[(kPtBlock / 64) * 256];
    const int tid = threadIdx.x, lane = tid & 63;
    uint4* waveBuf = fetchBuf + 256 * __builtin_amdgcn_readfirstlane(tid >> 6);
    uint2* stackLds = ldsStack + tid;
    uint2* stackSpill = spill + (static_cast<size_t>(blockIdx.x) * kPtBlock + tid) * spillCap;
    PixelId px; px.p = 0; px.x = 0; px.y = 0; px.slot = 0; px.valid = false;
    PtPath path;
    reset_vertex_out(path.o);
    path.alpha = f3(0.0f); path.contribution = f3(0.0f); path.dirPDensity = 0.0f; path.rng.state = 0; path.pos = f3(0.0f);
    bool active = false, rngMoved = false, exhausted = false;
    uint32_t pathLength = 2;
    uint32_t diagIterations = 0, diagLanes = 0, diagSteps = 0, diagRefills = 0, steps = 0;
    auto finish = [&]() {                                       // the pixel's RNG state and its running mean (k_pt_finish)
        if (px.valid) {
            const size_t p = px.p;
            if (rngMoved) static_cast<uint64_t*>(a.s.rngBuffer)[p] = path.rng.state;
            float4* beauty = static_cast<float4*>(a.s.beautyAccumBuffer) + p;
            f3 prev(0.0f);
            if (a.f.numAccumFrames > 0) { const float4 bb = *beauty; prev = f3(bb.x, bb.y, bb.z); }
            const float curWeight = 1.0f / (1 + a.f.numAccumFrames);
            const f3 result = (1 - curWeight) * prev + curWeight * path.contribution;
            *beauty = make_float4(result.x, result.y, result.z, 1.0f);
        }
        active = false;
    };
    const EnvMap env = load_env(a.s);
    const bool envEnabled = env.present() && a.f.enableEnvLight;
    for (;;) {
        // ---- the rays of the vertices the lanes stand on: NEE (any hit), its visibility applied, then the extension (closest hit)
        PtSetup su;                                             // the vertex a lane shades at the end of this iteration
        if (__ballot(active) != 0ull) {
            if (diag) { ++diagIterations; diagLanes += static_cast<uint32_t>(__popcll(__ballot(active))); }
            const bool nee = active && path.o.wantNee;
            const RayHit shadow = trace_wave_local<true>(accel, nee, path.o.neeFromOrg ? path.o.neeOrg : path.pos, path.o.neeDir, 0.0f, path.o.neeTmax,
                                                         stackLds, kPtBlock, stackSpill, spillCap, waveBuf, lane, 0xFFFFFFFFu, &steps);
            diagSteps += steps;
            if (nee) {                                          // k_pt_apply_nee
                f3 add = path.o.pending;
                if (shadow.tri != GFX_INVALID_SLOT) add = add * 0.0f;
                path.contribution = path.contribution + add;
            }
            bool done = active && !path.o.wantExt;
            const bool extend = active && path.o.wantExt;
            if (__ballot(extend) != 0ull) {
                const f3 rayOrg = path.pos, rayDir = path.o.extDir;
                const RayHit hit = trace_wave_local<false>(accel, extend, rayOrg, rayDir, 0.0f, 3.402823466e+38f, stackLds, kPtBlock, stackSpill, spillCap, waveBuf, lane, 0xFFFFFFFFu, &steps);
                diagSteps += steps;
                if (extend) {                                   // what the ray found: implicit light with MIS, Russian roulette, the next surface point
                    gfx_hit h; h.dist = hit.t; h.bcB = hit.bcB; h.bcC = hit.bcC; h.triIndex = hit.tri;
                    const bool lastVertex = pathLength >= maxPathLength;
                    if (pt_next_setup<false>(a, true, h, rayOrg, rayDir, nullptr, path, su, lastVertex ? 1 : 0) & kPtHitSurface) rngMoved = true;
                    if (lastVertex || !su.shade) done = true;   // (a path that is not shaded asks for no ray: it has ended)
                    ++pathLength;
                }
            }
            if (done) finish();
        }
        // ---- refill: when at least `minRefill` lanes are idle (or all of them), the idle lanes draw launch slots -- one wave-aggregated
        // atomic -- and set their pixel's first vertex up from the G-buffer.  A pixel without a surface (background) is finished on the spot
        // and its lane draws again, up to four times per refill.
#pragma nounroll
        for (int round = 0; round < 4 && !exhausted; ++round) {
            const unsigned long long need = __ballot(!active);
            const int idle = __popcll(need);
            if (idle == 0 || (idle < minRefill && idle < 64 && round == 0)) break;
            const uint32_t count = static_cast<uint32_t>(idle);
            ++diagRefills;
            uint32_t base = 0;
            if (lane == __builtin_ctzll(need)) base = atomicAdd(ticket, count);
            base = __shfl(base, __builtin_ctzll(need));
            if (!active) {
                const uint32_t slot = base + static_cast<uint32_t>(__popcll(need & ((1ull << lane) - 1ull)));
                if (slot < numSlots) {
                    px = pixel_of_block_thread(a.px, slot >> 8, slot & 255u);      // (kPtBlock = 256 slots per launch block)
                    rngMoved = pt_first_setup<false>(a, px, path, su);
                    pathLength = 2;
                    active = true;
                    if (!su.shade) finish();                    // nothing to shade: no ray will be asked for
                }
            }
            exhausted = base + count >= numSlots;
        }
        if (__ballot(active) == 0ull) { if (exhausted) break; else continue; }
        // ---- ONE shading step for the wave: the vertices the extension rays reached and the first vertices of the pixels just drawn
        // (light sample + MIS + BSDF sample: the code a wave executes once per iteration whichever lanes take part)
        shade_vertex<false>(a, active && su.shade, env, envEnabled, path.pos, su.vOutLocal, su.frame, su.bsdf, path.rng, path.alpha, path.contribution, path.dirPDensity, path.o);
    }
    if (diag && lane == 0) { atomicAdd(diag, diagIterations); atomicAdd(diag + 1, diagLanes); atomicAdd(diag + 2, diagSteps); atomicAdd(diag + 3, 1ull); atomicAdd(diag + 4, diagRefills); }
}

// ---------------------------------------------------------------- gfx_pt_last_nee_rays
// the owner pixel of every NEE queue entry: the w word of its pending record
__global__ __launch_bounds__(kPtBlock) void k_pt_nee_owners(const float4* __restrict__ pending, uint32_t n, uint32_t* __restrict__ owners) {
    const uint32_t i = blockIdx.x * kPtBlock + threadIdx.x;
    if (i < n) owners[i] = f2bits(pending[i].w);
}
void pt_last_nee_rays(Context& ctx, hipStream_t stream, void* dRayOrgTmin, void* dRayDirTmax, void* dOccluded, void* dOwnerPixel, uint32_t capacity, uint32_t* count) {
    const Context::LastNee& last = ctx.lastNee;
    if (!count) throw HipError("gfx_pt_last_nee_rays: null count");
    if (last.state == 0) throw HipError("gfx_pt_last_nee_rays: no NEE pass has run yet");
    if (last.state == 2) throw HipError("gfx_pt_last_nee_rays: the last path-tracing launch ran fused (one kernel, no ray queue); \"fuse_passes\" 1 keeps the wavefront form");
    if ((reinterpret_cast<uintptr_t>(dRayOrgTmin) | reinterpret_cast<uintptr_t>(dRayDirTmax)) & 15u) throw HipError("gfx_pt_last_nee_rays: the ray outputs must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(dOccluded) | reinterpret_cast<uintptr_t>(dOwnerPixel)) & 3u) throw HipError("gfx_pt_last_nee_rays: the occlusion and owner outputs must be 4-byte aligned");
    if (last.org != ctx.rayOrg.p || last.dir != ctx.rayDir.p || last.out != ctx.rayOut.p || last.pending != ctx.ptPending.p)
        throw HipError("gfx_pt_last_nee_rays: the NEE queue was reallocated for a larger launch since the last NEE pass");
    uint32_t n = 0;                              // the device count, once the launch is through (its streams are joined on `stream`)
    GFX_HIP(hipMemcpyAsync(&n, last.countPtr, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    GFX_HIP(hipStreamSynchronize(stream));
    *count = n;
    if (n > capacity) throw HipError("gfx_pt_last_nee_rays: the pass traced " + std::to_string(n) + " queue entries, capacity is " + std::to_string(capacity));
    if (n == 0) return;
    if (!dRayOrgTmin || !dRayDirTmax || !dOccluded) throw HipError("gfx_pt_last_nee_rays: null output");
    GFX_HIP(hipMemcpyAsync(dRayOrgTmin, last.org, 16 * static_cast<size_t>(n), hipMemcpyDeviceToDevice, stream));
    GFX_HIP(hipMemcpyAsync(dRayDirTmax, last.dir, 16 * static_cast<size_t>(n), hipMemcpyDeviceToDevice, stream));
    GFX_HIP(hipMemcpyAsync(dOccluded, last.out, 4 * static_cast<size_t>(n), hipMemcpyDeviceToDevice, stream));
    if (dOwnerPixel)
        launch_checked(stream, k_pt_nee_owners, dim3((n + kPtBlock - 1) / kPtBlock), dim3(kPtBlock), static_cast<const float4*>(last.pending), n, static_cast<uint32_t*>(dOwnerPixel));
}

// ---------------------------------------------------------------- host sequencing
// gfx_pt_launch in parts: what the pass is and whether it may run (pt_classify), the small NRC passes, the ReGIR grid passes, and for a
// tracer its buffers and PtArgs (pt_prepare), then the one-kernel form (pt_launch_one_kernel) or the wavefront loop (pt_launch_wavefront).
struct PtPass {
    bool displaced;               // a displaced-instance set is bound: the traces are the scene query (any binding)
    bool regirPass, nrcPass;      // the pass reads the ReGIR grid / the NRC render state
    bool regir, nrc;              // tracers: GFX_PT_PATH_TRACE_REGIR; the three NRC tracers
    bool nrcRegir, nrcRestir;     // ... of which the one with ReGIR NEE / with ReSTIR NEE at the first vertex
};

// Validation, and the refusals under a binding.
static PtPass pt_classify(Context& ctx, int pass) {
    if (!ctx.restir.valid) throw HipError("gfx_pt_launch: gfx_restir_set_params has not been called");
    PtPass k;
    k.displaced = ctx.displaced.set != nullptr;
    if (k.displaced) {
        // a binding that carries GFX_DISPLACED_REGIR runs the four ReGIR passes; NRC stays refused under every binding
        const bool regirBound = (ctx.displaced.passMask & GFX_DISPLACED_REGIR) != 0;
        const bool regirOwn = pass >= GFX_PT_REGIR_BUILD_CELL_RESERVOIRS && pass <= GFX_PT_REGIR_UPDATE_LAST_ACCESS;
        if (pass != GFX_PT_PATH_TRACE_BASELINE && !(regirBound && regirOwn)) {
            if (regirBound)
                throw HipError("gfx_pt_launch: a displaced instance set is bound (gfx_scene_bind_displaced_passes with GFX_DISPLACED_REGIR): the G-buffer pass, "
                               "the baseline path tracer and the ReGIR passes render displaced instances; NRC pass " + std::to_string(pass) + " is refused");
            throw HipError("gfx_pt_launch: a displaced instance set is bound (gfx_scene_bind_displaced): only the G-buffer pass and the baseline path tracer "
                           "render displaced instances; ReGIR / NRC pass " + std::to_string(pass) + " is refused");
        }
        displaced_check(ctx, "gfx_pt_launch");
    }
    k.nrcRegir = pass == GFX_PT_PATH_TRACE_NRC_REGIR; k.nrcRestir = pass == GFX_PT_PATH_TRACE_NRC_RESTIR;
    k.regirPass = (pass >= GFX_PT_REGIR_BUILD_CELL_RESERVOIRS && pass <= GFX_PT_REGIR_UPDATE_LAST_ACCESS) || k.nrcRegir;
    k.nrcPass = (pass >= GFX_PT_NRC_PREPROCESS && pass <= GFX_PT_NRC_COUNT_QUERIES) || k.nrcRegir || k.nrcRestir;
    if (!k.regirPass && !k.nrcPass && pass != GFX_PT_PATH_TRACE_BASELINE) throw HipError("gfx_pt_launch: unknown pass");
    if (k.regirPass && !ctx.regirValid) throw HipError("gfx_pt_launch: gfx_regir_set_params has not been called");
    if (k.nrcPass && !ctx.nrcRenderValid) throw HipError("gfx_pt_launch: gfx_nrc_set_render_params has not been called");
    k.regir = pass == GFX_PT_PATH_TRACE_REGIR;
    k.nrc = pass == GFX_PT_PATH_TRACE_NRC || k.nrcRegir || k.nrcRestir;
    return k;
}

// The NRC passes that are one small kernel each.  False: `pass` is none of them.
static bool pt_launch_nrc_small(Context& ctx, hipStream_t stream, int pass, PtArgs& a, uint32_t width, uint32_t height, uint32_t rowBegin, uint32_t rowEnd) {
    auto simple = [&](const char* name, void (*kernel)(PtArgs), size_t threads) {
        launch_timed(ctx, stream, name, kernel, dim3(static_cast<uint32_t>((threads + kPtBlock - 1) / kPtBlock)), dim3(kPtBlock), a);
    };
    switch (pass) {
    case GFX_PT_NRC_PREPROCESS: simple("nrc_preprocess", k_nrc_preprocess, a.nrc.maxNumTrainingSuffixes); return true;
    case GFX_PT_NRC_ACCUMULATE:   // the one per-pixel NRC pass besides the path tracing: honours the row band
        if (rowEnd > height || rowBegin > rowEnd) throw HipError("gfx_pt_launch: row range outside the image");
        a.px = make_pixel_grid(ctx, width, rowBegin, (rowBegin == 0 && rowEnd == 0) ? height : rowEnd);
        if (a.px.rowEnd != a.px.rowBegin) simple("nrc_accumulate", k_nrc_accumulate, static_cast<size_t>(a.px.launchBlocks) * kPtBlock);
        return true;
    case GFX_PT_NRC_PROPAGATE: simple("nrc_propagate", k_nrc_propagate, a.nrc.maxNumTrainingSuffixes); return true;
    case GFX_PT_NRC_SHUFFLE: simple("nrc_shuffle", k_nrc_shuffle, kNumTrainingDataPerFrame); return true;
    case GFX_PT_NRC_VISUALIZE_PREDICTION: simple("nrc_visualize", k_nrc_visualize, static_cast<size_t>(a.s.imageSizeX) * a.s.imageSizeY); return true;
    case GFX_PT_NRC_COUNT_QUERIES:
        if (!ctx.nrcQueryCount.p) { ctx.nrcQueryCount.reserve(256); GFX_HIP(hipMemsetAsync(ctx.nrcQueryCount.p, 0, 256, stream)); }
        launch_checked(stream, k_nrc_count_queries, dim3(1), dim3(1), a, ctx.nrcQueryCount.as<uint32_t>());
        return true;
    default: return false;
    }
}

// The ReGIR grid passes: cell build (with or without temporal reuse) and the last-access update.  False: `pass` is none of them.
static bool pt_launch_regir_grid(Context& ctx, hipStream_t stream, int pass, const PtArgs& a) {
    if (pass == GFX_PT_REGIR_BUILD_CELL_RESERVOIRS || pass == GFX_PT_REGIR_BUILD_CELL_RESERVOIRS_TEMPORAL) {
        const size_t numLightSlots = static_cast<size_t>(a.g.gridDimension[0]) * a.g.gridDimension[1] * a.g.gridDimension[2] * kNumLightSlotsPerCell;
        const bool temporal = pass != GFX_PT_REGIR_BUILD_CELL_RESERVOIRS;
        launch_timed(ctx, stream, "regir_build_cells", temporal ? k_regir_build<true> : k_regir_build<false>,
                     dim3(static_cast<uint32_t>((numLightSlots + kPtBlock - 1) / kPtBlock)), dim3(kPtBlock), a);
        return true;
    }
    if (pass == GFX_PT_REGIR_UPDATE_LAST_ACCESS) {
        const uint32_t numCells = a.g.gridDimension[0] * a.g.gridDimension[1] * a.g.gridDimension[2];
        launch_timed(ctx, stream, "regir_update_last_access", k_regir_update_last_access, dim3((numCells + kPtBlock - 1) / kPtBlock), dim3(kPtBlock), a);
        return true;
    }
    return false;
}

// One tracer launch over a row band: what the one-kernel form and the wavefront loop share.
struct PtLaunch {
    PtPass k;
    PtArgs a;
    uint32_t width, rowBegin, rowEnd, maxPathLength;
    size_t bandPixels;
    uint32_t grid;                // blocks of a launch with one thread per queue entry (capacity = the band's pixels)
    const Accel* accel;
    bool shellRender;             // a kinds binding over a set with a shell member: the extension trace hands the shell part of every hit on
    uint32_t* counters;           // [0] nee (even bounces), [1] ext ping, [2] ext pong, [3] nee (odd bounces), [4] the slot ticket of k_pt_regen
    uint32_t* neeCounts[2];
    float4* extOrg[2]; float4* extDir[2]; uint32_t* extOwner[2];
    void set_queues(int in, int out) {
        a.extOrgIn = extOrg[in]; a.extDirIn = extDir[in]; a.extOwnerIn = extOwner[in]; a.extCountIn = counters + 1 + in;
        a.extOrgOut = extOrg[out]; a.extDirOut = extDir[out]; a.extOwnerOut = extOwner[out]; a.extCountOut = counters + 1 + out;
    }
};

// The checks of a tracer launch, buffer reservation and the PtArgs set-up (L.k, L.a.scene / s / f / g / nrc are set).  False: the
// band is empty.
static bool pt_prepare(Context& ctx, hipStream_t stream, PtLaunch& L, uint32_t width, uint32_t height, uint32_t maxPathLength, uint32_t rowBegin, uint32_t rowEnd) {
    const RestirParams& rp = ctx.restir;
    const PtPass& k = L.k;
    PtArgs& a = L.a;
    if (k.nrcRestir) {
        if (!rp.s.reservoirBuffer[0] || !rp.s.reservoirBuffer[1] || !rp.s.reservoirInfoBuffer[0] || !rp.s.reservoirInfoBuffer[1] ||
            !rp.s.gbuffer2[0] || !rp.s.gbuffer3[0])
            throw HipError("gfx_pt_launch: GFX_PT_PATH_TRACE_NRC_RESTIR reads the reservoirs and G-buffers 2 / 3 of the ReSTIR passes (static parameters)");
        if (!(rowBegin == 0 && (rowEnd == 0 || rowEnd == height)))
            throw HipError("gfx_pt_launch: GFX_PT_PATH_TRACE_NRC_RESTIR is a whole-frame pass");
        a.curRes = rp.currentReservoirIndex & 1u;
    }
    if (static_cast<uint32_t>(rp.s.imageSizeX) != width || static_cast<uint32_t>(rp.s.imageSizeY) != height)
        throw HipError("gfx_pt_launch: launch size differs from imageSize in the static parameters");
    const uint64_t h = rp.f.travHandle;
    if (h == 0 || h > ctx.accels.size() || !ctx.accels[h - 1]) throw HipError("gfx_pt_launch: invalid travHandle");
    if (rowEnd > height || rowBegin > rowEnd) throw HipError("gfx_pt_launch: row range outside the image");
    L.width = width; L.rowBegin = rowBegin; L.rowEnd = rowEnd;
    L.maxPathLength = maxPathLength & 15u;   // 4-bit bitfield, path_tracing_shared.h:165
    L.accel = ctx.accels[h - 1];
    const size_t numPixels = static_cast<size_t>(width) * height;
    const size_t bandPixels = L.bandPixels = static_cast<size_t>(rowEnd - rowBegin) * width;
    if (bandPixels == 0) return false;
    ctx.rayOrg.reserve(16 * numPixels); ctx.rayDir.reserve(16 * numPixels);   // NEE queue
    ctx.rayOut.reserve(4 * numPixels);
    ctx.rayHits.reserve(sizeof(gfx_hit) * numPixels);
    ctx.ptPending.reserve(16 * bandPixels);
    ctx.ptExtOrg.reserve(2 * 16 * bandPixels); ctx.ptExtDir.reserve(2 * 16 * bandPixels); ctx.ptExtOwner.reserve(2 * 4 * bandPixels);
    ctx.ptState.reserve(32 * numPixels);
    if (k.nrc) { ctx.nrcState.reserve(32 * numPixels); ctx.neeTrainIdx.reserve(4 * numPixels); }
    if (k.displaced) { ctx.displaced.ptHits.reserve(sizeof(gfx_scene_hit) * bandPixels); ctx.displaced.ptPlain.reserve(sizeof(gfx_hit) * bandPixels); }
    L.shellRender = k.displaced && displaced_shell_render(ctx);
    if (L.shellRender) ctx.displaced.ptShellPart.reserve(sizeof(gfx_scene_shell_part) * bandPixels);
    ctx.smallCounters.reserve(kSmallCountersBytes);
    L.counters = ctx.smallCounters.as<uint32_t>() + 8;
    GFX_HIP(hipMemsetAsync(L.counters, 0, 5 * sizeof(uint32_t), stream));
    L.neeCounts[0] = L.counters; L.neeCounts[1] = L.counters + 3;
    // "pt_overlap": the second stream of the wavefront loop and the two events that order it (made here, before any kernel of the
    // launch: which of the context's streams exist first decides which keep a hardware queue to themselves, restir.hip block_order_end)
    if (ctx.tune.ptOverlap && !ctx.auxStream) GFX_HIP(hipStreamCreateWithFlags(&ctx.auxStream, hipStreamNonBlocking));
    if (ctx.tune.ptOverlap && !ctx.auxFork) {
        GFX_HIP(hipEventCreateWithFlags(&ctx.auxFork, hipEventDisableTiming));
        GFX_HIP(hipEventCreateWithFlags(&ctx.auxJoin, hipEventDisableTiming));
    }

    a.px = make_pixel_grid(ctx, width, rowBegin, rowEnd);
    a.neeOrg = ctx.rayOrg.as<float4>(); a.neeDir = ctx.rayDir.as<float4>(); a.neePending = ctx.ptPending.as<float4>();
    a.neeCount = L.neeCounts[0];
    a.occluded = ctx.rayOut.as<uint32_t>();
    a.hits = ctx.rayHits.as<gfx_hit>();
    a.tris = L.accel->trisPtr();
    a.state = ctx.ptState.as<float4>();
    if (k.nrc) { a.nrcState = ctx.nrcState.as<float4>(); a.neeTrainIdx = ctx.neeTrainIdx.as<uint32_t>(); }
    for (int i = 0; i < 2; ++i) {
        L.extOrg[i] = ctx.ptExtOrg.as<float4>() + i * bandPixels; L.extDir[i] = ctx.ptExtDir.as<float4>() + i * bandPixels;
        L.extOwner[i] = ctx.ptExtOwner.as<uint32_t>() + i * bandPixels;
    }
    L.grid = static_cast<uint32_t>((bandPixels + kPtBlock - 1) / kPtBlock);
    L.set_queues(1, 0);          // k_pt_first fills queue 0
    a.pathLength = 1; a.maxLengthTerminate = 0;
    a.nextMaxLengthTerminate = 2 >= L.maxPathLength ? 1u : 0u;
    return true;
}

// The path of a pixel in one kernel, for a launch of about one round of waves (512 x 512; a band of an 8-way split full-HD frame).
// "fuse_passes" 1 never, 2 always; counting launches keep the wavefront form (the counters live in k_trace), and so do a bound set and
// the NRC tracers.  False: the launch takes the wavefront form.
static bool pt_launch_one_kernel(Context& ctx, hipStream_t stream, PtLaunch& L) {
    PtArgs& a = L.a;
    const bool regir = L.k.regir;
    const uint32_t launchWaves = a.px.launchBlocks * (kPtBlock / 64), waveSlots = static_cast<uint32_t>(ctx.numCUs) * 16u;
    const int spillCap = static_cast<int>(local_spill_depth(L.accel->maxDepth));
    const size_t spillBytes = sizeof(uint2) * static_cast<size_t>(a.px.launchBlocks) * kPtBlock * spillCap;
    const bool small = launchWaves <= waveSlots + waveSlots / 2;
    if (L.k.displaced || L.k.nrc || ctx.countersEnabled || spillBytes > (size_t(1) << 30) || !(ctx.tune.fusePasses == 2 || (ctx.tune.fusePasses == 0 && small))) return false;
    ctx.lastNee.state = 2;
    ctx.spill.reserve(spillBytes);
    const DevAccel accel = L.accel->dev();
    unsigned long long* ptDiag = nullptr;             // "pt_diag": wave iterations / lanes with a ray / traversal steps / waves / refills (gfx_pt_diag_read)
    if (ctx.tune.ptDiag) {
        if (!ctx.ptDiag.p) { ctx.ptDiag.reserve(64); GFX_HIP(hipMemsetAsync(ctx.ptDiag.p, 0, 64, stream)); }
        ptDiag = ctx.ptDiag.as<unsigned long long>();
    }
    // Path regeneration (k_pt_regen): when the launch is more blocks than the GPU holds at once, launch what it holds and let the
    // lanes draw pixels until none are left ("pt_regen": resident blocks per CU, 0 = off)
    const uint32_t regenBlocks = static_cast<uint32_t>(ctx.tune.ptRegen) * static_cast<uint32_t>(ctx.numCUs);
    if (!regir && ctx.tune.ptRegen > 0 && a.px.launchBlocks > regenBlocks) {
        a.px.order = nullptr;
        launch_timed(ctx, stream, "pt_regen", k_pt_regen, dim3(regenBlocks), dim3(kPtBlock), a, accel, ctx.spill.as<uint2>(), spillCap, L.maxPathLength,
                     L.counters + 4, a.px.launchBlocks * static_cast<uint32_t>(kPtBlock), ctx.tune.ptRegenMin, ptDiag);
        return true;
    }
    // 159 VGPRs: three blocks per CU are resident, so a 512 x 512 frame (1 024 blocks) is already more than one round
    const uint64_t key = (static_cast<uint64_t>(L.rowBegin) << 44) ^ (static_cast<uint64_t>(L.rowEnd) << 24) ^ (static_cast<uint64_t>(L.width) << 4) ^ (regir ? 1u : 0u);
    launch_cost_ordered(ctx, stream, 4, a.px.launchBlocks, key, 3u * static_cast<uint32_t>(ctx.numCUs), a.px, [&](uint32_t* cost) {
        launch_timed(ctx, stream, regir ? "pt_regir_fused" : "pt_fused", regir ? k_pt_fused<true> : k_pt_fused<false>, dim3(a.px.launchBlocks), dim3(kPtBlock),
                     a, accel, ctx.spill.as<uint2>(), spillCap, L.maxPathLength, cost, ptDiag);
    });
    return true;
}

// The wavefront form: k_pt_first, then per bounce the NEE trace with its apply kernel and the extension trace with its bounce kernel.
static void pt_launch_wavefront(Context& ctx, hipStream_t stream, PtLaunch& L) {
    PtArgs& a = L.a;
    const PtPass& k = L.k;
    const bool regir = k.regir, nrc = k.nrc, displaced = k.displaced, shellRender = L.shellRender;
    const uint32_t maxPathLength = L.maxPathLength;
    uint32_t* const counters = L.counters;
    const DevAccel accel = L.accel->dev();
    const dim3 pixels(a.px.launchBlocks), entries(L.grid), block(kPtBlock);   // one thread per pixel of the band (a.px) / per queue entry
    // The NEE trace of a bounce (any-hit) and the kernel that applies its result touch the NEE queue, the occlusion words and the
    // per-pixel contribution; the extension trace of the same bounce (closest-hit) touches the extension queue and the hit records:
    // disjoint, and both only needed by the bounce kernel.  So the first two run on a second stream (own stack-spill / ticket scratch)
    // underneath the third -- small launches are mostly ramp-up and the tail of their longest rays (profiles/r04_experiments.txt 8),
    // which now overlap.  The NEE queue head alternates between two words so that the extension trace can zero the one the bounce kernel
    // appends to while the NEE trace still reads the other.
    const bool overlap = ctx.tune.ptOverlap != 0;      // (pt_prepare has made the second stream and its two events)
    hipStream_t neeStream = overlap ? ctx.auxStream : stream;
    auto join = [&]() { if (overlap) GFX_HIP(hipStreamWaitEvent(stream, ctx.auxJoin, 0)); };
    // Under a binding (any) a trace is the scene query with a device-side count over the queue capacity; the extension trace's plain
    // phase has a buffer of the binding's own, the any-hit form writes only its occlusion words: the two may overlap on two streams as
    // the plain ones do
    auto trace = [&](hipStream_t s, bool auxScratch, int mode, const float4* org, const float4* dir, const uint32_t* count, void* out,
                     uint32_t* zero0 = nullptr, uint32_t* zero1 = nullptr) {
        SceneTrace q;
        q.rayOrgTmin = org; q.rayDirTmax = dir; q.numRays = static_cast<uint32_t>(L.bandPixels); q.numRaysPtr = count; q.mode = mode; q.out = out;
        q.plainHits = ctx.displaced.ptPlain.p;
        if (shellRender && mode == GFX_TRACE_CLOSEST) q.shellPart = ctx.displaced.ptShellPart.p;
        q.zeroWords[0] = zero0; q.zeroWords[1] = zero1;
        if (auxScratch) { q.spill = &ctx.auxSpill; q.counters = &ctx.auxCounters; }
        trace_ray_queue(ctx, s, accel, displaced, q);
    };

    int cur = 0;                 // the queue k_pt_first fills (pt_prepare)
    void* const extHits = displaced ? ctx.displaced.ptHits.p : ctx.rayHits.p;
    if (displaced) {
        void (*const first[2][2])(PtArgs, DisplacedArgs) = { { k_pt_first_scene, k_pt_first_scene_shell }, { k_pt_regir_first_scene, k_pt_regir_first_scene_shell } };
        const char* const names[2][2] = { { "pt_first_scene", "pt_first_scene_shell" }, { "pt_regir_first_scene", "pt_regir_first_scene_shell" } };
        launch_timed(ctx, stream, names[regir][shellRender], first[regir][shellRender], pixels, block, a, displaced_args(ctx, extHits));
    }
    else if (nrc) launch_timed(ctx, stream, "nrc_pt_first", k.nrcRegir ? k_nrc_pt_first<1> : k.nrcRestir ? k_nrc_pt_first<2> : k_nrc_pt_first<0>, pixels, block, a);
    else launch_timed(ctx, stream, "pt_first", regir ? k_pt_first<true> : k_pt_first<false>, pixels, block, a);
    // while (true) { ++pathLength; trace; }.  Baseline: at least one extension even when maxPathLength < 2,
    // the terminal vertex (implicit light only) emits no NEE ray.  ReGIR: the loop head breaks before the
    // trace at the length limit, so the last vertex's NEE ray is resolved after the loop.  NRC:
    // maxPathLength == 0 means unlimited bounces (neural_radiance_caching_main.cpp:2246) -- the live
    // path count is read back every fourth bounce to stop (the 6-bit pathLength field caps it at 63).
    int nee = 0;                 // the NEE queue head the last vertex kernel appended to
    for (uint32_t pathLength = 2;; ++pathLength) {
        if (overlap) { GFX_HIP(hipEventRecord(ctx.auxFork, stream)); GFX_HIP(hipStreamWaitEvent(neeStream, ctx.auxFork, 0)); }
        a.neeCount = L.neeCounts[nee];
        trace(neeStream, overlap, GFX_TRACE_ANY, a.neeOrg, a.neeDir, a.neeCount, ctx.rayOut.p);
        ctx.lastNee = { 1, a.neeOrg, a.neeDir, ctx.rayOut.p, a.neePending, a.neeCount };
        launch_timed(ctx, neeStream, "pt_apply_nee", k_pt_apply_nee, entries, block, a);
        if (overlap) GFX_HIP(hipEventRecord(ctx.auxJoin, neeStream));
        if (regir && pathLength >= maxPathLength) { join(); break; }
        // NRC: training paths skip Russian roulette (and with it the length test) at pathLength 2 (:459-462),
        // so the last vertex that can exist is max(maxPathLength, 3)
        if (nrc && maxPathLength > 0 && pathLength > (maxPathLength > 3 ? maxPathLength : 3)) { join(); break; }
        if (nrc && pathLength >= 63) { join(); break; }
        if (nrc && maxPathLength == 0 && pathLength > 2 && (pathLength & 3u) == 2u) {
            uint32_t live = 0;
            GFX_HIP(hipMemcpyAsync(&live, counters + 1 + cur, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
            GFX_HIP(hipStreamSynchronize(stream));
            if (live == 0) { join(); break; }
        }
        // the extension trace also resets the two queue heads the bounce kernel appends to (the NEE head of the NEXT bounce -- not the
        // one the NEE trace above is reading -- and the other extension queue): no memset between the kernels of a bounce
        trace(stream, false, GFX_TRACE_CLOSEST, L.extOrg[cur], L.extDir[cur], counters + 1 + cur, extHits, L.neeCounts[nee ^ 1], counters + 1 + (cur ^ 1));
        join();                  // the bounce kernel adds to the contribution after k_pt_apply_nee has, and rewrites the NEE queue
        L.set_queues(cur, cur ^ 1);
        nee ^= 1;
        a.neeCount = L.neeCounts[nee];
        a.pathLength = pathLength;
        a.maxLengthTerminate = (pathLength >= maxPathLength && (!nrc || maxPathLength > 0)) ? 1u : 0u;
        a.nextMaxLengthTerminate = pathLength + 1 >= maxPathLength ? 1u : 0u;
        if (displaced) {
            const char* const names[2][2] = { { "pt_bounce_scene", "pt_bounce_scene_shell" }, { "pt_regir_bounce_scene", "pt_regir_bounce_scene_shell" } };
            if (shellRender)
                launch_timed(ctx, stream, names[regir][1], regir ? k_pt_regir_bounce_scene_shell : k_pt_bounce_scene_shell, entries, block, a, displaced_args(ctx, extHits),
                             displaced_shell_args(ctx, ctx.displaced.ptShellPart.p));
            else launch_timed(ctx, stream, names[regir][0], regir ? k_pt_regir_bounce_scene : k_pt_bounce_scene, entries, block, a, displaced_args(ctx, extHits));
        }
        else if (nrc) launch_timed(ctx, stream, "nrc_pt_bounce", k.nrcRegir ? k_nrc_pt_bounce<1> : k.nrcRestir ? k_nrc_pt_bounce<2> : k_nrc_pt_bounce<0>, entries, block, a);
        else launch_timed(ctx, stream, "pt_bounce", regir ? k_pt_bounce<true> : k_pt_bounce<false>, entries, block, a);
        cur ^= 1;
        if (!regir && !nrc && a.maxLengthTerminate) break;
    }
    if (nrc) launch_timed(ctx, stream, "nrc_pt_finish", k_nrc_pt_finish, pixels, block, a);
    else launch_timed(ctx, stream, "pt_finish", k_pt_finish, pixels, block, a);
}

void pathtrace_launch(Context& ctx, hipStream_t stream, int pass, uint32_t width, uint32_t height,
                      uint32_t maxPathLength, uint32_t rowBegin, uint32_t rowEnd) {
    if (pass == GFX_PT_SETUP_GBUFFERS) {
        // path_tracing/gpu_kernels/optix_gbuffer_kernels.cu: same program text as ReSTIR's G-buffer
        // pass (GBuffer0/1 + albedo/normal accumulation); GBuffer2/3 are simply not read afterwards.
        restir_launch(ctx, stream, GFX_RESTIR_SETUP_GBUFFERS, width, height, rowBegin, rowEnd);
        return;
    }
    PtLaunch L;
    L.k = pt_classify(ctx, pass);
    PtArgs& a = L.a;
    std::memset(&a, 0, sizeof(a));
    a.scene = ctx.devScene();
    a.s = ctx.restir.s; a.f = ctx.restir.f;
    if (L.k.nrcPass) {
        a.nrc = ctx.nrcRender;
        if (pt_launch_nrc_small(ctx, stream, pass, a, width, height, rowBegin, rowEnd)) return;
    }
    if (L.k.regirPass) a.g = ctx.regir;
    if (pt_launch_regir_grid(ctx, stream, pass, a)) return;
    if (!pt_prepare(ctx, stream, L, width, height, maxPathLength, rowBegin, rowEnd)) return;
    if (!pt_launch_one_kernel(ctx, stream, L)) pt_launch_wavefront(ctx, stream, L);
}

} // namespace gfx
