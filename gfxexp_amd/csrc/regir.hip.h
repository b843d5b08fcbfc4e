// regir.hip.h -- the first header of pathtrace.hip's translation unit: PtArgs, the launch arguments of every kernel of it, and ReGIR
// (regir/gpu_kernels/): the grid cell of a point, light sampling from a cell's slot reservoirs (the NEE of the ReGIR tracers,
// pt_vertex.hip.h shade_vertex<true>, which is why PtArgs stands here) and the kernels that maintain the grid.
#pragma once
#include "internal.h"
#include "shading.hip.h"
#include "pass_common.hip.h"
#include "restir_common.hip.h"
#include "trace_local.hip.h"
#include "tfdm/tfdm_set.h"
#include "tfdm/displaced_surface.hip.h"
#include "nrtdsm/displaced_kinds.hip.h"

namespace gfx {

constexpr int kPtBlock = 256;
constexpr uint32_t kNumLightSlotsPerCell = 512;   // regir_shared.h:7

struct PtArgs {
    DevScene scene;
    gfx_restir_static_params s;
    gfx_restir_frame_params f;
    PixelGrid px;                 // per-pixel launches: rows [rowBegin, rowEnd) (restir_common.hip.h)
    uint32_t pathLength;          // pathLength of the vertices k_pt_bounce processes
    uint32_t maxLengthTerminate;  // pathLength >= maxPathLength
    // NEE (any-hit) queue, rebuilt every bounce
    float4* neeOrg; float4* neeDir; float4* neePending;   // pending = alpha * NEE (rgb), owner pixel (w)
    uint32_t* neeCount;
    const uint32_t* occluded;
    // extension (closest-hit) queues: [in] produced by the previous vertex, [out] by this one
    const float4* extOrgIn; const float4* extDirIn; const uint32_t* extOwnerIn; const uint32_t* extCountIn;
    float4* extOrgOut; float4* extDirOut; uint32_t* extOwnerOut; uint32_t* extCountOut;
    const gfx_hit* hits;
    const Bvh8Tri* tris;
    float4* state;                // per pixel: [2p] = alpha.rgb, prevDirPDensity; [2p+1] = contribution.rgb
    gfx_regir_params g;           // ReGIR grid (REGIR kernels only)
    uint32_t nextMaxLengthTerminate;   // pathLength + 1 >= maxPathLength (ReGIR loop head)
    gfx_nrc_params nrc;           // NRC render state (NRC kernels only)
    float4* nrcState;             // per pixel: [2p] = prevLocalThroughput.rgb, primaryPathSpread;
                                  //            [2p+1] = curSqrtPathSpread, prevTrainDataIndex, flags, -
    uint32_t* neeTrainIdx;        // per NEE slot: training record initialised with that NEE estimate (or invalid)
    uint32_t curRes;              // GFX_PT_PATH_TRACE_NRC_RESTIR: the reservoir buffer the frame's ReSTIR passes finished in
};

GFX_DEV uint32_t regir_cell_index(const gfx_regir_params& g, f3 pw) {   // regir_shared.h:731-744
    const float rx = (pw.x - g.gridOrigin[0]) / g.gridCellSize[0];
    const float ry = (pw.y - g.gridOrigin[1]) / g.gridCellSize[1];
    const float rz = (pw.z - g.gridOrigin[2]) / g.gridCellSize[2];
    uint32_t ix = f2u_sat(rx); if (ix > g.gridDimension[0] - 1) ix = g.gridDimension[0] - 1;
    uint32_t iy = f2u_sat(ry); if (iy > g.gridDimension[1] - 1) iy = g.gridDimension[1] - 1;
    uint32_t iz = f2u_sat(rz); if (iz > g.gridDimension[2] - 1) iz = g.gridDimension[2] - 1;
    return iz * g.gridDimension[0] * g.gridDimension[1] + iy * g.gridDimension[0] + ix;
}

// atomicAdd(&perCellNumAccesses[cell], 1) with the lanes of a wave that touch the same cell merged
// into one atomic (same totals; neighbouring pixels mostly share a cell).
GFX_DEV void regir_count_access(uint32_t* perCellNumAccesses, bool active, uint32_t cell) {
    unsigned long long todo = __ballot(active);
    const int lane = threadIdx.x & 63;
    while (todo) {
        const int leader = __builtin_ctzll(todo);
        const uint32_t leaderCell = __shfl(cell, leader);
        const unsigned long long same = __ballot(active && cell == leaderCell) & todo;
        if (lane == leader) atomicAdd(perCellNumAccesses + leaderCell, static_cast<uint32_t>(__popcll(same)));
        todo &= ~same;
    }
}

// sampleFromCell, regir/gpu_kernels/optix_pathtracing_kernels.cu:18-82.  Every lane of the wave must
// call it (`active` = lanes that shade a vertex).
GFX_DEV f3 regir_sample_from_cell(const PtArgs& a, bool active, f3 pos, f3 vOutLocal, const Frame& frame, const Bsdf& bsdf, Pcg32& rng,
                                  LightSample& ls, float& recPDF) {
    const gfx_regir_params& g = a.g;
    uint32_t cell = 0;
    if (active) {
        f3 off(0.0f);
        if (g.enableCellRandomization) {
            const float r0 = rng.uniform();
            const float r1 = rng.uniform();
            const float r2 = rng.uniform();
            off = f3(g.gridCellSize[0], g.gridCellSize[1], g.gridCellSize[2]) * f3(-0.5f + r0, -0.5f + r1, -0.5f + r2);
        }
        cell = regir_cell_index(g, pos + off);
    }
    regir_count_access(static_cast<uint32_t*>(g.perCellNumAccesses), active, cell);
    f3 selectedContribution(0.0f);
    ls.emittance = f3(0.0f); ls.position = f3(0.0f); ls.normal = f3(0.0f); ls.atInfinity = 0;
    recPDF = 0.0f;
    if (!active) return selectedContribution;
    const size_t numLightSlots = static_cast<size_t>(g.gridDimension[0]) * g.gridDimension[1] * g.gridDimension[2] * kNumLightSlotsPerCell;
    const size_t resStart = static_cast<size_t>(kNumLightSlotsPerCell) * cell;
    const uint32_t bufferIndex = a.f.bufferIndex;
    const uint32_t numResampling = 1u << g.log2NumCandidatesPerCell;
    Reservoir combined;
    combined.reset();
    uint32_t combinedStreamLength = 0;
    float selectedTarget = 0.0f;
    for (uint32_t i = 0; i < numResampling; ++i) {
        uint32_t k = f2u_sat(rng.uniform() * kNumLightSlotsPerCell);
        if (k > kNumLightSlotsPerCell - 1) k = kNumLightSlotsPerCell - 1;
        const size_t slot = resStart + k;
        const Reservoir r = load_reservoir(g.reservoirs[bufferIndex], numLightSlots, slot);
        const float slotRecPDF = static_cast<const float2*>(g.reservoirInfos[bufferIndex])[slot].x;
        combinedStreamLength += r.streamLength;
        if (slotRecPDF == 0.0f) continue;
        const f3 cont = direct_lighting(pos, vOutLocal, frame, bsdf, r.sample);
        const float target = target_weight(cont);
        const float weight = target * slotRecPDF * r.streamLength;
        if (combined.update(r.sample, weight, rng.uniform())) { selectedContribution = cont; selectedTarget = target; }
    }
    combined.streamLength = combinedStreamLength;
    ls = combined.sample;
    const float weightForEstimate = 1.0f / combined.streamLength;
    recPDF = weightForEstimate * combined.sumWeights / selectedTarget;
    if (!is_finite(recPDF)) recPDF = 0.0f;
    return selectedContribution;
}

// ---------------------------------------------------------------- ReGIR grid maintenance
// sampleIntensity, regir/gpu_kernels/build_cell_reservoirs.cu:6-68 (the half-space tests compare lpCos,
// still 1 at that point, with minSquaredDistance -- restated literally)
GFX_DEV f3 regir_sample_intensity(const LightSample& ls, f3 cellCenter, f3 halfCellSize, float minSquaredDistance) {
    float dist2 = minSquaredDistance;
    float lpCos = 1;
    const bool outside = ls.atInfinity ||
        ls.position.x < cellCenter.x - halfCellSize.x || ls.position.x > cellCenter.x + halfCellSize.x ||
        ls.position.y < cellCenter.y - halfCellSize.y || ls.position.y > cellCenter.y + halfCellSize.y ||
        ls.position.z < cellCenter.z - halfCellSize.z || ls.position.z > cellCenter.z + halfCellSize.z;
    if (outside) {
        const f3 d = ls.atInfinity ? ls.position : (ls.position - cellCenter);
        const float perpDistance = dot(-d, ls.normal);
        dist2 = len2(d);
        const float dist = sqrtf(dist2);
        const bool valid = lpCos > minSquaredDistance || ls.atInfinity;
        const bool invalid = lpCos < -minSquaredDistance;
        if (valid) lpCos = perpDistance / dist;
        else if (invalid) lpCos = 0.0f;
    }
    if (lpCos > 0.0f) {
        const f3 Le = ls.emittance / kPi;
        return Le * (lpCos / dist2);
    }
    return f3(0.0f);
}

// buildCellReservoirsAndTemporalReuse<TEMPORAL>, build_cell_reservoirs.cu:70-219: one thread per light slot
template <bool TEMPORAL>
__global__ __launch_bounds__(kPtBlock) void k_regir_build(PtArgs a) {
    const gfx_regir_params& g = a.g;
    const uint32_t numCells = g.gridDimension[0] * g.gridDimension[1] * g.gridDimension[2];
    const size_t numLightSlots = static_cast<size_t>(numCells) * kNumLightSlotsPerCell;
    const size_t i = static_cast<size_t>(blockIdx.x) * kPtBlock + threadIdx.x;
    if (i >= numLightSlots) return;
    const uint32_t bufferIndex = a.f.bufferIndex;
    const uint32_t cell = static_cast<uint32_t>(i / kNumLightSlotsPerCell);
    const uint32_t lastAccess = static_cast<const uint32_t*>(g.lastAccessFrameIndices)[cell];
    if (i == 0) *static_cast<uint32_t*>(g.numActiveCells[bufferIndex]) = 0;
    if (i % kNumLightSlotsPerCell == 0) static_cast<uint32_t*>(g.perCellNumAccesses)[cell] = 0;
    if (a.f.frameIndex - lastAccess > 8) return;      // block-uniform: a cell owns 512 = 2 x kPtBlock consecutive slots
    const uint32_t gx = g.gridDimension[0], gy = g.gridDimension[1];
    const uint32_t iz = cell / (gx * gy), iy = (cell % (gx * gy)) / gx, ix = cell % gx;
    const f3 cs(g.gridCellSize[0], g.gridCellSize[1], g.gridCellSize[2]);
    const f3 cellCenter = f3(g.gridOrigin[0], g.gridOrigin[1], g.gridOrigin[2]) + f3((ix + 0.5f) * cs.x, (iy + 0.5f) * cs.y, (iz + 0.5f) * cs.z);
    const f3 halfCellSize = 0.5f * cs;
    const float minSquaredDistance = len2(0.5f * cs);
    uint64_t* rngs = static_cast<uint64_t*>(g.lightSlotRngs);
    Pcg32 rng; rng.state = rngs[i];
    const EnvMap env = load_env(a.s);
    const bool envEnabled = env.present() && a.f.enableEnvLight;
    float selectedTarget = 0.0f;
    Reservoir reservoir;
    reservoir.reset();
    const uint32_t numCandidates = 1u << g.log2NumCandidatesPerLightSlot;
    for (uint32_t c = 0; c < numCandidates; ++c) {
        float ul = rng.uniform();
        bool sampleEnv = false;
        float probCurType = 1.0f;
        if (envEnabled) {
            if (*a.scene.lightInstIntegral > 0.0f) {
                const float prob = fmin2(fmax2(0.25f * numCandidates - c, 0.0f), 1.0f);
                // prob is 0 or 1 for every candidate count >= 4: x / 1 and (x - 0) / (1 - 0) are x, no division needed
                if (prob == 1.0f) { probCurType = 0.25f; sampleEnv = true; }
                else if (prob == 0.0f) probCurType = 1.0f - 0.25f;
                else if (ul < prob) { probCurType = 0.25f; ul = ul / prob; sampleEnv = true; }
                else { probCurType = 1.0f - 0.25f; ul = (ul - prob) / (1 - prob); }
            }
            else sampleEnv = true;
        }
        LightSample ls;
        ls.emittance = f3(0.0f); ls.position = f3(0.0f); ls.normal = f3(0.0f); ls.atInfinity = 0;
        float pd;
        const float u0 = rng.uniform();
        const float u1 = rng.uniform();
        sample_light(a.scene, env, a.f.envLightRotation, a.f.envLightPowerCoeff, ul, sampleEnv, u0, u1, ls, pd);
        const f3 cont = regir_sample_intensity(ls, cellCenter, halfCellSize, minSquaredDistance);
        pd *= probCurType;
        const float target = target_weight(cont);
        const float weight = target / pd;
        if (reservoir.update(ls, weight, rng.uniform())) selectedTarget = target;
    }
    float recPDF = reservoir.sumWeights / (selectedTarget * reservoir.streamLength);
    if (!is_finite(recPDF)) { recPDF = 0.0f; selectedTarget = 0.0f; }
    if (TEMPORAL) {
        const uint32_t prevBuffer = (bufferIndex + 1) % 2;
        const uint32_t selfStreamLength = reservoir.streamLength;
        if (recPDF == 0.0f) reservoir.reset();
        uint32_t combinedStreamLength = selfStreamLength;
        const uint32_t maxNumPrevSamples = 20 * selfStreamLength;
        const Reservoir prev = load_reservoir(g.reservoirs[prevBuffer], numLightSlots, i);
        const float prevTarget = static_cast<const float2*>(g.reservoirInfos[prevBuffer])[i].y;
        const uint32_t prevLen = prev.streamLength < maxNumPrevSamples ? prev.streamLength : maxNumPrevSamples;
        const float lengthCorrection = static_cast<float>(prevLen) / prev.streamLength;
        const float weight = lengthCorrection * prev.sumWeights;
        if (reservoir.update(prev.sample, weight, rng.uniform())) selectedTarget = prevTarget;
        combinedStreamLength += prevLen;
        reservoir.streamLength = combinedStreamLength;
        const float weightForEstimate = 1.0f / reservoir.streamLength;
        recPDF = weightForEstimate * reservoir.sumWeights / selectedTarget;
        if (!is_finite(recPDF)) { recPDF = 0.0f; selectedTarget = 0.0f; }
    }
    rngs[i] = rng.state;
    store_reservoir(g.reservoirs[bufferIndex], numLightSlots, i, reservoir);
    static_cast<float2*>(g.reservoirInfos[bufferIndex])[i] = make_float2(recPDF, selectedTarget);
}

// updateLastAccessFrameIndices, build_cell_reservoirs.cu:229-243
__global__ __launch_bounds__(kPtBlock) void k_regir_update_last_access(PtArgs a) {
    const gfx_regir_params& g = a.g;
    const uint32_t numCells = g.gridDimension[0] * g.gridDimension[1] * g.gridDimension[2];
    const uint32_t cell = blockIdx.x * kPtBlock + threadIdx.x;
    bool accessed = false;
    if (cell < numCells) {
        accessed = static_cast<const uint32_t*>(g.perCellNumAccesses)[cell] > 0;
        if (accessed) static_cast<uint32_t*>(g.lastAccessFrameIndices)[cell] = a.f.frameIndex;
    }
    const unsigned long long mask = __ballot(accessed);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(static_cast<uint32_t*>(g.numActiveCells[a.f.bufferIndex]), static_cast<uint32_t>(__popcll(mask)));
}

} // namespace gfx
