// nrc_render.hip.h -- neural radiance caching, render side: neural_radiance_caching/gpu_kernels/optix_pathtracing_kernels.cu +
// nrc_setup_kernels.cu on the wavefront pipeline of pathtrace.hip (part of its translation unit; the surface points and the miss
// term are pt_vertex.hip.h's).  Training-record indices come from one wave-aggregated atomicAdd per
// kernel wave (the reference's per-thread atomicAdd order is unspecified as well); the initial
// target of a record is the NEE estimate of its vertex, so the apply kernel zeroes it when the
// shadow ray turns out occluded.
#pragma once
#include "pt_vertex.hip.h"

namespace gfx {

constexpr uint32_t kInvalidVertexDataIndex = 0x007FFFFFu;     // neural_radiance_caching_shared.h:146
constexpr uint32_t kNumTrainingDataPerFrame = 1u << 16, kTrainBufferSize = 2u << 16;   // :8-9
constexpr uint32_t kNrcFlagRenderEnds = 1u, kNrcFlagSuffixEnds = 2u;

GFX_DEV uint32_t nrc_terminal_bits(bool hasQuery, uint32_t pathLength, bool training, bool unbiased) {
    return (hasQuery ? 1u : 0u) | ((pathLength & 0xFFu) << 1) | ((training ? 1u : 0u) << 9) | ((unbiased ? 1u : 0u) << 10);
}
GFX_DEV uint32_t nrc_suffix_bits(uint32_t prevIdx, bool hasQuery, uint32_t pathLength) {
    return (prevIdx & 0x7FFFFFu) | ((hasQuery ? 1u : 0u) << 23) | ((pathLength & 0xFFu) << 24);
}
struct NrcTile { uint32_t linearTileIndex; bool training, unbiased; };
GFX_DEV NrcTile nrc_tile_of(const PtArgs& a, uint32_t pixel) {   // optix_pathtracing_kernels.cu:107-131
    const uint32_t W = static_cast<uint32_t>(a.s.imageSizeX);
    const uint32_t x = pixel % W, y = pixel / W;
    const uint2 ts = *static_cast<const uint2*>(a.nrc.tileSize[a.f.bufferIndex]);
    const uint32_t local = (y % ts.y) * ts.x + (x % ts.x);
    NrcTile t;
    t.training = (local + *static_cast<const uint32_t*>(a.nrc.offsetToSelectTrainingPath)) % (ts.x * ts.y) == 0;
    const uint32_t numTilesX = (W + ts.x - 1) / ts.x;
    const uint32_t tx = x / ts.x, ty = y / ts.y;
    t.linearTileIndex = ty * numTilesX + tx;
    t.unbiased = ((ty % 4) * 4 + (tx % 4) + *static_cast<const uint32_t*>(a.nrc.offsetToSelectUnbiasedTile)) % 16 == 0;
    return t;
}
struct NrcQuery { float v[14]; };
GFX_DEV NrcQuery nrc_make_query(const PtArgs& a, f3 pos, f3 normal, f3 vOut, const Bsdf& bsdf) {   // :12-32
    NrcQuery q;
    const float* lo = a.nrc.sceneAabbMin; const float* hi = a.nrc.sceneAabbMax;
    const float p[3] = { pos.x, pos.y, pos.z };
#pragma unroll
    for (int k = 0; k < 3; ++k) { const float den = hi[k] - lo[k]; q.v[k] = den != 0 ? (p[k] - lo[k]) / den : 0.0f; }
    q.v[4] = gm_acos(fmin2(fmax2(normal.z, -1.0f), 1.0f)); q.v[3] = gm_atan2(normal.y, normal.x);
    q.v[6] = gm_acos(fmin2(fmax2(vOut.z, -1.0f), 1.0f)); q.v[5] = gm_atan2(vOut.y, vOut.x);
    q.v[7] = 1 - gm_exp(-bsdf.roughness);
    q.v[8] = bsdf.diffuse.x; q.v[9] = bsdf.diffuse.y; q.v[10] = bsdf.diffuse.z;
    q.v[11] = bsdf.specularF0.x; q.v[12] = bsdf.specularF0.y; q.v[13] = bsdf.specularF0.z;
    return q;
}
GFX_DEV void nrc_store_query(void* buf, size_t idx, const NrcQuery& q) {
    float2* dst = reinterpret_cast<float2*>(static_cast<float*>(buf) + 14 * idx);
#pragma unroll
    for (int k = 0; k < 7; ++k) dst[k] = make_float2(q.v[2 * k], q.v[2 * k + 1]);
}
// trainDataIndex = atomicAdd(numTrainingData, 1) for the lanes with want, one atomic per wave
GFX_DEV uint32_t nrc_alloc_train_index(uint32_t* counter, bool want) {
    const unsigned long long mask = __ballot(want);
    if (mask == 0ull) return kInvalidVertexDataIndex;
    const int lane = threadIdx.x & 63;
    const int leader = __builtin_ctzll(mask);
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(counter, static_cast<uint32_t>(__popcll(mask)));
    base = __shfl(base, leader);
    return base + __popcll(mask & ((1ull << lane) - 1ull));
}
GFX_DEV void nrc_write_train_vertex(const PtArgs& a, uint32_t idx, const NrcQuery& q, f3 localThroughput, uint32_t prevIdx,
                                    uint32_t pathLength, f3 target) {
    nrc_store_query(a.nrc.trainRadianceQueryBuffer[0], idx, q);
    static_cast<float4*>(a.nrc.trainVertexInfoBuffer)[idx] =
        make_float4(localThroughput.x, localThroughput.y, localThroughput.z, bits2f((prevIdx & 0x7FFFFFu) | ((pathLength & 0xFFu) << 23)));
    float* t = static_cast<float*>(a.nrc.trainTargetBuffer[0]) + 3ull * idx;
    t[0] = target.x; t[1] = target.y; t[2] = target.z;
}
// tail of the ray-generation program for a path that stops here (:339-373)
GFX_DEV void nrc_end_path(const PtArgs& a, uint32_t pixel, const NrcTile& tile, uint32_t flags, uint32_t prevTrainIdx, uint32_t pathLength) {
    if (tile.training && !(flags & kNrcFlagSuffixEnds))
        static_cast<uint32_t*>(a.nrc.trainSuffixTerminalInfoBuffer)[tile.linearTileIndex] = nrc_suffix_bits(prevTrainIdx, false, pathLength);
    if (!(flags & kNrcFlagRenderEnds))
        static_cast<float4*>(a.nrc.inferenceTerminalInfoBuffer)[pixel] =
            make_float4(0.0f, 0.0f, 0.0f, bits2f(nrc_terminal_bits(false, pathLength, tile.training, tile.unbiased)));
}

// preprocessNRC, nrc_setup_kernels.cu:6-49
__global__ __launch_bounds__(kPtBlock) void k_nrc_preprocess(PtArgs a) {
    const uint32_t i = blockIdx.x * kPtBlock + threadIdx.x;
    if (i >= a.nrc.maxNumTrainingSuffixes) return;
    const uint32_t bufIdx = a.f.bufferIndex, prevBufIdx = (a.f.bufferIndex + 1) % 2;
    if (i == 0) {
        uint32_t nx = 8, ny = 8;
        if (!a.nrc.isNewSequence) {
            const uint32_t prevNum = *static_cast<const uint32_t*>(a.nrc.numTrainingData[prevBufIdx]);
            const float r = sqrtf(static_cast<float>(prevNum) / kNumTrainingDataPerFrame);
            const uint2 cur = *static_cast<const uint2*>(a.nrc.tileSize[prevBufIdx]);
            nx = f2u_sat(cur.x * r); ny = f2u_sat(cur.y * r);
            nx = nx < 4u ? 4u : (nx > 128u ? 128u : nx);
            ny = ny < 4u ? 4u : (ny > 128u ? 128u : ny);
        }
        *static_cast<uint2*>(a.nrc.tileSize[bufIdx]) = make_uint2(nx, ny);
        *static_cast<uint32_t*>(a.nrc.numTrainingData[bufIdx]) = 0;
        *static_cast<uint32_t*>(a.nrc.offsetToSelectUnbiasedTile) = a.nrc.preprocessOffsetToSelectUnbiasedTile;
        *static_cast<uint32_t*>(a.nrc.offsetToSelectTrainingPath) = a.nrc.preprocessOffsetToSelectTrainingPath;
        int32_t* mm = static_cast<int32_t*>(a.nrc.targetMinMax[bufIdx]);
        mm[0] = mm[1] = mm[2] = 0x7F800000;                         // floatToOrderedInt(+inf)
        mm[3] = mm[4] = mm[5] = static_cast<int32_t>(0xFF800000u) ^ 0x7FFFFFFF;   // floatToOrderedInt(-inf)
        float* avg = static_cast<float*>(a.nrc.targetAvg[bufIdx]);
        avg[0] = avg[1] = avg[2] = 0.0f;
    }
    static_cast<uint32_t*>(a.nrc.trainSuffixTerminalInfoBuffer)[i] = nrc_suffix_bits(kInvalidVertexDataIndex, false, 0);
}

// pathTrace_raygen_generic<true> up to the path extension loop (:133-318).  REGIR: next-event estimation from the ReGIR
// grid (GFX_PT_PATH_TRACE_NRC_REGIR, include/gfxexp.h).
// NEE: 0 the tracer's own light sample, 1 ReGIR cell sampling, 2 the pixel's ReSTIR DI reservoir (first vertex only).
template <int NEE>
__global__ __launch_bounds__(kPtBlock) void k_nrc_pt_first(PtArgs a) {
    constexpr bool REGIR = NEE == 1;
    const PixelId px = pixel_of_thread(a.px);
    const size_t p = px.p;
    const uint32_t bufIdx = a.f.bufferIndex;
    PtVertexOut o;
    reset_vertex_out(o);
    f3 pos(0.0f), vOutLocal(0.0f), vOut(0.0f);
    Frame frame(f3(0, 0, 1), f3(1, 0, 0));
    Bsdf bsdf; bsdf.type = 0; bsdf.diffuse = f3(0.0f); bsdf.specularF0 = f3(0.0f); bsdf.roughness = 1.0f;
    Pcg32 rng; rng.state = 0;
    const EnvMap env = load_env(a.s);
    const bool envEnabled = env.present() && a.f.enableEnvLight;
    f3 contribution(0.001f, 0.001f, 0.001f);
    f3 alpha(1.0f);
    float dirPDensity = 0.0f, primaryPathSpread = 0.0f;
    const bool inImage = px.valid;
    uint4 g0 = make_uint4(0xFFFFFFFFu, 0, 0, 0);
    if (inImage) g0 = static_cast<const uint4*>(a.s.gbuffer0[bufIdx])[p];
    const bool surface = g0.x != 0xFFFFFFFFu;
    NrcTile tile; tile.linearTileIndex = 0; tile.training = false; tile.unbiased = false;
    if (inImage) tile = nrc_tile_of(a, static_cast<uint32_t>(p));
    if (surface) {
        const PtSurface sp = pt_gbuffer_surface(a, g0);
        const Camera cam = load_camera(a.f.camera);
        rng.state = static_cast<const uint64_t*>(a.s.rngBuffer)[p];
        const gfx_material& mat = a.scene.materials[sp.materialSlot];
        // (unit() spelt out: the path spread wants the squared distance and the cosine as well)
        vOut = cam.pos - sp.pos;
        const float primaryDist2 = len2(vOut);
        vOut = vOut / sqrtf(primaryDist2);
        const float primaryDotVN = dot(vOut, sp.ng);
        const float frontHit = primaryDotVN >= 0.0f ? 1.0f : -1.0f;
        pos = offset_ray_origin(sp.pos, frontHit * sp.ng);
        primaryPathSpread = primaryDist2 / (4 * kPi * fabsf(primaryDotVN));
        const float tu = sp.tu(), tv = sp.tv();
        frame = Frame(sp.ns, sp.tc0);
        if (a.f.enableBumpMapping) apply_bump_mapping(read_modified_normal(a.scene, mat, tu, tv), frame);
        vOutLocal = frame.to_local(vOut);
        contribution = f3(0.0f);
        if (vOutLocal.z > 0 && mat.hasEmittance)
            contribution = contribution + alpha * material_emittance(a.scene, mat, tu, tv) / kPi;
        bsdf.setup(a.scene, mat, tu, tv);
    }
    else if (inImage && envEnabled) {
        contribution = a.f.envLightPowerCoeff * env.fetch(decode_bc(g0.w & 0xFFFF), decode_bc(g0.w >> 16));
    }
    if (NEE == 2) {
        ReservoirNee given;
        given.ret = f3(0.0f); given.org = f3(0.0f);
        given.ls.emittance = f3(0.0f); given.ls.position = f3(0.0f); given.ls.normal = f3(0.0f); given.ls.atInfinity = 0;
        if (surface) given = restir_reservoir_nee(a, bufIdx, p);
        shade_vertex<false, false>(a, surface, env, envEnabled, pos, vOutLocal, frame, bsdf, rng, alpha, contribution, dirPDensity, o, &given);
    }
    else shade_vertex<REGIR, false>(a, surface, env, envEnabled, pos, vOutLocal, frame, bsdf, rng, alpha, contribution, dirPDensity, o);
    // training record of the first vertex (:238-277)
    uint32_t trainIdx = nrc_alloc_train_index(static_cast<uint32_t*>(a.nrc.numTrainingData[bufIdx]), surface && tile.training);
    if (surface && tile.training) {
        if (trainIdx < kTrainBufferSize)
            nrc_write_train_vertex(a, trainIdx, nrc_make_query(a, pos, frame.n, vOut, bsdf), o.localThroughput, kInvalidVertexDataIndex, 1, o.neeRet);
        else trainIdx = kInvalidVertexDataIndex;
    }
    else trainIdx = kInvalidVertexDataIndex;   // (never read for non-training paths)
    o.trainIdx = trainIdx;
    if (surface) static_cast<uint64_t*>(a.s.rngBuffer)[p] = rng.state;
    if (inImage) {
        a.state[2 * p] = make_float4(alpha.x, alpha.y, alpha.z, dirPDensity);
        a.state[2 * p + 1] = make_float4(contribution.x, contribution.y, contribution.z, 0.0f);
        a.nrcState[2 * p] = make_float4(o.localThroughput.x, o.localThroughput.y, o.localThroughput.z, primaryPathSpread);
        a.nrcState[2 * p + 1] = make_float4(0.0f, bits2f(trainIdx), bits2f(0u), 0.0f);
        if (!o.wantExt) {
            NrcTile t = tile;
            if (!surface) t.training = false;      // the suffix terminal is only written inside the surface branch (:344-350)
            nrc_end_path(a, static_cast<uint32_t>(p), t, 0u, trainIdx, 1);
            if (!surface)   // ... but the terminal info of a background pixel still records the tile flags (:365-372)
                static_cast<float4*>(a.nrc.inferenceTerminalInfoBuffer)[p] =
                    make_float4(0.0f, 0.0f, 0.0f, bits2f(nrc_terminal_bits(false, 1, tile.training, tile.unbiased)));
        }
    }
    push_vertex(a, static_cast<uint32_t>(p), pos, o);
}

// pathTrace_closestHit_generic<true> / pathTrace_miss_generic<true> for one extension ray, then the
// loop head and, when the path stops, the tail of the ray-generation program (:380-677, :320-373).  REGIR: emitters
// found by BSDF sampling contribute nothing (the ReGIR NEE has no density to weight them against).
template <int NEE>
__global__ __launch_bounds__(kPtBlock) void k_nrc_pt_bounce(PtArgs a) {
    constexpr bool REGIR = NEE == 1;
    // NEE == 2: the first vertex's direct light came from the ReSTIR reservoir, which has no density to weight a BSDF-sampled emitter
    // against: what the first extension ray finds emitting counts nothing (GFX_PT_PATH_TRACE_NRC_RESTIR, include/gfxexp.h)
    const bool noImplicit = REGIR || (NEE == 2 && a.pathLength == 2);
    const uint32_t i = blockIdx.x * kPtBlock + threadIdx.x;
    const uint32_t count = *a.extCountIn;
    const uint32_t bufIdx = a.f.bufferIndex;
    const size_t numPixels = static_cast<size_t>(a.s.imageSizeX) * a.s.imageSizeY;
    PtVertexOut o;
    reset_vertex_out(o);
    f3 pos(0.0f), vOutLocal(0.0f), vOut(0.0f);
    Frame frame(f3(0, 0, 1), f3(1, 0, 0));
    Bsdf bsdf; bsdf.type = 0; bsdf.diffuse = f3(0.0f); bsdf.specularF0 = f3(0.0f); bsdf.roughness = 1.0f;
    Pcg32 rng; rng.state = 0;
    const EnvMap env = load_env(a.s);
    const bool envEnabled = env.present() && a.f.enableEnvLight;
    f3 alpha(0.0f), contribution(0.0f), prevLocalThroughput(0.0f);
    float dirPDensity = 0.0f, primaryPathSpread = 0.0f, curSqrtPathSpread = 0.0f;
    uint32_t pixel = 0, prevTrainIdx = kInvalidVertexDataIndex, flags = 0;
    NrcTile tile; tile.linearTileIndex = 0; tile.training = false; tile.unbiased = false;
    const uint32_t pathLength = a.pathLength;
    bool active = i < count, hitSurface = false, shade = false;
    if (active) {
        pixel = a.extOwnerIn[i];
        tile = nrc_tile_of(a, pixel);
        const gfx_hit h = a.hits[i];
        const float4 ro4 = a.extOrgIn[i], rd4 = a.extDirIn[i];
        const f3 rayOrg(ro4.x, ro4.y, ro4.z), rayDir(rd4.x, rd4.y, rd4.z);
        const float4 s0 = a.state[2ull * pixel], s1 = a.state[2ull * pixel + 1];
        const float4 n0 = a.nrcState[2ull * pixel], n1 = a.nrcState[2ull * pixel + 1];
        alpha = f3(s0.x, s0.y, s0.z);
        const float prevDirPDensity = s0.w;
        dirPDensity = prevDirPDensity;
        contribution = f3(s1.x, s1.y, s1.z);
        prevLocalThroughput = f3(n0.x, n0.y, n0.z); primaryPathSpread = n0.w;
        curSqrtPathSpread = n1.x; prevTrainIdx = f2bits(n1.y); flags = f2bits(n1.z);
        float* prevTarget = static_cast<float*>(a.nrc.trainTargetBuffer[0]) + 3ull * prevTrainIdx;
        const bool linkPrev = tile.training && prevTrainIdx != kInvalidVertexDataIndex;
        if (h.triIndex == GFX_INVALID_SLOT) {
            if (envEnabled && !noImplicit) {
                f3 luminance;
                float misWeight;
                // 0.25 whether or not an instance emits, where pt_next_setup has 1 without one: the difference is the reference's
                pt_miss_environment(a, env, rayDir, prevDirPDensity, 0.25f, luminance, misWeight);
                const f3 implicit = misWeight * luminance;
                contribution = contribution + alpha * implicit;
                if (linkPrev) {
                    const f3 add = prevLocalThroughput * implicit;
                    prevTarget[0] += add.x; prevTarget[1] += add.y; prevTarget[2] += add.z;
                }
            }
        }
        else {
            hitSurface = true;
            PtSurface sp;
            pt_hit_surface<REGIR>(a, h, rayOrg, envEnabled, sp);
            const float hypAreaPDensity = sp.hypAreaPDensity;
            const gfx_material& mat = a.scene.materials[sp.materialSlot];
            vOut = unit(-rayDir);
            const float frontHit = dot(vOut, sp.ng) >= 0.0f ? 1.0f : -1.0f;
            const float tu = sp.tu(), tv = sp.tv();
            frame = Frame(sp.ns, sp.tc0);
            if (a.f.enableBumpMapping) apply_bump_mapping(read_modified_normal(a.scene, mat, tu, tv), frame);
            pos = offset_ray_origin(sp.pos, frontHit * sp.ng);
            vOutLocal = frame.to_local(vOut);
            const float dist2 = len2(rayOrg - pos);
            curSqrtPathSpread += sqrtf(dist2 / (prevDirPDensity * fabsf(vOutLocal.z)));
            if (!noImplicit && vOutLocal.z > 0 && mat.hasEmittance) {
                const f3 emittance = material_emittance(a.scene, mat, tu, tv);
                const float lightPDensity = hypAreaPDensity * dist2 / vOutLocal.z;
                const float misWeight = (prevDirPDensity * prevDirPDensity) / (prevDirPDensity * prevDirPDensity + lightPDensity * lightPDensity);
                const f3 implicit = emittance * (misWeight / kPi);
                contribution = contribution + alpha * implicit;
                if (linkPrev) {
                    const f3 add = prevLocalThroughput * implicit;
                    prevTarget[0] += add.x; prevTarget[1] += add.y; prevTarget[2] += add.z;
                }
            }
            rng.state = static_cast<const uint64_t*>(a.s.rngBuffer)[pixel];
            // Russian roulette (:455-474)
            bool performRR = true, terminatedByRR = false, stop = false;
            float recContinueProb = 1.0f;
            if (tile.training) performRR = pathLength > 2;
            const bool unbiasedSuffix = (flags & kNrcFlagRenderEnds) && tile.training && tile.unbiased;
            if (performRR) {
                const float continueProb = fminf(luminance_srgb(alpha) / luminance_srgb(f3(1.0f)), 1.0f);
                if (rng.uniform() >= continueProb || a.maxLengthTerminate) {
                    if (unbiasedSuffix) stop = true;
                    terminatedByRR = true;
                }
                recContinueProb = 1.0f / continueProb;
            }
            bsdf.setup(a.scene, mat, tu, tv);
            if (!stop) {   // cache termination heuristic (:479-538)
                bool endsWithCache = curSqrtPathSpread * curSqrtPathSpread > 0.01f * primaryPathSpread;
                if (unbiasedSuffix) endsWithCache = false;
                if (endsWithCache) {
                    const NrcQuery q = nrc_make_query(a, pos, frame.n, vOut, bsdf);
                    if (!(flags & kNrcFlagRenderEnds)) {
                        nrc_store_query(a.nrc.inferenceRadianceQueryBuffer, pixel, q);
                        static_cast<float4*>(a.nrc.inferenceTerminalInfoBuffer)[pixel] =
                            make_float4(alpha.x, alpha.y, alpha.z, bits2f(nrc_terminal_bits(true, pathLength, tile.training, tile.unbiased)));
                        flags |= kNrcFlagRenderEnds;
                        if (tile.training) curSqrtPathSpread = 0;
                        else stop = true;
                    }
                    else {
                        if (!(flags & kNrcFlagSuffixEnds)) {
                            nrc_store_query(a.nrc.inferenceRadianceQueryBuffer, numPixels + tile.linearTileIndex, q);
                            static_cast<uint32_t*>(a.nrc.trainSuffixTerminalInfoBuffer)[tile.linearTileIndex] = nrc_suffix_bits(prevTrainIdx, true, pathLength);
                            flags |= kNrcFlagSuffixEnds;
                        }
                        stop = true;
                    }
                }
            }
            if (!stop && terminatedByRR) stop = true;
            if (!stop) {
                alpha = alpha * recContinueProb;
                if (linkPrev) {
                    float4* vi = static_cast<float4*>(a.nrc.trainVertexInfoBuffer) + prevTrainIdx;
                    float4 v = *vi;
                    v.x *= recContinueProb; v.y *= recContinueProb; v.z *= recContinueProb;
                    *vi = v;
                }
                shade = true;
            }
        }
    }
    shade_vertex<REGIR, false>(a, shade, env, envEnabled, pos, vOutLocal, frame, bsdf, rng, alpha, contribution, dirPDensity, o);
    // training record of this vertex (:574-631)
    const bool wantRecord = shade && tile.training && !(flags & kNrcFlagSuffixEnds);
    uint32_t trainIdx = nrc_alloc_train_index(static_cast<uint32_t*>(a.nrc.numTrainingData[bufIdx]), wantRecord);
    if (wantRecord) {
        const NrcQuery q = nrc_make_query(a, pos, frame.n, vOut, bsdf);
        if (trainIdx < kTrainBufferSize) {
            nrc_write_train_vertex(a, trainIdx, q, o.localThroughput, prevTrainIdx, pathLength, o.neeRet);
            prevTrainIdx = trainIdx;
            o.trainIdx = trainIdx;
        }
        else {
            nrc_store_query(a.nrc.inferenceRadianceQueryBuffer, numPixels + tile.linearTileIndex, q);
            static_cast<uint32_t*>(a.nrc.trainSuffixTerminalInfoBuffer)[tile.linearTileIndex] = nrc_suffix_bits(prevTrainIdx, true, pathLength);
            flags |= kNrcFlagSuffixEnds;
        }
    }
    if (shade) prevLocalThroughput = o.localThroughput;
    if (active) {
        if (hitSurface) {
            static_cast<uint64_t*>(a.s.rngBuffer)[pixel] = rng.state;
            a.state[2ull * pixel] = make_float4(alpha.x, alpha.y, alpha.z, dirPDensity);
        }
        a.state[2ull * pixel + 1] = make_float4(contribution.x, contribution.y, contribution.z, 0.0f);
        a.nrcState[2ull * pixel] = make_float4(prevLocalThroughput.x, prevLocalThroughput.y, prevLocalThroughput.z, primaryPathSpread);
        a.nrcState[2ull * pixel + 1] = make_float4(curSqrtPathSpread, bits2f(prevTrainIdx), bits2f(flags), 0.0f);
        if (!o.wantExt) nrc_end_path(a, pixel, tile, flags, prevTrainIdx, pathLength);
    }
    push_vertex(a, pixel, pos, o);
}

// numInferenceQueries of the frame on the device (neural_radiance_caching_main.cpp:2293-2303 does this on the host)
__global__ void k_nrc_count_queries(PtArgs a, uint32_t* out) {
    const uint2 ts = *static_cast<const uint2*>(a.nrc.tileSize[a.f.bufferIndex]);
    const uint32_t W = static_cast<uint32_t>(a.s.imageSizeX), H = static_cast<uint32_t>(a.s.imageSizeY);
    const uint32_t n = W * H + ((W + ts.x - 1) / ts.x) * ((H + ts.y - 1) / ts.y);
    *out = (n + 127u) / 128u * 128u;
}

// perFrameContributionBuffer = contribution (:375)
__global__ __launch_bounds__(kPtBlock) void k_nrc_pt_finish(PtArgs a) {
    const PixelId px = pixel_of_thread(a.px);
    if (!px.valid) return;
    const size_t p = px.p;
    const float4 c = a.state[2 * p + 1];
    float* dst = static_cast<float*>(a.nrc.perFrameContributionBuffer) + 3 * p;
    dst[0] = c.x; dst[1] = c.y; dst[2] = c.z;
}

GFX_DEV f3 nrc_scaled_prediction(const PtArgs& a, size_t entry) {
    const float* r = static_cast<const float*>(a.nrc.inferredRadianceBuffer) + 3 * entry;
    f3 radiance(fmax2(r[0], 0.0f), fmax2(r[1], 0.0f), fmax2(r[2], 0.0f));
    if (a.nrc.radianceScale > 0) radiance = radiance / a.nrc.radianceScale;
    const float* q = static_cast<const float*>(a.nrc.inferenceRadianceQueryBuffer) + 14 * entry;
    return radiance * f3(q[8] + q[11], q[9] + q[12], q[10] + q[13]);
}

// accumulateInferredRadianceValues, nrc_setup_kernels.cu:51-93
__global__ __launch_bounds__(kPtBlock) void k_nrc_accumulate(PtArgs a) {
    const PixelId px = pixel_of_thread(a.px);
    if (!px.valid) return;
    const size_t p = px.p;
    const float4 t = static_cast<const float4*>(a.nrc.inferenceTerminalInfoBuffer)[p];
    const float* d = static_cast<const float*>(a.nrc.perFrameContributionBuffer) + 3 * p;
    const f3 directCont(d[0], d[1], d[2]);
    f3 radiance(0.0f);
    if (f2bits(t.w) & 1u) radiance = nrc_scaled_prediction(a, p);
    const f3 contribution = directCont + f3(t.x, t.y, t.z) * radiance;
    float4* beauty = static_cast<float4*>(a.s.beautyAccumBuffer) + p;
    f3 prev(0.0f);
    if (a.f.numAccumFrames > 0) { const float4 b = *beauty; prev = f3(b.x, b.y, b.z); }
    const float curWeight = 1.0f / (1 + a.f.numAccumFrames);
    const f3 result = (1 - curWeight) * prev + curWeight * contribution;
    *beauty = make_float4(result.x, result.y, result.z, 1.0f);
}

// propagateRadianceValues, nrc_setup_kernels.cu:95-137
__global__ __launch_bounds__(kPtBlock) void k_nrc_propagate(PtArgs a) {
    const uint32_t i = blockIdx.x * kPtBlock + threadIdx.x;
    if (i >= a.nrc.maxNumTrainingSuffixes) return;
    const uint32_t bits = static_cast<const uint32_t*>(a.nrc.trainSuffixTerminalInfoBuffer)[i];
    uint32_t last = bits & 0x7FFFFFu;
    if (last == kInvalidVertexDataIndex) return;
    f3 contribution(0.0f);
    if ((bits >> 23) & 1u) contribution = nrc_scaled_prediction(a, static_cast<size_t>(a.s.imageSizeX) * a.s.imageSizeY + i);
    while (last != kInvalidVertexDataIndex) {
        const float4 vi = static_cast<const float4*>(a.nrc.trainVertexInfoBuffer)[last];
        float* t = static_cast<float*>(a.nrc.trainTargetBuffer[0]) + 3ull * last;
        contribution = f3(t[0], t[1], t[2]) + f3(vi.x, vi.y, vi.z) * contribution;
        const float* q = static_cast<const float*>(a.nrc.trainRadianceQueryBuffer[0]) + 14ull * last;
        const f3 ref(q[8] + q[11], q[9] + q[12], q[10] + q[13]);
        t[0] = ref.x != 0 ? contribution.x / ref.x : 0.0f;
        t[1] = ref.y != 0 ? contribution.y / ref.y : 0.0f;
        t[2] = ref.z != 0 ? contribution.z / ref.z : 0.0f;
        last = f2bits(vi.w) & 0x7FFFFFu;
    }
}

GFX_DEV int32_t float_to_ordered_int(float f) { const int32_t i = static_cast<int32_t>(f2bits(f)); return i >= 0 ? i : i ^ 0x7FFFFFFF; }

// shuffleTrainingData, nrc_setup_kernels.cu:139-216 (one thread per destination candidate, 65536 threads)
__global__ __launch_bounds__(kPtBlock) void k_nrc_shuffle(PtArgs a) {
    const uint32_t i = blockIdx.x * kPtBlock + threadIdx.x;
    const uint32_t bufIdx = a.f.bufferIndex;
    const uint32_t numTrainingData = *static_cast<const uint32_t*>(a.nrc.numTrainingData[bufIdx]);
    float* dstQ = static_cast<float*>(a.nrc.trainRadianceQueryBuffer[1]);
    float* dstT = static_cast<float*>(a.nrc.trainTargetBuffer[1]);
    if (numTrainingData == 0) {
        for (int k = 0; k < 14; ++k) dstQ[14ull * i + k] = 0.0f;
        dstT[3ull * i] = 0.0f; dstT[3ull * i + 1] = 0.0f; dstT[3ull * i + 2] = 0.0f;
        return;
    }
    uint32_t* shuffler = static_cast<uint32_t*>(a.nrc.dataShufflerBuffer) + i;
    const uint32_t state = (*shuffler * 1103515245u + 12345u) % (1u << 31);    // LinearCongruentialGenerator, :164-181
    *shuffler = state;
    const uint32_t dstIdx = state % kNumTrainingDataPerFrame;
    const uint32_t srcIdx = i % numTrainingData;
    const float* sq = static_cast<const float*>(a.nrc.trainRadianceQueryBuffer[0]) + 14ull * srcIdx;
    const float* st = static_cast<const float*>(a.nrc.trainTargetBuffer[0]) + 3ull * srcIdx;
    float q[14];
    bool valid = true;
#pragma unroll
    for (int k = 0; k < 14; ++k) { q[k] = sq[k]; valid = valid && is_finite(q[k]); }
    if (!valid) for (int k = 0; k < 14; ++k) q[k] = 0.0f;
    f3 target(st[0], st[1], st[2]);
    if (!all_finite(target)) target = f3(0.0f);
    // statistics (min / max exact; the average accumulates in arrival order)
    int32_t* mm = static_cast<int32_t*>(a.nrc.targetMinMax[bufIdx]);
    float* avg = static_cast<float*>(a.nrc.targetAvg[bufIdx]);
    const float c[3] = { target.x, target.y, target.z };
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int32_t lo = float_to_ordered_int(c[k]), hi = lo;
        float sum = c[k] / kNumTrainingDataPerFrame;
        for (int off = 32; off >= 1; off >>= 1) {
            lo = min(lo, __shfl_xor(lo, off)); hi = max(hi, __shfl_xor(hi, off)); sum += __shfl_xor(sum, off);
        }
        if ((threadIdx.x & 63) == 0) { atomicMin(mm + k, lo); atomicMax(mm + 3 + k, hi); atomicAdd(avg + k, sum); }
    }
    if (a.nrc.radianceScale > 0) target = target * a.nrc.radianceScale;
    target = f3(fmin2(target.x, 1e+6f), fmin2(target.y, 1e+6f), fmin2(target.z, 1e+6f));
#pragma unroll
    for (int k = 0; k < 14; ++k) dstQ[14ull * dstIdx + k] = q[k];
    dstT[3ull * dstIdx] = target.x; dstT[3ull * dstIdx + 1] = target.y; dstT[3ull * dstIdx + 2] = target.z;
}

// visualizePrediction ray generation, optix_pathtracing_kernels.cu:705-778
__global__ __launch_bounds__(kPtBlock) void k_nrc_visualize(PtArgs a) {
    const size_t p = static_cast<size_t>(blockIdx.x) * kPtBlock + threadIdx.x;
    if (p >= static_cast<size_t>(a.s.imageSizeX) * a.s.imageSizeY) return;
    const uint4 g0 = static_cast<const uint4*>(a.s.gbuffer0[a.f.bufferIndex])[p];
    const bool surface = g0.x != 0xFFFFFFFFu;
    if (surface) {
        const PtSurface sp = pt_gbuffer_surface(a, g0);
        const Camera cam = load_camera(a.f.camera);
        const f3 vOut = unit(cam.pos - sp.pos);
        const float frontHit = dot(vOut, sp.ng) >= 0.0f ? 1.0f : -1.0f;
        const f3 pos = offset_ray_origin(sp.pos, frontHit * sp.ng);
        const gfx_material& mat = a.scene.materials[sp.materialSlot];
        const float tu = sp.tu(), tv = sp.tv();
        Frame frame(sp.ns, sp.tc0);
        if (a.f.enableBumpMapping) apply_bump_mapping(read_modified_normal(a.scene, mat, tu, tv), frame);
        Bsdf bsdf; bsdf.setup(a.scene, mat, tu, tv);
        nrc_store_query(a.nrc.inferenceRadianceQueryBuffer, p, nrc_make_query(a, pos, frame.n, vOut, bsdf));
    }
    static_cast<float4*>(a.nrc.inferenceTerminalInfoBuffer)[p] = make_float4(1.0f, 1.0f, 1.0f, bits2f(nrc_terminal_bits(surface, 1, false, false)));
}

} // namespace gfx
