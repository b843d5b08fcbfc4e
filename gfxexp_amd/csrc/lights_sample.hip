// lights_sample.hip -- test / inspection entry of the light sampler (shading.hip.h): draws light samples from a list of
// (ul, u0, u1) with exactly the functions the passes call (sample_light, light_select_search + light_fetch,
// sample_light_solid_angle) and reports which emitter record each one picked.
#include "internal.h"
#include "shading.hip.h"

namespace gfx {

template <bool EMITTER_TEX>
__global__ void k_lights_sample(DevScene sc, int mode, float3 shadingPoint, const float4* __restrict__ u, uint32_t n, float4* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 r = u[i];
    const EnvMap env{};
    LightSample ls;
    ls.emittance = f3(0.0f); ls.position = f3(0.0f); ls.normal = f3(0.0f); ls.atInfinity = 0;
    float pd = 0.0f;
    // the selection on its own, for the record index (the samplers below repeat it: same function, same ul)
    const LightPick pk = mode == GFX_LIGHTS_SAMPLE ? light_select(sc, r.x) : light_select_search(sc, r.x);
    if (mode == GFX_LIGHTS_SAMPLE) sample_light<EMITTER_TEX>(sc, env, 0.0f, 0.0f, r.x, false, r.y, r.z, ls, pd);
    else if (mode == GFX_LIGHTS_SAMPLE_SOLID_ANGLE) sample_light_solid_angle(sc, env, 0.0f, 0.0f, f3(shadingPoint.x, shadingPoint.y, shadingPoint.z), r.x, false, r.y, r.z, ls, pd);
    else if (pk.ok) light_fetch<EMITTER_TEX>(sc, pk, r.y, r.z, ls, pd);
    float4* o = out + 4ull * i;
    o[0] = make_float4(ls.emittance.x, ls.emittance.y, ls.emittance.z, pd);
    o[1] = make_float4(ls.position.x, ls.position.y, ls.position.z, bits2f(ls.atInfinity));
    o[2] = make_float4(ls.normal.x, ls.normal.y, ls.normal.z, bits2f(pk.ok ? pk.rec : 0xFFFFFFFFu));
    // the table's lookup returns the instance only out of a boundary cell of its guide (emitter_spans.h): read the record's span itself
    const uint32_t instSlot = !pk.ok ? 0xFFFFFFFFu : (pk.table ? sc.spans[pk.rec].instSlot : pk.instSlot);
    o[3] = make_float4(bits2f(instSlot), bits2f(pk.table ? 1u : 0u), 0.0f, 0.0f);
}

void lights_sample(Context& ctx, hipStream_t stream, int mode, const float shadingPoint[3], const void* dU, uint32_t n, void* dOut) {
    if (mode != GFX_LIGHTS_SAMPLE && mode != GFX_LIGHTS_SAMPLE_SEARCH && mode != GFX_LIGHTS_SAMPLE_SOLID_ANGLE) throw HipError("gfx_lights_sample: unknown mode");
    if (ctx.sceneDirty || !ctx.lightsStaticBuilt || !ctx.instDistValid || ctx.transformsDirty)
        throw HipError("gfx_lights_sample: the light distributions are not built for the current scene (gfx_lights_build_static, gfx_lights_build_instances)");
    if (!n) return;
    if (!dU || !dOut || ((reinterpret_cast<uintptr_t>(dU) | reinterpret_cast<uintptr_t>(dOut)) & 15u))
        throw HipError("gfx_lights_sample: the random-number and the output buffer must be 16-byte aligned");
    const float3 sp = shadingPoint ? make_float3(shadingPoint[0], shadingPoint[1], shadingPoint[2]) : make_float3(0.0f, 0.0f, 0.0f);
    const dim3 grid((n + 255) / 256), block(256);
    if (ctx.anyEmittanceTexture)
        hipLaunchKernelGGL(k_lights_sample<true>, grid, block, 0, stream, ctx.devScene(), mode, sp, static_cast<const float4*>(dU), n, static_cast<float4*>(dOut));
    else
        hipLaunchKernelGGL(k_lights_sample<false>, grid, block, 0, stream, ctx.devScene(), mode, sp, static_cast<const float4*>(dU), n, static_cast<float4*>(dOut));
    GFX_HIP(hipGetLastError());
}

} // namespace gfx
