// bsdf_eval.hip -- test / inspection entry of the shading layer (shading.hip.h): the BSDFs, the hemisphere sampler, the shading frame
// with its bump mapping and the unshadowed direct-lighting term, evaluated on lists of arguments with exactly the functions the passes
// call; every result is returned as bits.  One thread per element, no shared memory.  The material is given per element as constants
// (all texture slots 0) and goes through Bsdf::setup here, so the SimplePBR derivation and the 0.999 clamp are part of what is run.
#include "internal.h"
#include "shading.hip.h"

namespace gfx {

namespace {
constexpr uint32_t kNeedMat = 1u, kNeedA = 2u, kNeedB = 4u, kNeedC = 8u;
// per gfx_bsdf_fn: the lists read and the number of result words (gfx_bsdf_eval_words)
constexpr uint32_t kNeeds[GFX_BSDF_FN_COUNT] = {
    kNeedMat, kNeedMat | kNeedA | kNeedB, kNeedMat | kNeedA | kNeedB, kNeedMat | kNeedA | kNeedB, kNeedMat | kNeedA,
    kNeedA, kNeedA, kNeedA | kNeedB | kNeedC, kNeedMat | kNeedA | kNeedB | kNeedC };
constexpr uint32_t kWords[GFX_BSDF_FN_COUNT] = { 8, 4, 4, 8, 4, 8, 8, 16, 12 };
constexpr uint32_t kMaxWords = 16;
}

GFX_DEV f3 xyz(float4 v) { return f3(v.x, v.y, v.z); }

GFX_DEV Bsdf bsdf_of(const float4* __restrict__ mat, uint32_t i) {
    const float4 m0 = mat[2 * static_cast<size_t>(i)], m1 = mat[2 * static_cast<size_t>(i) + 1];
    gfx_material m = {};                                   // every texture slot 0: the constants are the values
    m.bsdfType = f2bits(m0.x);
    m.a[0] = m0.y; m.a[1] = m0.z; m.a[2] = m0.w;
    m.b[0] = m1.x; m.b[1] = m1.y; m.b[2] = m1.z;
    m.smoothness = m1.w;
    const DevScene sc = {};                                // never read without a texture slot
    Bsdf b;
    b.setup(sc, m, 0.0f, 0.0f);
    return b;
}

__global__ void k_bsdf_eval(int fn, uint32_t words, const float4* __restrict__ mat, const float4* __restrict__ a, const float4* __restrict__ b,
                            const float4* __restrict__ c, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float o[kMaxWords];
#pragma unroll
    for (uint32_t k = 0; k < kMaxWords; ++k) o[k] = 0.0f;
    auto put3 = [&](int at, f3 v) { o[at] = v.x; o[at + 1] = v.y; o[at + 2] = v.z; };
    switch (fn) {
    case GFX_BSDF_SETUP: {
        const Bsdf bsdf = bsdf_of(mat, i);
        put3(0, bsdf.diffuse); put3(3, bsdf.specularF0); o[6] = bsdf.roughness;
    } break;
    case GFX_BSDF_EVALUATE: put3(0, bsdf_of(mat, i).evaluate(xyz(a[i]), xyz(b[i]))); break;
    case GFX_BSDF_PDF: o[0] = bsdf_of(mat, i).evaluate_pdf(xyz(a[i]), xyz(b[i])); break;
    case GFX_BSDF_SAMPLE: {
        const float4 u = b[i];
        f3 dir(0.0f); float pdf = 0.0f;                    // an early out of sample_throughput leaves the direction unwritten: reported as 0
        put3(0, bsdf_of(mat, i).sample_throughput(xyz(a[i]), u.x, u.y, dir, pdf));
        put3(3, dir); o[6] = pdf;
    } break;
    case GFX_BSDF_DHR: put3(0, bsdf_of(mat, i).dh_reflectance_estimate(xyz(a[i]))); break;
    case GFX_BSDF_COSINE_HEMISPHERE: {
        const float4 u = a[i];
        concentric_disk(u.x, u.y, o[0], o[1]);
        put3(2, cosine_hemisphere(u.x, u.y));
    } break;
    case GFX_BSDF_COORDINATE_SYSTEM: {
        f3 t, bt;
        make_coordinate_system(xyz(a[i]), t, bt);
        put3(0, t); put3(3, bt);
    } break;
    case GFX_BSDF_BUMP_FRAME: {
        const size_t j = 4 * static_cast<size_t>(i);
        Frame frame(xyz(a[i]), xyz(b[i]));
        apply_bump_mapping(xyz(c[j]), frame);
        const f3 probe = xyz(c[j + 1]);
        put3(0, frame.t); put3(3, frame.b); put3(6, frame.n);
        put3(9, frame.to_local(probe)); put3(12, frame.from_local(probe));
    } break;
    case GFX_BSDF_DIRECT_LIGHTING: {
        const size_t j = 4 * static_cast<size_t>(i);
        const float4 c0 = c[j], c1 = c[j + 1], c2 = c[j + 2], c3 = c[j + 3];
        const Bsdf bsdf = bsdf_of(mat, i);
        const f3 shadingPoint = xyz(a[i]);
        const Frame frame(xyz(c0), xyz(c1));
        LightSample ls;
        ls.emittance = xyz(c2); ls.position = xyz(c3); ls.normal = f3(c0.w, c1.w, c2.w); ls.atInfinity = f2bits(c3.w);
        const ShadowRay sr = shadow_ray(shadingPoint, ls);
        const f3 cont = direct_lighting(shadingPoint, xyz(b[i]), frame, bsdf, ls);
        put3(0, sr.dir); o[3] = sr.dist2; o[4] = sr.tmax;
        put3(5, cont); o[8] = target_weight(cont);
    } break;
    }
#pragma unroll
    for (uint32_t k = 0; k < kMaxWords; ++k)
        if (k < words) out[k * static_cast<size_t>(n) + i] = f2bits(o[k]);
}

uint32_t bsdf_eval_words(int fn) {
    if (fn < 0 || fn >= GFX_BSDF_FN_COUNT) throw HipError("gfx_bsdf_eval: unknown fn");
    return kWords[fn];
}

void bsdf_eval(Context& ctx, hipStream_t stream, int fn, const void* dMat, const void* dA, const void* dB, const void* dC, uint32_t n, void* dOut) {
    (void)ctx;
    const uint32_t words = bsdf_eval_words(fn);
    if (!n) return;
    const uint32_t needs = kNeeds[fn];
    if (!dOut) throw HipError("gfx_bsdf_eval: the output buffer must not be null");
    if ((needs & kNeedMat) && !dMat) throw HipError("gfx_bsdf_eval: this fn needs the material list, which is null");
    if ((needs & kNeedA) && !dA) throw HipError("gfx_bsdf_eval: this fn needs the first argument list, which is null");
    if ((needs & kNeedB) && !dB) throw HipError("gfx_bsdf_eval: this fn needs the second argument list, which is null");
    if ((needs & kNeedC) && !dC) throw HipError("gfx_bsdf_eval: this fn needs the extra argument list, which is null");
    if ((reinterpret_cast<uintptr_t>(dMat) | reinterpret_cast<uintptr_t>(dA) | reinterpret_cast<uintptr_t>(dB) | reinterpret_cast<uintptr_t>(dC) |
         reinterpret_cast<uintptr_t>(dOut)) & 15u)
        throw HipError("gfx_bsdf_eval: the argument lists and the output buffer must be 16-byte aligned");
    const dim3 grid((n - 1) / 256 + 1), block(256);
    hipLaunchKernelGGL(k_bsdf_eval, grid, block, 0, stream, fn, words, static_cast<const float4*>(dMat), static_cast<const float4*>(dA),
                       static_cast<const float4*>(dB), static_cast<const float4*>(dC), n, static_cast<uint32_t*>(dOut));
    GFX_HIP(hipGetLastError());
}

} // namespace gfx
