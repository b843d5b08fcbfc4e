// math_eval.hip -- test / inspection entry of the deterministic math contract (gm_math.hip.h) and the 16-bit quantisers
// (shading.hip.h): evaluates one of them on a list of arguments with exactly the functions the passes call, and returns
// every result as bits.  One thread per element, no shared memory.
#include "internal.h"
#include "shading.hip.h"

namespace gfx {

__global__ void k_math_eval(int fn, const float4* __restrict__ a, const float4* __restrict__ b, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 A = a[i];
    uint32_t o0 = 0, o1 = 0, o2 = 0, o3 = 0;
    switch (fn) {
    case GFX_MATH_SINCOS: {
        float s, c;
        gm_sincos(A.x, s, c);
        o0 = f2bits(s); o1 = f2bits(c); o2 = f2bits(gm_tan(A.x)); o3 = f2bits(gm_sin(A.x));
    } break;
    case GFX_MATH_EXP: o0 = f2bits(gm_exp(A.x)); break;
    case GFX_MATH_ACOS: o0 = f2bits(gm_acos(A.x)); break;
    case GFX_MATH_ATAN: o0 = f2bits(gm_atan(A.x)); break;
    case GFX_MATH_ATAN2: o0 = f2bits(gm_atan2(A.x, A.y)); break;
    case GFX_MATH_SAT: o0 = static_cast<uint32_t>(f2i_sat(A.x)); o1 = f2u_sat(A.x); o2 = q16(A.x); break;
    case GFX_MATH_TO_POLAR: {
        float phi, theta;
        to_polar_yup(f3(A.x, A.y, A.z), phi, theta);
        o0 = f2bits(phi); o1 = f2bits(theta); o2 = encode_dir(f3(A.x, A.y, A.z));
    } break;
    case GFX_MATH_DECODE_DIR: {
        const f3 v = decode_dir(f2bits(A.x));
        o0 = f2bits(v.x); o1 = f2bits(v.y); o2 = f2bits(v.z);
    } break;
    case GFX_MATH_ENCODE_UV: o0 = encode_uv(A.x, A.y); break;
    case GFX_MATH_DECODE_UV: {
        float u, v;
        decode_uv(f2bits(A.x), u, v);
        o0 = f2bits(u); o1 = f2bits(v);
    } break;
    case GFX_MATH_ENCODE_BC: o0 = encode_bc(A.x); break;
    case GFX_MATH_DECODE_BC: o0 = f2bits(decode_bc(f2bits(A.x) & 0xFFFFu)); break;   // the G-buffer holds 16 bits
    case GFX_MATH_OFFSET_RAY_ORIGIN: {
        const float4 B = b[i];
        const f3 p = offset_ray_origin(f3(A.x, A.y, A.z), f3(B.x, B.y, B.z));
        o0 = f2bits(p.x); o1 = f2bits(p.y); o2 = f2bits(p.z);
    } break;
    }
    out[i] = o0;
    out[static_cast<size_t>(n) + i] = o1;
    out[2 * static_cast<size_t>(n) + i] = o2;
    out[3 * static_cast<size_t>(n) + i] = o3;
}

void math_eval(Context& ctx, hipStream_t stream, int fn, const void* dA, const void* dB, uint32_t n, void* dOut) {
    (void)ctx;
    if (fn < GFX_MATH_SINCOS || fn > GFX_MATH_OFFSET_RAY_ORIGIN) throw HipError("gfx_math_eval: unknown fn");
    if (!n) return;
    if (!dA || !dOut) throw HipError("gfx_math_eval: the argument and the output buffer must not be null");
    if (fn == GFX_MATH_OFFSET_RAY_ORIGIN && !dB) throw HipError("gfx_math_eval: GFX_MATH_OFFSET_RAY_ORIGIN needs the second argument buffer, which is null");
    if ((reinterpret_cast<uintptr_t>(dA) | reinterpret_cast<uintptr_t>(dB) | reinterpret_cast<uintptr_t>(dOut)) & 15u)
        throw HipError("gfx_math_eval: the argument buffers and the output buffer must be 16-byte aligned");
    const dim3 grid((n - 1) / 256 + 1), block(256);
    hipLaunchKernelGGL(k_math_eval, grid, block, 0, stream, fn, static_cast<const float4*>(dA), static_cast<const float4*>(dB), n, static_cast<uint32_t*>(dOut));
    GFX_HIP(hipGetLastError());
}

} // namespace gfx
