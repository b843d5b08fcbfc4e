// taa.hip -- temporal anti-aliasing over a linear colour buffer (gfx_taa_apply, include/gfxexp.h).
//
// The TAA half of the reference's svgf/ output pass, applyAlbedoModulationAndTemporalAntiAliasing (svgf/gpu_kernels/svgf.cu:533-611)
// with reprojectPreviousAccumulation (:465-531), restated over a float4 colour and the output chain's flow.  It runs after gfx_denoise
// or directly on the beauty: the reference's enableSVGF and enableTemporalAA are independent switches.  Written fresh; line numbers
// cite the reference.
//
// SPECIFICATION (the kernel below and tests/taa_ref.cpp both follow this text; fp32, no contraction, IEEE division,
// a op b op c evaluated left to right):
//   mn(a, b) = a < b ? a : b;  mx(a, b) = a > b ? a : b            (spelled out: fminf / fmaxf may return either zero of (-0, +0))
//   cl(i, n) = i < 0 ? 0 : (i > n - 1 ? n - 1 : i)                  (edge clamp of a coordinate)
//   Inputs: C float4[W*H] (the current colour), F float2[W*H] (pixel centre minus previous position, in pixels, as gfx_denoise
//   reads it), the history Hp float4[W*H] the previous call wrote, isFirstFrame, N = historyLength 1..256.
// 1. Current: c = C[p].rgb at p = (x, y).  The output alpha is C[p].w (the reference writes 1; this chain copies alpha, as
//    gfx_denoise does).
// 2. Neighbourhood (svgf.cu:569-594): bMin = bMax = xMin = xMax = c; for i = -1..1 (rows), j = -1..1, skipping (0, 0):
//    v = C[(cl(x + j, W), cl(y + i, H))].rgb;  bMin.k = mn(bMin.k, v.k), bMax.k = mx(bMax.k, v.k); when i == 0 or j == 0 also
//    xMin.k = mn(xMin.k, v.k), xMax.k = mx(xMax.k, v.k).  nbMin.k = 0.5 * (bMin.k + xMin.k), nbMax.k = 0.5 * (bMax.k + xMax.k).
// 3. Reprojection (svgf.cu:465-531, for the flow convention): Px = (x + 0.5) - F[p].x, Py = (y + 0.5) - F[p].y.
//    Off screen unless 0 <= Px < W and 0 <= Py < H (a NaN is off screen).  Otherwise qx = (int)Px, qy = (int)Py (truncation),
//    fx = Px - (qx + 0.5), fy likewise; dx = fx < 0 ? -1 : 1, dy likewise (0 counts as +1); s = |fx|, t = |fy|;
//    taps h0 = Hp[(qx, qy)], h1 = Hp[(cl(qx + dx, W), qy)], h2 = Hp[(qx, cl(qy + dy, H))], h3 = Hp[(cl(qx + dx, W), cl(qy + dy, H))]
//    with weights w0 = (1 - s)(1 - t), w1 = s (1 - t), w2 = (1 - s) t, w3 = s t;
//    S.k = w0 h0.k + w1 h1.k + w2 h2.k + w3 h3.k, sw = w0 + w1 + w2 + w3; prev.k = sw != 0 ? S.k / sw : 0.
// 4. Blend: when isFirstFrame or off screen, out.rgb = c.  Otherwise h.k = mn(mx(prev.k, nbMin.k), nbMax.k),
//    a = 1 / float(N), b = 1 - a, out.k = b h.k + a c.k.
//    Deviation: the reference computes the off-screen flag and drops it, so a pixel that has just come on screen blends
//    clamp(0, nbMin, nbMax) = nbMin at weight 1 - 1/N, and a panning camera darkens a band along the leading edge; here such a
//    pixel outputs c.
// 5. History: out (all four channels) is what the next call reprojects.  The object keeps two buffers and swaps them.
//
// Kernel (one launch per call): k_taa, 16 x 16 workgroups; C of the workgroup plus a one-pixel edge-clamped halo (18 x 18 float4,
// 5 KiB) in LDS for step 2; the four history taps straight from global memory (neighbouring pixels share their lines); one write
// to the caller's output and one to the history.
//
// The flow TAA wants (gfx_restir_copy_taa_flow_to_linear, k_taa_flow): the G-buffer's motion vector is pixel centre minus the previous
// raster position of the point the pixel's primary ray hit.  Under enableJittering that ray runs through a random point of the pixel,
// so the vector carries the jitter offset (up to half a pixel), and a reprojection through it resamples the history at a random
// sub-pixel position every frame: a blur that accumulates over the history.  For pixels without a surface it projects the view
// direction as if it were a point (restir_di's miss program, optix_gbuffer_kernels.cu:205-221, :56-62).  k_taa_flow writes
// instead, per pixel, current minus previous raster position of the same point: for a surface, mv - ((x + 0.5) - cur) with cur the
// point's raster position under the current camera (the jitter offset removed); for background, the view direction's raster
// position under the current camera minus under the previous one, rotation only (svgf.cu:443-449); 0 under resetFlowBuffer.  Read
// as "pixel centre minus previous position", it is the motion of the pixel centre when the motion is locally a translation.
#include "taa.h"
#include "../pass_common.hip.h"
#include <cmath>

namespace gfx {

namespace {

constexpr int kTaaTile = 16;
constexpr int kTaaHalo = kTaaTile + 2;

struct TaaParams {
    int W, H;
    int first;
    float curWeight, prevWeight;    // 1 / N and 1 - 1 / N
};

GFX_DEV float taa_min(float a, float b) { return a < b ? a : b; }
GFX_DEV float taa_max(float a, float b) { return a > b ? a : b; }
GFX_DEV int taa_clamp(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

__global__ __launch_bounds__(kTaaTile * kTaaTile) void k_taa(TaaParams P, const float4* __restrict__ color, const float2* __restrict__ flow,
                                                             const float4* __restrict__ prev, float4* __restrict__ hist,
                                                             float4* __restrict__ out) {
    __shared__ float4 sC[kTaaHalo * kTaaHalo];
    const int bx0 = blockIdx.x * kTaaTile, by0 = blockIdx.y * kTaaTile;
    const int tid = threadIdx.y * kTaaTile + threadIdx.x;
    for (int k = tid; k < kTaaHalo * kTaaHalo; k += kTaaTile * kTaaTile) {
        const int gx = taa_clamp(bx0 - 1 + k % kTaaHalo, P.W), gy = taa_clamp(by0 - 1 + k / kTaaHalo, P.H);
        sC[k] = color[gy * P.W + gx];
    }
    __syncthreads();
    const int x = bx0 + static_cast<int>(threadIdx.x), y = by0 + static_cast<int>(threadIdx.y);
    if (x >= P.W || y >= P.H) return;
    const int p = y * P.W + x;
    // the tile holds C at clamped coordinates, so cell (x + j, y + i) is C[(cl(x + j), cl(y + i))]
    const int tc = (threadIdx.y + 1) * kTaaHalo + (threadIdx.x + 1);
    const float4 c = sC[tc];
    float4 o = c;
    bool blend = !P.first;
    float Px = 0.0f, Py = 0.0f;
    if (blend) {
        const float2 f = flow[p];
        Px = (static_cast<float>(x) + 0.5f) - f.x;
        Py = (static_cast<float>(y) + 0.5f) - f.y;
        blend = Px >= 0.0f && Px < static_cast<float>(P.W) && Py >= 0.0f && Py < static_cast<float>(P.H);
    }
    if (blend) {
        // step 3: four bilinear taps of the previous history
        const int qx = static_cast<int>(Px), qy = static_cast<int>(Py);
        const float fx = Px - (static_cast<float>(qx) + 0.5f), fy = Py - (static_cast<float>(qy) + 0.5f);
        const int ax = taa_clamp(qx + (fx < 0.0f ? -1 : 1), P.W), ay = taa_clamp(qy + (fy < 0.0f ? -1 : 1), P.H);
        const float s = fabsf(fx), t = fabsf(fy);
        const float w0 = (1.0f - s) * (1.0f - t), w1 = s * (1.0f - t), w2 = (1.0f - s) * t, w3 = s * t;
        const float4 h0 = prev[qy * P.W + qx], h1 = prev[qy * P.W + ax], h2 = prev[ay * P.W + qx], h3 = prev[ay * P.W + ax];
        const float sw = ((w0 + w1) + w2) + w3;
        float pr = ((w0 * h0.x + w1 * h1.x) + w2 * h2.x) + w3 * h3.x;
        float pg = ((w0 * h0.y + w1 * h1.y) + w2 * h2.y) + w3 * h3.y;
        float pb = ((w0 * h0.z + w1 * h1.z) + w2 * h2.z) + w3 * h3.z;
        if (sw != 0.0f) { pr = pr / sw; pg = pg / sw; pb = pb / sw; }
        else { pr = 0.0f; pg = 0.0f; pb = 0.0f; }
        // step 2: box and cross extrema of the 3 x 3 neighbourhood
        float bnr = c.x, bng = c.y, bnb = c.z, bxr = c.x, bxg = c.y, bxb = c.z;
        float cnr = c.x, cng = c.y, cnb = c.z, cxr = c.x, cxg = c.y, cxb = c.z;
#pragma unroll
        for (int i = -1; i <= 1; ++i) {
#pragma unroll
            for (int j = -1; j <= 1; ++j) {
                if (i == 0 && j == 0) continue;
                const float4 v = sC[tc + i * kTaaHalo + j];
                bnr = taa_min(bnr, v.x); bng = taa_min(bng, v.y); bnb = taa_min(bnb, v.z);
                bxr = taa_max(bxr, v.x); bxg = taa_max(bxg, v.y); bxb = taa_max(bxb, v.z);
                if (i == 0 || j == 0) {
                    cnr = taa_min(cnr, v.x); cng = taa_min(cng, v.y); cnb = taa_min(cnb, v.z);
                    cxr = taa_max(cxr, v.x); cxg = taa_max(cxg, v.y); cxb = taa_max(cxb, v.z);
                }
            }
        }
        const float lr = 0.5f * (bnr + cnr), lg = 0.5f * (bng + cng), lb = 0.5f * (bnb + cnb);
        const float ur = 0.5f * (bxr + cxr), ug = 0.5f * (bxg + cxg), ub = 0.5f * (bxb + cxb);
        // step 4
        const float hr = taa_min(taa_max(pr, lr), ur), hg = taa_min(taa_max(pg, lg), ug), hb = taa_min(taa_max(pb, lb), ub);
        o.x = P.prevWeight * hr + P.curWeight * c.x;
        o.y = P.prevWeight * hg + P.curWeight * c.y;
        o.z = P.prevWeight * hb + P.curWeight * c.z;
    }
    out[p] = o;
    hist[p] = o;
}

// raster position (pixels) of a world-space point (PerspectiveCamera::calcScreenPosition, restir_di_shared.h:51-59); `direction`:
// rotation only.  false when the point is not in front of the camera.
GFX_DEV bool taa_raster(const Camera& cam, f3 v, bool direction, float W, float H, float& rx, float& ry) {
    const f3 pv = mul(inverse(cam.ori), direction ? v : v - cam.pos);
    if (!(pv.z > 0.0f)) return false;
    const float ax = pv.x / pv.z, ay = pv.y / pv.z;
    const float h = 2 * gm_tan(cam.fovY / 2);
    const float w = cam.aspect * h;
    rx = (1 - (ax + 0.5f * w) / w) * W;
    ry = (1 - (ay + 0.5f * h) / h) * H;
    return true;
}

__global__ __launch_bounds__(kTaaTile * kTaaTile) void k_taa_flow(const gfx_gbuffer0* __restrict__ g0, const float2* __restrict__ g1,
                                                                  const float4* __restrict__ g2, gfx_camera curCam, gfx_camera prevCam,
                                                                  int W, int H, int reset, float2* __restrict__ flow) {
    const int p = blockIdx.x * (kTaaTile * kTaaTile) + threadIdx.x;
    if (p >= W * H) return;
    const int x = p % W, y = p / W;
    float2 f = make_float2(0.0f, 0.0f);
    if (!reset) {
        const Camera cur = load_camera(curCam);
        const float4 pw = g2[p];
        const f3 v(pw.x, pw.y, pw.z);
        const float fw = static_cast<float>(W), fh = static_cast<float>(H);
        float cx, cy;
        if (g0[p].instSlot == 0xFFFFFFFFu) {
            float px, py;
            // a direction behind the previous camera: a previous position left of the image (off screen for TAA and gfx_denoise)
            if (!taa_raster(load_camera(prevCam), v, true, fw, fh, px, py)) f = make_float2((static_cast<float>(x) + 0.5f) + 1.0f, 0.0f);
            else if (taa_raster(cur, v, true, fw, fh, cx, cy)) f = make_float2(cx - px, cy - py);
        } else if (taa_raster(cur, v, false, fw, fh, cx, cy)) {
            const float2 mv = g1[p];
            f = make_float2(mv.x - ((static_cast<float>(x) + 0.5f) - cx), mv.y - ((static_cast<float>(y) + 0.5f) - cy));
        } else {
            f = g1[p];
        }
    }
    flow[p] = f;
}

} // namespace

void restir_copy_taa_flow_to_linear(Context& ctx, hipStream_t stream, void* flow) {
    if (!ctx.restir.valid) throw HipError("gfx_restir_copy_taa_flow_to_linear: gfx_restir_set_params first");
    if (!flow) throw HipError("gfx_restir_copy_taa_flow_to_linear: null output");
    const gfx_restir_static_params& s = ctx.restir.s;
    const gfx_restir_frame_params& f = ctx.restir.f;
    const int n = s.imageSizeX * s.imageSizeY;
    if (n <= 0) return;
    const uint32_t b = f.bufferIndex;
    constexpr int kBlock = kTaaTile * kTaaTile;
    hipLaunchKernelGGL(k_taa_flow, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, static_cast<const gfx_gbuffer0*>(s.gbuffer0[b]),
                       static_cast<const float2*>(s.gbuffer1[b]), static_cast<const float4*>(s.gbuffer2[b]), f.camera, f.prevCamera,
                       static_cast<int>(s.imageSizeX), static_cast<int>(s.imageSizeY), f.resetFlowBuffer ? 1 : 0, static_cast<float2*>(flow));
    GFX_HIP(hipGetLastError());
}

void taa_init(TemporalAA& t, uint32_t width, uint32_t height, uint32_t historyLength) {
    if (!width || !height || width > 16384 || height > 16384) throw HipError("gfx_taa_create: size must be 1..16384 per side");
    if (historyLength < 1 || historyLength > kTaaMaxHistoryLength) throw HipError("gfx_taa_create: historyLength must be 1..256");
    t.width = width; t.height = height; t.historyLength = historyLength; t.cur = 0;
    const size_t bytes = static_cast<size_t>(width) * height * sizeof(float4);
    for (int k = 0; k < 2; ++k) {
        t.history[k].reserve(bytes);
        GFX_HIP(hipMemset(t.history[k].p, 0, bytes));
    }
    GFX_HIP(hipDeviceSynchronize());
}

void taa_release(TemporalAA& t) {
    for (int k = 0; k < 2; ++k) t.history[k].release();
}

void taa_apply(TemporalAA& t, hipStream_t stream, const void* color, const void* flow, bool isFirstFrame, void* out) {
    TaaParams P;
    P.W = static_cast<int>(t.width); P.H = static_cast<int>(t.height);
    P.first = isFirstFrame ? 1 : 0;
    P.curWeight = 1.0f / static_cast<float>(t.historyLength);
    P.prevWeight = 1.0f - P.curWeight;
    const uint32_t rd = t.cur, wr = t.cur ^ 1u;
    const dim3 grid((t.width + kTaaTile - 1) / kTaaTile, (t.height + kTaaTile - 1) / kTaaTile);
    hipLaunchKernelGGL(k_taa, grid, dim3(kTaaTile, kTaaTile), 0, stream, P, static_cast<const float4*>(color),
                       static_cast<const float2*>(flow), t.history[rd].as<const float4>(), t.history[wr].as<float4>(),
                       static_cast<float4*>(out));
    GFX_HIP(hipGetLastError());
    t.cur = wr;
}

} // namespace gfx
