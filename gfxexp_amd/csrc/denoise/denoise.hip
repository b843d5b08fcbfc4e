// denoise.hip -- SVGF temporal denoiser over the linear output buffers (gfx_denoise, include/gfxexp.h).
//
// Stands in for the OptiX temporal denoiser of restir_di_main.cpp (:1400-1432, :2504-2533) with the open SVGF of the reference's
// svgf/ sample, restated over the inputs the OptiX call receives (beauty, albedo, normal, flow) plus an optional depth guide instead
// of svgf's GL raster G-buffer.  Written fresh; line numbers cite the reference.
//
// SPECIFICATION (the kernels below and tests/denoise_ref.cpp both follow this text; fp32, no contraction, IEEE division and sqrt,
// a op b op c evaluated left to right):
//   lum(v)      = 0.2126729 v.r + 0.7151522 v.g + 0.0721750 v.b                       (sRGB_calcLuminance)
//   E(num, den) = a = -num / den;  0 if !(a >= -80), gm_exp(a) otherwise
//   pw(x)       = x squared log2(sigmaN) times                                          (pow(x, sigmaN), sigmaN = 2^k)
//   dot(a, b)   = a.x b.x + a.y b.y + a.z b.z
//   bg(p)       = emissive given and emissive[p] != 0, or with depth: depth[p] == +inf; without: normal[p].xyz == 0
//                 (an emitting surface is background: its beauty carries emission that demodulation would blow up, see gfxexp.h)
//   guide(p)    = (normal.xyz, bg ? +inf : (with depth ? depth : 0)); a guide is background iff its w is +inf
// 1. Background pixel: output = beauty (all four channels); history lighting = 0, moments = 0, length = 0, guide as above.
// 2. Demodulate: L.k = a.k > 1e-3 ? c.k / a.k : c.k (c = beauty.rgb, a = albedo.rgb);  m = (lum(L), lum(L) * lum(L)).
// 3. Temporal (optix_pathtracing_kernels.cu:55-130, :354-364).  Unless isFirstFrame: fx = ((x + 0.5) - flow.x) - 0.5, fy likewise;
//    no tap unless -1 < fx < W and -1 < fy < H; x0 = floor(fx), s = fx - x0 (t, y0 likewise); taps in the order
//    (x0, y0) (1-s)(1-t), (x0+1, y0) s(1-t), (x0, y0+1) (1-s)t, (x0+1, y0+1) s t.  A tap q is accepted when it is on screen,
//    length_prev[q] > 0, dot(n_prev[q], n) > 0.85 and, with depth, |z_prev[q] - z| <= 0.1 z.  Accepted taps accumulate, in order,
//    sw += w; P.k += w L_prev.k; M.j += w m_prev.j; nf += w float(length_prev).  If sw > 0: P.k /= sw, M.j /= sw,
//    n = min(roundf(nf / sw) + 1, 255) (roundf: halves away from zero); else (and with isFirstFrame) n = 1.
//    If n > 1: alpha = max(1 / float(n), minAlpha), beta = 1 - alpha, L.k = beta P.k + alpha L.k, m.j = beta M.j + alpha m.j.
//    History: lighting = (L, 0), moments = m, length = n, guide.
// 4. Variance (svgf.cu:30-130): n >= 4: var = max(m.2 - m.1 m.1, 0).  n < 4 (only when numStages > 0): over the moments m' of
//    this frame's history, c3 = 0.383103 * 0.383103, S1 = c3 m.1, S2 = c3 m.2, sw = c3; for i = -3..3 (rows), j = -3..3, skipping
//    off-screen and the centre and background neighbours: w = ((h[j] h[i]) wz) wn (h = 0.00598 0.060626 0.241843 0.383103 ...),
//    S1 += w m'.1, S2 += w m'.2, sw += w; then var = max(S2/sw - (S1/sw)(S1/sw), 0).
//    wz = with depth E(|z_q - z|, sigmaZ |dzdx ox + dzdy oy| + 1e-6), 1 without; wn = pw(max(0, dot(n_q, n))); (ox, oy) = q - p.
//    Depth gradient (svgf.cu:91-97, :268-272): dx = x < W/2 ? 1 : -1 (integer W/2), hz = z at (clamp(x + dx), y), or z when that
//    pixel is background; dzdx = (hz - z) * dx; dzdy likewise with dy, rows.
// 5. A-trous stage i, step 2^i (svgf.cu:220-350), over (L, var) of the previous stage (stage 0: of steps 3 and 4):
//    sigma = sqrt(Sv / Svw) over the 3x3 neighbours at clamped coordinates, weights (1/4 1/2 1/4) x (1/4 1/2 1/4), w = hx hy,
//    background neighbours skipped (Sv += w var_q, Svw += w);  l = lum(L_p);
//    h_c = centre weight, sw = h_c, A.k = h_c L_p.k, V = (h_c h_c) var_p; for every other tap of the kernel table (row-major
//    order; Box3x3 all 1, Gauss3x3 1/16 1/8 1/4, Gauss5x5 k/256), at q = p + step offset: skip off-screen and background;
//    w = ((h wz) wn) wl with wl = E(|lum(L_q) - l|, sigmaL sigma + 1e-6);  A.k += w L_q.k; V += (w w) var_q; sw += w.
//    Result L.k = A.k / sw, var = V / (sw sw).  Stage 0 with feedbackStage = 1 writes its L into the history lighting.
// 6. Output (svgf.cu:378-611 without the TAA half; OPTIX_DENOISER_ALPHA_MODE_COPY): out.k = a.k > 1e-3 ? L.k * a.k : L.k,
//    out.w = beauty.w, with L of the last stage (of step 3 when numStages = 0); background pixels output the beauty.
//
// Kernels (launches per call: numStages + 2 at most)
//   k_dn_temporal           steps 1-3 and the variance of n >= 4; packs the 16-B guide record and the 16-B (L, var) record
//   k_dn_variance           the 7x7 fallback of pixels with n < 4 (skipped when numStages = 0)
//   k_dn_atrous<K, R, LAST> one stage; steps 1 and 2 read a (16 + 2R)^2 tile of both records from LDS, wider steps gather from
//                           L2; the last stage fuses step 6
//   k_dn_output             step 6 alone (numStages = 0)
#include "denoise.h"
#include "../gm_math.hip.h"
#include <cmath>

namespace gfx {

namespace {

constexpr int kDnBlock = 256;                 // 1-D kernels
constexpr int kDnTile = 16;                   // a-trous: 16 x 16 pixels per workgroup

struct DnParams {
    int W, H;
    int hasDepth;
    int sigmaNLog2;
    float sigmaZ, sigmaL, minAlpha;
};

GFX_DEV float dn_lum(float r, float g, float b) { return 0.2126729f * r + 0.7151522f * g + 0.0721750f * b; }
GFX_DEV float dn_weight(float num, float den) {
    const float a = -num / den;
    return !(a >= -80.0f) ? 0.0f : gm_exp(a);
}
GFX_DEV float dn_pow(float x, int k) {
    for (int i = 0; i < k; ++i) x = x * x;
    return x;
}
GFX_DEV float dn_dot(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
GFX_DEV float dn_max(float a, float b) { return a > b ? a : b; }   // spelled out: fmaxf may return either zero of (-0, +0)
GFX_DEV bool dn_bg(float4 guide) { return guide.w == INFINITY; }
GFX_DEV int dn_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
GFX_DEV float dn_demod(float c, float a) { return a > 1e-3f ? c / a : c; }
GFX_DEV float dn_remod(float l, float a) { return a > 1e-3f ? l * a : l; }

// step 6 for one pixel: re-modulated lighting, or the beauty itself for background
GFX_DEV float4 dn_output(bool bg, float4 L, float4 beauty, float4 albedo) {
    if (bg) return beauty;
    return make_float4(dn_remod(L.x, albedo.x), dn_remod(L.y, albedo.y), dn_remod(L.z, albedo.z), beauty.w);
}

struct DnHistory {
    float4* lighting; float2* moments; uint32_t* length; float4* guide;
};
struct DnHistoryIn {
    const float4* lighting; const float2* moments; const uint32_t* length; const float4* guide;
};

// ---------------------------------------------------------------- steps 1-4 (n >= 4)
__global__ __launch_bounds__(kDnBlock) void k_dn_temporal(DnParams P, const float4* __restrict__ beauty, const float4* __restrict__ albedo,
                                                          const float4* __restrict__ normal, const float2* __restrict__ flow,
                                                          const float* __restrict__ depth, const uint32_t* __restrict__ emissive,
                                                          int first, DnHistoryIn prev, DnHistory hist,
                                                          float4* __restrict__ lv) {
    const int p = blockIdx.x * kDnBlock + threadIdx.x;
    if (p >= P.W * P.H) return;
    const int x = p % P.W, y = p / P.W;
    const float4 nv = normal[p];
    const float z = P.hasDepth ? depth[p] : 0.0f;
    const bool bg = (emissive && emissive[p] != 0u) || (P.hasDepth ? z == INFINITY : (nv.x == 0.0f && nv.y == 0.0f && nv.z == 0.0f));
    const float4 g = make_float4(nv.x, nv.y, nv.z, bg ? INFINITY : z);
    hist.guide[p] = g;
    if (bg) {
        hist.lighting[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        hist.moments[p] = make_float2(0.0f, 0.0f);
        hist.length[p] = 0u;
        lv[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float4 c = beauty[p], a = albedo[p];
    float Lr = dn_demod(c.x, a.x), Lg = dn_demod(c.y, a.y), Lb = dn_demod(c.z, a.z);
    float m1 = dn_lum(Lr, Lg, Lb);
    float m2 = m1 * m1;
    uint32_t n = 1;
    if (!first) {
        const float2 f = flow[p];
        const float fx = ((static_cast<float>(x) + 0.5f) - f.x) - 0.5f;
        const float fy = ((static_cast<float>(y) + 0.5f) - f.y) - 0.5f;
        if (fx > -1.0f && fx < static_cast<float>(P.W) && fy > -1.0f && fy < static_cast<float>(P.H)) {
            const float flx = floorf(fx), fly = floorf(fy);
            const int x0 = static_cast<int>(flx), y0 = static_cast<int>(fly);
            const float s = fx - flx, t = fy - fly;
            const float wts[4] = {(1.0f - s) * (1.0f - t), s * (1.0f - t), (1.0f - s) * t, s * t};
            float sw = 0.0f, Pr = 0.0f, Pg = 0.0f, Pb = 0.0f, M1 = 0.0f, M2 = 0.0f, nf = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
                if (qx < 0 || qx >= P.W || qy < 0 || qy >= P.H) continue;
                const int q = qy * P.W + qx;
                const uint32_t len = prev.length[q];
                if (len == 0u) continue;
                const float4 gq = prev.guide[q];
                if (!(dn_dot(gq, g) > 0.85f)) continue;
                if (P.hasDepth && !(fabsf(gq.w - z) <= 0.1f * z)) continue;
                const float w = wts[k];
                const float4 lq = prev.lighting[q];
                const float2 mq = prev.moments[q];
                sw += w;
                Pr += w * lq.x; Pg += w * lq.y; Pb += w * lq.z;
                M1 += w * mq.x; M2 += w * mq.y;
                nf += w * static_cast<float>(len);
            }
            if (sw > 0.0f) {
                Pr /= sw; Pg /= sw; Pb /= sw; M1 /= sw; M2 /= sw;
                const uint32_t r = static_cast<uint32_t>(roundf(nf / sw)) + 1u;
                n = r < 255u ? r : 255u;
                if (n > 1u) {
                    const float alpha = dn_max(1.0f / static_cast<float>(n), P.minAlpha);
                    const float beta = 1.0f - alpha;
                    Lr = beta * Pr + alpha * Lr; Lg = beta * Pg + alpha * Lg; Lb = beta * Pb + alpha * Lb;
                    m1 = beta * M1 + alpha * m1; m2 = beta * M2 + alpha * m2;
                }
            }
        }
    }
    hist.lighting[p] = make_float4(Lr, Lg, Lb, 0.0f);
    hist.moments[p] = make_float2(m1, m2);
    hist.length[p] = n;
    lv[p] = make_float4(Lr, Lg, Lb, n >= 4u ? dn_max(m2 - m1 * m1, 0.0f) : 0.0f);
}

// depth gradient towards the image centre (svgf.cu:91-97): `gz(x, y)` returns the guide's depth at a clamped pixel
template <typename G>
GFX_DEV void dn_gradient(const DnParams& P, int x, int y, float z, G gz, float& dzdx, float& dzdy) {
    const int dx = x < P.W / 2 ? 1 : -1, dy = y < P.H / 2 ? 1 : -1;
    float hz = gz(dn_clamp(x + dx, P.W - 1), y);
    float vz = gz(x, dn_clamp(y + dy, P.H - 1));
    if (hz == INFINITY) hz = z;
    if (vz == INFINITY) vz = z;
    dzdx = (hz - z) * static_cast<float>(dx);
    dzdy = (vz - z) * static_cast<float>(dy);
}
GFX_DEV float dn_wz(const DnParams& P, float zq, float z, float dzdx, float dzdy, int ox, int oy) {
    if (!P.hasDepth) return 1.0f;
    return dn_weight(fabsf(zq - z), P.sigmaZ * fabsf(dzdx * static_cast<float>(ox) + dzdy * static_cast<float>(oy)) + 1e-6f);
}

// ---------------------------------------------------------------- step 4, n < 4: the 7x7 fallback (svgf.cu:60-115)
__global__ __launch_bounds__(kDnBlock) void k_dn_variance(DnParams P, DnHistoryIn hist, float4* __restrict__ lv) {
    const int p = blockIdx.x * kDnBlock + threadIdx.x;
    if (p >= P.W * P.H) return;
    const uint32_t n = hist.length[p];
    if (n == 0u || n >= 4u) return;
    const int x = p % P.W, y = p / P.W;
    const float h[7] = {0.00598f, 0.060626f, 0.241843f, 0.383103f, 0.241843f, 0.060626f, 0.00598f};
    const float4 g = hist.guide[p];
    const float2 m = hist.moments[p];
    float dzdx = 0.0f, dzdy = 0.0f;
    if (P.hasDepth) dn_gradient(P, x, y, g.w, [&](int qx, int qy) { return hist.guide[qy * P.W + qx].w; }, dzdx, dzdy);
    const float c3 = 0.383103f * 0.383103f;
    float S1 = c3 * m.x, S2 = c3 * m.y, sw = c3;
    for (int i = -3; i <= 3; ++i) {
        const int qy = y + i;
        if (qy < 0 || qy >= P.H) continue;
        for (int j = -3; j <= 3; ++j) {
            const int qx = x + j;
            if (qx < 0 || qx >= P.W || (i == 0 && j == 0)) continue;
            const int q = qy * P.W + qx;
            const float4 gq = hist.guide[q];
            if (dn_bg(gq)) continue;
            const float wz = dn_wz(P, gq.w, g.w, dzdx, dzdy, j, i);
            const float wn = dn_pow(dn_max(dn_dot(gq, g), 0.0f), P.sigmaNLog2);
            const float w = ((h[j + 3] * h[i + 3]) * wz) * wn;
            const float2 mq = hist.moments[q];
            S1 += w * mq.x; S2 += w * mq.y; sw += w;
        }
    }
    const float M1 = S1 / sw, M2 = S2 / sw;
    float4 r = lv[p];
    r.w = dn_max(M2 - M1 * M1, 0.0f);
    lv[p] = r;
}

// ---------------------------------------------------------------- step 5 (+ step 6 in the last stage)
template <int K> struct DnKernel;
template <> struct DnKernel<GFX_DENOISE_BOX3X3> {
    static constexpr int kRadius = 1;
    GFX_DEV static float h(int, int) { return 1.0f; }
};
template <> struct DnKernel<GFX_DENOISE_GAUSS3X3> {
    static constexpr int kRadius = 1;
    GFX_DEV static float h(int i, int j) {     // 1/16 1/8 1/16 / 1/8 1/4 1/8 / ...
        const int d = (i != 0) + (j != 0);
        return d == 0 ? 0.25f : (d == 1 ? 0.125f : 0.0625f);
    }
};
template <> struct DnKernel<GFX_DENOISE_GAUSS5X5> {
    static constexpr int kRadius = 2;
    GFX_DEV static float h(int i, int j) {     // (1 4 6 4 1)^T (1 4 6 4 1) / 256
        const float b[5] = {1.0f, 4.0f, 6.0f, 4.0f, 1.0f};
        return (b[i + 2] * b[j + 2]) / 256.0f;
    }
};

struct DnStageArgs {
    DnParams P;
    int step;
    const float4* __restrict__ lvIn;
    const float4* __restrict__ guide;
    float4* __restrict__ lvOut;            // not the last stage
    float4* __restrict__ feedback;         // stage 0 with feedbackStage: the history lighting; else null
    const float4* __restrict__ beauty;     // the last stage
    const float4* __restrict__ albedo;
    float4* __restrict__ out;
};

// R > 0: the workgroup's 16 x 16 pixels and an R-pixel halo (at clamped coordinates) in LDS; R = 0: every read from global memory
template <int K, int R, bool LAST>
__global__ __launch_bounds__(kDnTile * kDnTile) void k_dn_atrous(DnStageArgs A) {
    constexpr int TW = kDnTile + 2 * (R > 0 ? R : 0);
    constexpr int kTileCells = R > 0 ? TW * TW : 1;
    __shared__ float4 sLv[kTileCells];
    __shared__ float4 sGuide[kTileCells];
    const DnParams& P = A.P;
    const int bx0 = blockIdx.x * kDnTile, by0 = blockIdx.y * kDnTile;
    const int x = bx0 + static_cast<int>(threadIdx.x), y = by0 + static_cast<int>(threadIdx.y);
    if constexpr (R > 0) {
        const int tid = threadIdx.y * kDnTile + threadIdx.x;
        for (int c = tid; c < TW * TW; c += kDnTile * kDnTile) {
            const int gx = dn_clamp(bx0 - R + c % TW, P.W - 1), gy = dn_clamp(by0 - R + c / TW, P.H - 1);
            sLv[c] = A.lvIn[gy * P.W + gx];
            sGuide[c] = A.guide[gy * P.W + gx];
        }
        __syncthreads();
    }
    if (x >= P.W || y >= P.H) return;
    // (qx, qy) within R of (x, y) (or clamped into the image, which keeps it within the tile)
    auto lvAt = [&](int qx, int qy) -> float4 {
        if constexpr (R > 0) return sLv[(qy - by0 + R) * TW + (qx - bx0 + R)];
        else return A.lvIn[qy * P.W + qx];
    };
    auto guideAt = [&](int qx, int qy) -> float4 {
        if constexpr (R > 0) return sGuide[(qy - by0 + R) * TW + (qx - bx0 + R)];
        else return A.guide[qy * P.W + qx];
    };
    const int p = y * P.W + x;
    const float4 g = guideAt(x, y);
    if (dn_bg(g)) {
        if constexpr (LAST) A.out[p] = A.beauty[p];
        else A.lvOut[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float4 c = lvAt(x, y);
    const float l = dn_lum(c.x, c.y, c.z);
    float dzdx = 0.0f, dzdy = 0.0f;
    if (P.hasDepth) dn_gradient(P, x, y, g.w, [&](int qx, int qy) { return guideAt(qx, qy).w; }, dzdx, dzdy);
    // 3x3 Gaussian of the variance (svgf.cu:274-291)
    const float gk[3] = {0.25f, 0.5f, 0.25f};
    float Sv = 0.0f, Svw = 0.0f;
#pragma unroll
    for (int i = -1; i <= 1; ++i) {
        const int qy = dn_clamp(y + i, P.H - 1);
#pragma unroll
        for (int j = -1; j <= 1; ++j) {
            const int qx = dn_clamp(x + j, P.W - 1);
            if (dn_bg(guideAt(qx, qy))) continue;
            const float w = gk[j + 1] * gk[i + 1];
            Sv += w * lvAt(qx, qy).w;
            Svw += w;
        }
    }
    const float sigma = sqrtf(Sv / Svw);
    const float lden = P.sigmaL * sigma + 1e-6f;
    using Kern = DnKernel<K>;
    constexpr int KR = Kern::kRadius;
    const float hc = Kern::h(0, 0);
    float sw = hc, Ar = hc * c.x, Ag = hc * c.y, Ab = hc * c.z, V = (hc * hc) * c.w;
#pragma unroll
    for (int i = -KR; i <= KR; ++i) {
#pragma unroll
        for (int j = -KR; j <= KR; ++j) {
            if (i == 0 && j == 0) continue;
            const int ox = j * A.step, oy = i * A.step;
            const int qx = x + ox, qy = y + oy;
            if (qx < 0 || qx >= P.W || qy < 0 || qy >= P.H) continue;
            const float4 gq = guideAt(qx, qy);
            if (dn_bg(gq)) continue;
            const float wz = dn_wz(P, gq.w, g.w, dzdx, dzdy, ox, oy);
            const float wn = dn_pow(dn_max(dn_dot(gq, g), 0.0f), P.sigmaNLog2);
            const float4 q = lvAt(qx, qy);
            const float wl = dn_weight(fabsf(dn_lum(q.x, q.y, q.z) - l), lden);
            const float w = ((Kern::h(i, j) * wz) * wn) * wl;
            Ar += w * q.x; Ag += w * q.y; Ab += w * q.z;
            V += (w * w) * q.w;
            sw += w;
        }
    }
    const float4 L = make_float4(Ar / sw, Ag / sw, Ab / sw, V / (sw * sw));
    if (A.feedback) A.feedback[p] = make_float4(L.x, L.y, L.z, 0.0f);
    if constexpr (LAST) A.out[p] = dn_output(false, L, A.beauty[p], A.albedo[p]);
    else A.lvOut[p] = L;
}

// ---------------------------------------------------------------- step 6 alone (numStages = 0)
__global__ __launch_bounds__(kDnBlock) void k_dn_output(DnParams P, const float4* __restrict__ lv, const float4* __restrict__ guide,
                                                        const float4* __restrict__ beauty, const float4* __restrict__ albedo,
                                                        float4* __restrict__ out) {
    const int p = blockIdx.x * kDnBlock + threadIdx.x;
    if (p >= P.W * P.H) return;
    out[p] = dn_output(dn_bg(guide[p]), lv[p], beauty[p], albedo[p]);
}

// R: the LDS halo of stages with step <= 2 (the kernel's reach, and at least the 3x3 variance / gradient neighbours); 0 = gather from L2
template <int K, bool LAST>
void launch_stage(hipStream_t stream, const DnStageArgs& a, dim3 grid) {
    constexpr int KR = DnKernel<K>::kRadius;
    const dim3 block(kDnTile, kDnTile);
    if (a.step == 1) hipLaunchKernelGGL((k_dn_atrous<K, KR, LAST>), grid, block, 0, stream, a);
    else if (a.step == 2) hipLaunchKernelGGL((k_dn_atrous<K, 2 * KR, LAST>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((k_dn_atrous<K, 0, LAST>), grid, block, 0, stream, a);
}
template <bool LAST>
void launch_stage_kernel(hipStream_t stream, int kernel, const DnStageArgs& a, dim3 grid) {
    switch (kernel) {
    case GFX_DENOISE_GAUSS3X3: launch_stage<GFX_DENOISE_GAUSS3X3, LAST>(stream, a, grid); break;
    case GFX_DENOISE_GAUSS5X5: launch_stage<GFX_DENOISE_GAUSS5X5, LAST>(stream, a, grid); break;
    default: launch_stage<GFX_DENOISE_BOX3X3, LAST>(stream, a, grid); break;
    }
}

int log2_exact(float v) {
    for (int k = 0; k <= 10; ++k) if (v == static_cast<float>(1u << k)) return k;
    return -1;
}

} // namespace

void denoiser_default_settings(gfx_denoiser_settings* out) {
    out->numStages = 5;
    out->kernel = GFX_DENOISE_BOX3X3;
    out->feedbackStage = 1;
    out->sigmaZ = 1.0f;
    out->sigmaN = 128.0f;
    out->sigmaL = 4.0f;
    out->minAlpha = 0.2f;
}

void denoiser_check_settings(const gfx_denoiser_settings& st) {
    if (st.numStages > 5) throw HipError("gfx_denoiser: numStages must be 0..5");
    if (st.kernel > GFX_DENOISE_GAUSS5X5) throw HipError("gfx_denoiser: unknown kernel");
    if (st.feedbackStage > 1) throw HipError("gfx_denoiser: feedbackStage must be 0 or 1");
    if (log2_exact(st.sigmaN) < 0) throw HipError("gfx_denoiser: sigmaN must be a power of two 1..1024");
    if (!(st.sigmaZ > 0.0f) || !std::isfinite(st.sigmaZ) || !(st.sigmaL > 0.0f) || !std::isfinite(st.sigmaL))
        throw HipError("gfx_denoiser: sigmaZ and sigmaL must be positive and finite");
    if (!(st.minAlpha >= 0.0f && st.minAlpha <= 1.0f)) throw HipError("gfx_denoiser: minAlpha must be 0..1");
}

void denoiser_init(Denoiser& d, uint32_t width, uint32_t height, const gfx_denoiser_settings& st) {
    denoiser_check_settings(st);
    if (!width || !height || width > 16384 || height > 16384) throw HipError("gfx_denoiser_create: size must be 1..16384 per side");
    d.width = width; d.height = height; d.st = st; d.cur = 0;
    const size_t n = static_cast<size_t>(width) * height;
    for (int k = 0; k < 2; ++k) {
        d.lighting[k].reserve(n * sizeof(float4));
        d.moments[k].reserve(n * sizeof(float2));
        d.length[k].reserve(n * sizeof(uint32_t));
        d.guide[k].reserve(n * sizeof(float4));
        d.lv[k].reserve(n * sizeof(float4));
        // no history yet: every length 0
        GFX_HIP(hipMemset(d.length[k].p, 0, n * sizeof(uint32_t)));
        GFX_HIP(hipMemset(d.lighting[k].p, 0, n * sizeof(float4)));
        GFX_HIP(hipMemset(d.moments[k].p, 0, n * sizeof(float2)));
        GFX_HIP(hipMemset(d.guide[k].p, 0, n * sizeof(float4)));
    }
    GFX_HIP(hipDeviceSynchronize());
}

void denoiser_release(Denoiser& d) {
    for (int k = 0; k < 2; ++k) {
        d.lighting[k].release(); d.moments[k].release(); d.length[k].release(); d.guide[k].release(); d.lv[k].release();
    }
}

void denoise(Denoiser& d, hipStream_t stream, const gfx_denoiser_inputs& in, bool isFirstFrame, void* out) {
    const gfx_denoiser_settings& st = d.st;
    DnParams P;
    P.W = static_cast<int>(d.width); P.H = static_cast<int>(d.height);
    P.hasDepth = in.depth != nullptr;
    P.sigmaNLog2 = log2_exact(st.sigmaN);
    P.sigmaZ = st.sigmaZ; P.sigmaL = st.sigmaL; P.minAlpha = st.minAlpha;
    const uint32_t rd = d.cur, wr = d.cur ^ 1u;
    const DnHistoryIn prev{d.lighting[rd].as<const float4>(), d.moments[rd].as<const float2>(), d.length[rd].as<const uint32_t>(),
                           d.guide[rd].as<const float4>()};
    const DnHistory hist{d.lighting[wr].as<float4>(), d.moments[wr].as<float2>(), d.length[wr].as<uint32_t>(), d.guide[wr].as<float4>()};
    const DnHistoryIn histIn{hist.lighting, hist.moments, hist.length, hist.guide};
    const int n = P.W * P.H;
    const dim3 grid1((n + kDnBlock - 1) / kDnBlock);
    const float4* beauty = static_cast<const float4*>(in.beauty);
    const float4* albedo = static_cast<const float4*>(in.albedo);
    hipLaunchKernelGGL(k_dn_temporal, grid1, dim3(kDnBlock), 0, stream, P, beauty, albedo, static_cast<const float4*>(in.normal),
                       static_cast<const float2*>(in.flow), static_cast<const float*>(in.depth), static_cast<const uint32_t*>(in.emissive),
                       isFirstFrame ? 1 : 0, prev, hist,
                       d.lv[0].as<float4>());
    GFX_HIP(hipGetLastError());
    if (st.numStages == 0) {
        hipLaunchKernelGGL(k_dn_output, grid1, dim3(kDnBlock), 0, stream, P, d.lv[0].as<const float4>(), histIn.guide, beauty, albedo,
                           static_cast<float4*>(out));
        GFX_HIP(hipGetLastError());
    } else {
        hipLaunchKernelGGL(k_dn_variance, grid1, dim3(kDnBlock), 0, stream, P, histIn, d.lv[0].as<float4>());
        GFX_HIP(hipGetLastError());
        const dim3 grid2((d.width + kDnTile - 1) / kDnTile, (d.height + kDnTile - 1) / kDnTile);
        for (uint32_t i = 0; i < st.numStages; ++i) {
            DnStageArgs a;
            a.P = P;
            a.step = 1 << i;
            a.lvIn = d.lv[i & 1].as<const float4>();
            a.guide = histIn.guide;
            a.lvOut = d.lv[(i + 1) & 1].as<float4>();
            a.feedback = (i == 0 && st.feedbackStage) ? hist.lighting : nullptr;
            a.beauty = beauty; a.albedo = albedo;
            a.out = static_cast<float4*>(out);
            if (i + 1 == st.numStages) launch_stage_kernel<true>(stream, static_cast<int>(st.kernel), a, grid2);
            else launch_stage_kernel<false>(stream, static_cast<int>(st.kernel), a, grid2);
            GFX_HIP(hipGetLastError());
        }
    }
    d.cur = wr;
}

// ---------------------------------------------------------------- depth guide from the G-buffers
__global__ __launch_bounds__(kDnBlock) void k_copy_depth(const gfx_gbuffer0* __restrict__ g0, const gfx_gbuffer2* __restrict__ g2, float cx, float cy,
                                                         float cz, int n, float* __restrict__ depth) {
    const int p = blockIdx.x * kDnBlock + threadIdx.x;
    if (p >= n) return;
    if (g0[p].instSlot == 0xFFFFFFFFu) { depth[p] = INFINITY; return; }
    const float dx = g2[p].positionInWorld[0] - cx, dy = g2[p].positionInWorld[1] - cy, dz = g2[p].positionInWorld[2] - cz;
    depth[p] = sqrtf(dx * dx + dy * dy + dz * dz);
}

__global__ __launch_bounds__(kDnBlock) void k_copy_emissive(const gfx_gbuffer0* __restrict__ g0, const uint4* __restrict__ g3,
                                                            const gfx_material* __restrict__ materials, uint32_t numMaterials, int n,
                                                            uint32_t* __restrict__ emissive) {
    const int p = blockIdx.x * kDnBlock + threadIdx.x;
    if (p >= n) return;
    const uint32_t mat = g3[p].w;      // gfx_gbuffer3.matSlot
    emissive[p] = (g0[p].instSlot != 0xFFFFFFFFu && mat < numMaterials && materials[mat].hasEmittance) ? 1u : 0u;
}

void restir_copy_emissive_to_linear(Context& ctx, hipStream_t stream, void* emissive) {
    if (!ctx.restir.valid) throw HipError("gfx_restir_copy_emissive_to_linear: gfx_restir_set_params first");
    if (!emissive) throw HipError("gfx_restir_copy_emissive_to_linear: null output");
    const gfx_restir_static_params& s = ctx.restir.s;
    const int n = s.imageSizeX * s.imageSizeY;
    if (n <= 0) return;
    const uint32_t b = ctx.restir.f.bufferIndex;
    const DevScene sc = ctx.devScene();
    hipLaunchKernelGGL(k_copy_emissive, dim3((n + kDnBlock - 1) / kDnBlock), dim3(kDnBlock), 0, stream, static_cast<const gfx_gbuffer0*>(s.gbuffer0[b]),
                       static_cast<const uint4*>(s.gbuffer3[b]), sc.materials, static_cast<uint32_t>(ctx.materials.size()), n,
                       static_cast<uint32_t*>(emissive));
    GFX_HIP(hipGetLastError());
}

void restir_copy_depth_to_linear(Context& ctx, hipStream_t stream, void* depth) {
    if (!ctx.restir.valid) throw HipError("gfx_restir_copy_depth_to_linear: gfx_restir_set_params first");
    if (!depth) throw HipError("gfx_restir_copy_depth_to_linear: null output");
    const gfx_restir_static_params& s = ctx.restir.s;
    const int n = s.imageSizeX * s.imageSizeY;
    if (n <= 0) return;
    const uint32_t b = ctx.restir.f.bufferIndex;
    const float* cam = ctx.restir.f.camera.position;
    hipLaunchKernelGGL(k_copy_depth, dim3((n + kDnBlock - 1) / kDnBlock), dim3(kDnBlock), 0, stream, static_cast<const gfx_gbuffer0*>(s.gbuffer0[b]),
                       static_cast<const gfx_gbuffer2*>(s.gbuffer2[b]), cam[0], cam[1], cam[2], n, static_cast<float*>(depth));
    GFX_HIP(hipGetLastError());
}

} // namespace gfx
