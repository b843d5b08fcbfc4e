// emitter_cull.h -- a 16-byte bound per emitter record that proves most zero-weight light candidates zero
// before their record is fetched.
//
// A candidate of the initial pass (restir.hip initial_candidates) has a target of exactly zero when
//   (a) the emitter faces away from the shading point:   lpCos = dot(-dir, ls.normal) <= 0       (direct_lighting*: returns 0), or
//   (b) it lies below the shading point's horizon:       dirLocal.z * vOutLocal.z <= 0           (Bsdf::evaluate: returns 0, and
//       0 * Le * G is 0 for a finite Le and a finite G).
// About four candidates in five of a street scene are of that kind.  Both conditions follow from a few numbers per record:
//   plane   N, hLo : N a direction close to the record's world normal, hLo = the smallest dot(N, vertex).  Every point x the
//                    sampler can return is a convex combination of the vertices, so dot(N, x) >= hLo and
//                    dot(N, p) <= hLo - margin  =>  dot(N, x - p) >= margin  =>  (a).
//                    Only flat emitters (three bit-equal vertex normals: ls.normal is the same for every point) get a plane.
//   sphere  c, r   : every vertex, hence every x, lies within r of c.  With n the shading normal and s the sign of vOutLocal.z
//                    s * dot(n, c - p) + r < -margin  =>  s * dot(n, x - p) < -margin  =>  (b).
// "Never cull" is an entry like any other: hLo = -inf (no plane), r = +inf (no sphere; the predicate also refuses an infinite S).
//
// Layout (EmitterCull): N octahedral 2 x 16 bit, hLo fp32, c 3 x fp16, r fp16.  The builder folds every quantisation outward:
// hLo is computed with the DECODED N, r is measured from the DECODED c and rounded up, and an N that decodes more than
// kCullNormalTol away from the true normal gets no plane.
//
// The margin.  margin = kCullMargin * (S + 1),  S = |c - p|_1 + |p|_1 + r.  S bounds |x - p| and every coordinate of p and x.
// What it has to cover, with eps = 2^-24 and unit-length n, N_w (the decoded shading normal is unit within 1e-5):
//   * the predicate's own fp32 arithmetic: two three-term dot products and a handful of sums of numbers <= S: < 16 eps S;
//   * the exact path: x = bcA pA + bcB pB + bcC pC with bcA + bcB + bcC = 1 within 2 eps (6 eps S off a convex combination),
//     d = x - p (eps S), dir = d / |d| (4 eps relative), ls.normal = unit(M n) (the builder refuses matrices for which this is
//     not within 2e-5 of N_w), the final dot product (4 eps): < 16 eps S in dot(d, .), < 1e-5 in the cosines;
//   * the quantisation of N: |N / |N| - N_w| <= kCullNormalTol = 2e-4, i.e. at most 2e-4 |x - p| <= 2e-4 S in dot(N_w, x - p).
//     The decoded N is not normalised: it lies on the octahedron |N|_1 = 1, so |N|_2 <= 1 and dot(N / |N|, x - p) >=
//     dot(N, x - p) >= margin.
// Together < 2.1e-4 S against kCullMargin S = 1e-3 S: the true dot(N_w, x - p) (plane) and -s dot(n, x - p) (sphere) exceed
// 7.9e-4 (S + 1), the cosines the exact path computes exceed 7.9e-4 - 1e-5 in magnitude (|x - p| <= S) and have the proven sign;
// |x - p| >= 7.9e-4, so G = lpCos |spCos| / dist2 is finite.  The factor of ~4 between need and margin is head room for
// scenes the analysis did not think of (every build compiles with -ffp-contract=off, so host and device evaluate the same
// operations) and costs about one candidate in a hundred (a float64 model of the bench street culls 0.782 of the candidates at 1e-3
// and 0.769 at 1e-2).  Every comparison is written so that a NaN anywhere leaves the candidate live.
//
// Plain C++ for the device (hipcc) and the host (g++: tests/test_emitter_cull.py drives builder and predicate against the
// oracle's light sampler and an fp32 restatement of shadow_ray / direct_lighting).
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define GFX_CULL_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define GFX_CULL_HD inline
#endif

namespace gfx {

struct alignas(16) EmitterCull {
    uint32_t octN;     // plane direction, octahedral: x in bits 0-15, y in bits 16-31
    float hLo;         // smallest dot(decoded N, vertex); -inf: no plane
    uint32_t cxy;      // sphere centre x | y << 16 (fp16)
    uint32_t czr;      // sphere centre z | radius << 16 (fp16, rounded up; +inf: never cull)
};
static_assert(sizeof(EmitterCull) == 16, "EmitterCull must be 16 bytes");

constexpr float kCullMargin = 1e-3f;
constexpr float kCullNormalTol = 2e-4f;
constexpr uint32_t kCullHalfInf = 0x7C00u;

GFX_CULL_HD uint32_t cull_bits(float f) { return __builtin_bit_cast(uint32_t, f); }
GFX_CULL_HD float cull_float(uint32_t u) { return __builtin_bit_cast(float, u); }
GFX_CULL_HD float cull_abs(float x) { return cull_float(cull_bits(x) & 0x7FFFFFFFu); }
GFX_CULL_HD float cull_neg_inf() { return cull_float(0xFF800000u); }

// fp16 bit pattern -> fp32 (exact).  The builder never emits subnormals.
GFX_CULL_HD float cull_half_to_float(uint32_t h) {
#if defined(__HIP_DEVICE_COMPILE__)
    return static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(h)));
#else
    const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 0x1Fu, m = h & 0x3FFu;
    if (e == 0u) return cull_float(sign);                                  // zero (subnormals are not produced)
    if (e == 31u) return cull_float(sign | 0x7F800000u | (m << 13));       // inf / NaN
    return cull_float(sign | ((e + 112u) << 23) | (m << 13));
#endif
}
// fp32 -> fp16 toward zero; ok = false when x is not finite or too large for a finite fp16.  Below the smallest normal: zero.
GFX_CULL_HD uint32_t cull_float_to_half_trunc(float x, bool& ok) {
    const uint32_t u = cull_bits(x), sign = (u >> 16) & 0x8000u;
    const int32_t e = static_cast<int32_t>((u >> 23) & 0xFFu) - 112;
    if (e >= 31) { ok = false; return sign; }
    if (e <= 0) return sign;
    return sign | (static_cast<uint32_t>(e) << 10) | ((u >> 13) & 0x3FFu);
}
// The smallest fp16 >= x for x >= 0; +inf when there is none or x is not a number.
GFX_CULL_HD uint32_t cull_float_to_half_up(float x) {
    if (!(x <= 65504.0f)) return kCullHalfInf;
    if (!(x >= 6.103515625e-05f)) return 0x0400u;                          // the smallest normal
    bool ok = true;
    uint32_t h = cull_float_to_half_trunc(x, ok);
    if (cull_half_to_float(h) < x) h += 1u;                                // the next fp16 up, across an exponent step too
    return h;
}

// Octahedral direction, not normalised: |N|_1 = 1, hence |N|_2 <= 1.
GFX_CULL_HD void cull_oct_decode(uint32_t q, float& x, float& y, float& z) {
    const float f = static_cast<float>(q & 0xFFFFu) * (2.0f / 65535.0f) - 1.0f;
    const float g = static_cast<float>(q >> 16) * (2.0f / 65535.0f) - 1.0f;
    z = 1.0f - cull_abs(f) - cull_abs(g);
    const float t = z < 0.0f ? -z : 0.0f;
    x = f + (f >= 0.0f ? -t : t);
    y = g + (g >= 0.0f ? -t : t);
}
GFX_CULL_HD uint32_t cull_oct_encode(float x, float y, float z) {
    const float l1 = cull_abs(x) + cull_abs(y) + cull_abs(z);
    float f = x / l1, g = y / l1;
    if (z < 0.0f) {
        const float ff = (1.0f - cull_abs(g)) * (f >= 0.0f ? 1.0f : -1.0f);
        const float gg = (1.0f - cull_abs(f)) * (g >= 0.0f ? 1.0f : -1.0f);
        f = ff; g = gg;
    }
    auto q16 = [](float v) {
        const float s = (v * 0.5f + 0.5f) * 65535.0f + 0.5f;
        return !(s > 0.0f) ? 0u : s >= 65535.0f ? 65535u : static_cast<uint32_t>(s);
    };
    return q16(f) | (q16(g) << 16);
}

GFX_CULL_HD EmitterCull cull_never() {
    EmitterCull e;
    e.octN = 0x80008000u; e.hLo = cull_neg_inf(); e.cxy = 0u; e.czr = kCullHalfInf << 16;
    return e;
}

// The entry of one record.  m: the instance's normal matrix, rows m[0..2], m[3..5], m[6..8]; nA: the first vertex normal in
// object space; flat: the three vertex normals are bit-equal (EmitterRec::flags without kEmitterSmooth); pA, pB, pC: the world
// positions stored in the record; finiteEmittance: the record's emittance is three finite numbers.
GFX_CULL_HD EmitterCull cull_build(const float* m, const float* nA, bool flat, const float* pA, const float* pB, const float* pC, bool finiteEmittance) {
    EmitterCull e = cull_never();
    if (!finiteEmittance) return e;                        // 0 * Le must be 0
    const float inf = cull_float(0x7F800000u);
    // degenerate or non-finite triangle: its density 2 / |ng| is not a finite non-zero number either
    const float ax = pB[0] - pA[0], ay = pB[1] - pA[1], az = pB[2] - pA[2];
    const float bx = pC[0] - pA[0], by = pC[1] - pA[1], bz = pC[2] - pA[2];
    const float gx = ay * bz - az * by, gy = az * bx - ax * bz, gz = ax * by - ay * bx;
    const float g2 = gx * gx + gy * gy + gz * gz;
    if (!(g2 > 0.0f && g2 < inf)) return e;
    // sphere: fp16 centre near the centroid, radius measured from the decoded centre
    bool ok = true;
    const uint32_t hx = cull_float_to_half_trunc((pA[0] + pB[0] + pC[0]) * (1.0f / 3.0f), ok);
    const uint32_t hy = cull_float_to_half_trunc((pA[1] + pB[1] + pC[1]) * (1.0f / 3.0f), ok);
    const uint32_t hz = cull_float_to_half_trunc((pA[2] + pB[2] + pC[2]) * (1.0f / 3.0f), ok);
    if (!ok) return e;
    const float cx = cull_half_to_float(hx), cy = cull_half_to_float(hy), cz = cull_half_to_float(hz);
    float r2 = 0.0f;
    const float* v[3] = { pA, pB, pC };
    for (int k = 0; k < 3; ++k) {
        const float dx = v[k][0] - cx, dy = v[k][1] - cy, dz = v[k][2] - cz;
        const float d2 = dx * dx + dy * dy + dz * dz;
        if (!(d2 <= r2)) r2 = d2;                          // a NaN sticks
    }
    const uint32_t hr = cull_float_to_half_up(__builtin_sqrtf(r2) * 1.00001f);
    if (hr >= kCullHalfInf) return e;
    e.cxy = hx | (hy << 16);
    e.czr = hz | (hr << 16);
    if (!flat) return e;                                   // smooth emitter: sphere only
    // plane: N_w = unit(M nA) as light_from_record forms it
    const float wx = m[0] * nA[0] + m[1] * nA[1] + m[2] * nA[2];
    const float wy = m[3] * nA[0] + m[4] * nA[1] + m[5] * nA[2];
    const float wz = m[6] * nA[0] + m[7] * nA[1] + m[8] * nA[2];
    const float len = __builtin_sqrtf(wx * wx + wy * wy + wz * wz);
    // cancellation inside M nA: each component is off by at most 3 eps sum_j |M_ij nA_j|; within 64 |M nA| that moves the
    // direction by less than 2e-5
    float mag = 0.0f;
    for (int k = 0; k < 9; ++k) mag += cull_abs(m[k] * nA[k % 3]);
    if (!(len > 0.0f && len < inf && mag <= 64.0f * len)) return e;
    const float ux = wx / len, uy = wy / len, uz = wz / len;
    const uint32_t q = cull_oct_encode(ux, uy, uz);
    float nx, ny, nz;
    cull_oct_decode(q, nx, ny, nz);
    const float nl = __builtin_sqrtf(nx * nx + ny * ny + nz * nz);
    const float ex = nx / nl - ux, ey = ny / nl - uy, ez = nz / nl - uz;
    if (!(ex * ex + ey * ey + ez * ez <= (0.5f * kCullNormalTol) * (0.5f * kCullNormalTol))) return e;   // half the tolerance: this check is fp32 too
    float hLo = inf;
    for (int k = 0; k < 3; ++k) {
        const float h = nx * v[k][0] + ny * v[k][1] + nz * v[k][2];
        if (!(h >= hLo)) hLo = h;
    }
    if (!(hLo > -inf && hLo < inf)) return e;
    e.octN = q;
    e.hLo = hLo;
    return e;
}

// True: a sample on the record has a target of exactly zero at shading point p (the offset ray origin the exact path uses)
// with shading normal n (Frame::n) and vz = vOutLocal.z.
GFX_CULL_HD bool cull_proves_zero(const EmitterCull& e, float px, float py, float pz, float nx, float ny, float nz, float vz) {
    const float cx = cull_half_to_float(e.cxy & 0xFFFFu), cy = cull_half_to_float(e.cxy >> 16);
    const float cz = cull_half_to_float(e.czr & 0xFFFFu), r = cull_half_to_float(e.czr >> 16);
    const float dx = cx - px, dy = cy - py, dz = cz - pz;
    const float S = ((cull_abs(dx) + cull_abs(dy)) + cull_abs(dz)) + ((cull_abs(px) + cull_abs(py)) + cull_abs(pz)) + r;
    const float margin = kCullMargin * S + kCullMargin;
    float Nx, Ny, Nz;
    cull_oct_decode(e.octN, Nx, Ny, Nz);
    const bool plane = Nx * px + Ny * py + Nz * pz <= e.hLo - margin;
    const float h = nx * dx + ny * dy + nz * dz;
    const bool horizon = vz > 0.0f ? h + r < -margin : vz < 0.0f ? r - h < -margin : false;
    return S < 3.0e38f && (plane || horizon);              // an infinite S (never-cull entry, non-finite point) proves nothing
}

} // namespace gfx
