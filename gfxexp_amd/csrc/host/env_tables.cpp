// env_tables.cpp -- tables the host builds for the device samplers: the environment map's importance distributions, guides, row
// records and sketches, the procedural sky, and the Halton disk of the spatial reuse pass.
#include <cstring>
#include "host_scene.h"

using namespace gfx_host;

extern "C" {

// restir_di_main.cpp:1487-1542 -- Halton(2,3) through the concentric square->disk map.  The host
// program uses <cmath> cos/sin; here the table goes through the same deterministic sincos as the
// kernels so any consumer (including a CPU checker) reproduces it bit for bit.
static void host_sincos(float x, float* s, float* c) {
    // identical algorithm to gfx::gm_sincos (gm_math.hip.h), host build
    const float q = std::rint(x * 0.6366197466850281f);
    float r = std::fma(q, -1.5703125f, x);
    r = std::fma(q, -0.0004837512969970703f, r);
    r = std::fma(q, -7.549790126404332e-08f, r);
    const int n = static_cast<int>(q);
    const float r2 = r * r;
    float ps = std::fma(-1.9515295891e-4f, r2, 8.3321608736e-3f);
    ps = std::fma(ps, r2, -1.6666654611e-1f);
    const float sr = std::fma(ps * r2, r, r);
    float pc = std::fma(2.443315711809948e-5f, r2, -1.388731625493765e-3f);
    pc = std::fma(pc, r2, 4.166664568298827e-2f);
    const float cr = std::fma(pc * r2, r2, std::fma(-0.5f, r2, 1.0f));
    const float ss = (n & 1) ? cr : sr, cc = (n & 1) ? sr : cr;
    *s = (n & 2) ? -ss : ss;
    *c = ((n + 1) & 2) ? -cc : cc;
}
// RegularConstantContinuousDistribution1D::initialize, common/common_host.cpp:292-316 (Kahan sums)
static float build_rccd1d(const float* values, uint32_t n, float* pdf, float* cdf) {
    float result = 0.0f, comp = 0.0f;   // CompensatedSum_T, common/basic_types.h:5428-5452
    for (uint32_t i = 0; i < n; ++i) {
        cdf[i] = result;
        const float input = values[i] / n - comp;
        const float t = result + input;
        comp = (t - result) - input;
        result = t;
    }
    const float integral = result;
    for (uint32_t i = 0; i < n; ++i) { pdf[i] = values[i] / integral; cdf[i] /= integral; }
    cdf[n] = 1.0f;
    return integral;
}

int gfxh_env_build_importance(float* texels, uint32_t w, uint32_t h, float* rowPDF, float* rowCDF,
                              float* rowIntegrals, float* topPDF, float* topCDF, float* topIntegral) {
    std::vector<float> importance(static_cast<size_t>(w) * h);
    for (uint32_t y = 0; y < h; ++y) {
        const float theta = 3.14159265358979323846f * (y + 0.5f) / h;
        float sinTheta, cosTheta;
        host_sincos(theta, &sinTheta, &cosTheta);
        for (uint32_t x = 0; x < w; ++x) {
            float* t = texels + 4 * (static_cast<size_t>(y) * w + x);
            for (int c = 0; c < 3; ++c) t[c] = std::min(std::max(t[c], 0.0f), 65504.0f);
            importance[static_cast<size_t>(y) * w + x] = (0.2126729f * t[0] + 0.7151522f * t[1] + 0.0721750f * t[2]) * sinTheta;
        }
    }
    for (uint32_t y = 0; y < h; ++y)
        rowIntegrals[y] = build_rccd1d(importance.data() + static_cast<size_t>(y) * w, w, rowPDF + static_cast<size_t>(y) * w,
                                       rowCDF + static_cast<size_t>(y) * (w + 1));
    *topIntegral = build_rccd1d(rowIntegrals, h, topPDF, topCDF);
    return 0;
}

// guide[k] = largest index i in [0, n) with cell(cdf[i]) <= k, cell(x) = min(n - 1, uint(x * n)): the device
// samplers (shading.hip.h, EnvMap::sample1d) bracket the search for u with guide[cell(u) - 1] .. guide[cell(u)].
static bool build_guide(const float* cdf, uint32_t n, uint16_t* guide) {
    if (n == 0 || n > 65536u) return false;
    if (!(cdf[0] == 0.0f)) return false;
    for (uint32_t i = 0; i + 1 < n; ++i) if (!(cdf[i] <= cdf[i + 1])) return false;
    auto cell = [n](float x) { return std::min<uint32_t>(n - 1u, static_cast<uint32_t>(x * static_cast<float>(n))); };
    uint32_t idx = 0;
    for (uint32_t k = 0; k < n; ++k) {
        while (idx + 1 < n && cell(cdf[idx + 1]) <= k) ++idx;
        guide[k] = static_cast<uint16_t>(idx);
    }
    return true;
}

int gfxh_env_build_guides(const float* rowCDF, const float* topCDF, uint32_t w, uint32_t h, uint16_t* rowGuide, uint16_t* topGuide) {
    if (!build_guide(topCDF, h, topGuide)) return 0;
    for (uint32_t y = 0; y < h; ++y)
        if (!build_guide(rowCDF + static_cast<size_t>(y) * (w + 1), w, rowGuide + static_cast<size_t>(y) * w)) return 0;
    return 1;
}

void gfxh_env_build_row_table(const float* texels, const float* rowPDF, const float* rowCDF, const uint16_t* rowGuide, uint32_t w, uint32_t h, void* outRecords) {
    // record (row, i) of 32 bytes: {cdf, pdf, guide, r | g, b, cdf of record i + 1, 0} (shading.hip.h EnvRowRec); i = w: the row's final CDF
    // value alone; rows GFX_ENV_ROW_STRIDE(w) records apart, so that four consecutive records from a multiple of four are one 128-byte line
    uint32_t* out = static_cast<uint32_t*>(outRecords);
    auto bits = [](float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; };
    const size_t stride = GFX_ENV_ROW_STRIDE(w);
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t i = 0; i < stride; ++i) {
            uint32_t* rec = out + 8 * (static_cast<size_t>(y) * stride + i);
            for (int k = 0; k < 8; ++k) rec[k] = 0u;
            if (i > w) continue;
            rec[0] = bits(rowCDF[static_cast<size_t>(y) * (w + 1) + i]);
            if (i < w) {
                const float* t = texels + 4 * (static_cast<size_t>(y) * w + i);
                rec[1] = bits(rowPDF[static_cast<size_t>(y) * w + i]);
                rec[2] = rowGuide[static_cast<size_t>(y) * w + i];
                rec[3] = bits(t[0]); rec[4] = bits(t[1]); rec[5] = bits(t[2]);
                rec[6] = bits(rowCDF[static_cast<size_t>(y) * (w + 1) + i + 1]);
            }
        }
}

// The column RegularConstantContinuousDistribution1D::sample's bisection ends on: the largest index of [0, n - 1] whose CDF value is <= u.
static uint32_t env_column_of(const float* cdf, uint32_t n, float u) {
    uint32_t lo = 0, hi = n - 1;
    while (lo < hi) { const uint32_t mid = (lo + hi + 1) >> 1; if (cdf[mid] <= u) lo = mid; else hi = mid - 1; }
    return lo;
}
// The device's interpolation between two knots (shading.hip.h EnvMap::sample1d_row_sketch: the same operations in the same order; the
// position t inside the cell is exact, the rest is one subtraction, one product, one sum).
static int env_sketch_interpolate(const float* knots, uint32_t k, float t) {
    const float d = knots[k + 1] - knots[k];
    const float p = knots[k] + t * d;
    return static_cast<int>(p);
}
// One sketch record over [uLo, uLo + 32 step): 33 knots of the row's inverse CDF and the mask of the cells whose interpolation is within
// one column of the bisection's answer for EVERY u of the cell.  `local(u, k, t)`: the cell and the position inside it the device derives
// for u at this level.  The interpolation is monotone in u inside a cell (a product and a sum of non-negative terms, correctly rounded)
// and the column is constant between the lowest and the highest u that end on it: testing both ends of every column covers the cell.
extern "C++" {
template <typename Local>
static uint32_t env_sketch_record(const float* cdf, uint32_t w, float uLo, float step, Local local, float knots[GFX_ENV_SKETCH_CELLS + 1]) {
    const uint32_t K = GFX_ENV_SKETCH_CELLS;
    for (uint32_t j = 0; j <= K; ++j) {
        const float u = uLo + static_cast<float>(j) * step;          // exact: powers of two
        float pos = static_cast<float>(w);
        if (u < 1.0f) {
            const uint32_t c = env_column_of(cdf, w, u);
            const float width = cdf[c + 1] - cdf[c];
            const float t = width > 0.0f ? (u - cdf[c]) / width : 0.0f;
            pos = static_cast<float>(c) + std::min(std::max(t, 0.0f), 1.0f);
        }
        knots[j] = pos;
    }
    for (uint32_t j = 0; j < K; ++j) if (!(knots[j] <= knots[j + 1])) return 0u;   // the prediction must not decrease inside a cell
    uint32_t mask = 0;
    for (uint32_t k = 0; k < K; ++k) {
        const float cLo = uLo + static_cast<float>(k) * step, cHi = std::nextafter(uLo + static_cast<float>(k + 1) * step, 0.0f);
        const uint32_t cFirst = env_column_of(cdf, w, cLo), cLast = env_column_of(cdf, w, cHi);
        bool ok = true;
        for (uint32_t c = cFirst; c <= cLast && ok; ++c) {
            const float a = std::max(cLo, cdf[c]);
            const float b = cdf[c + 1] <= cHi ? std::nextafter(cdf[c + 1], 0.0f) : cHi;
            if (!(a <= b)) continue;                                  // an empty column: never the bisection's answer
            for (float u : { a, b }) {
                if (env_column_of(cdf, w, u) != c) continue;          // (ties: this u belongs to a later column of equal CDF value, tested there)
                uint32_t kk; float t;
                local(u, kk, t);
                if (kk != k) { ok = false; break; }                   // (cannot happen: the cell bounds are exact)
                const int pred = env_sketch_interpolate(knots, kk, t);
                if (pred < static_cast<int>(c) - 1 || pred > static_cast<int>(c) + 1) ok = false;
            }
        }
        if (ok) mask |= 1u << k;
    }
    return mask;
}
}   // extern "C++"

uint32_t gfxh_env_build_row_sketch(const float* rowCDF, uint32_t w, uint32_t h, void* outSketch, uint32_t capacityRecords, uint32_t* numRecords) {
    const uint32_t K = GFX_ENV_SKETCH_CELLS, W = GFX_ENV_SKETCH_WORDS;
    std::vector<uint32_t> rows(static_cast<size_t>(h) * W, 0u), children;
    uint32_t good = 0, numChildren = 0;
    auto cell_of = [](float x, uint32_t& k, float& t) {
        const uint32_t K = GFX_ENV_SKETCH_CELLS;             // the device's split of a position in [0, 1) into cell and remainder
        const float xk = x * static_cast<float>(K);
        k = static_cast<uint32_t>(xk);
        if (k > K - 1u) k = K - 1u;
        t = xk - static_cast<float>(k);
    };
    for (uint32_t y = 0; y < h; ++y) {
        const float* cdf = rowCDF + static_cast<size_t>(y) * (w + 1);
        bool monotone = cdf[0] == 0.0f;
        for (uint32_t i = 0; i < w && monotone; ++i) monotone = cdf[i] <= cdf[i + 1];
        float knots[GFX_ENV_SKETCH_CELLS + 1];
        uint32_t mask = 0;
        if (monotone) mask = env_sketch_record(cdf, w, 0.0f, 1.0f / K, [&](float u, uint32_t& k, float& t) { cell_of(u, k, t); }, knots);
        else for (uint32_t j = 0; j <= K; ++j) knots[j] = 0.0f;
        uint32_t* row = rows.data() + static_cast<size_t>(y) * W;
        std::memcpy(row, knots, 4 * (K + 1));
        for (uint32_t k = 0; k < K; ++k) if (!((mask >> k) & 1u)) row[k] |= 0x80000000u;   // the sign bit of knot k repeats mask bit k (cleared = verified): one sector per sample
        row[K + 1] = mask; row[K + 2] = numChildren;
        for (uint32_t k = 0; k < K; ++k) {
            if ((mask >> k) & 1u) { ++good; continue; }
            // a child record for the failing cell: the same at 1/32 of the step (a row whose CDF is not monotone gets empty children: the guide)
            float sub[GFX_ENV_SKETCH_CELLS + 1];
            uint32_t subMask = 0;
            if (monotone) {
                const uint32_t k1 = k;
                subMask = env_sketch_record(cdf, w, static_cast<float>(k1) / K, 1.0f / (K * K), [&](float u, uint32_t& kk, float& t) {
                    uint32_t ka; float ta;
                    cell_of(u, ka, ta);                              // level 1: ka == k1 for every u of this cell
                    cell_of(ta, kk, t);                              // level 2: the remainder is the position inside the cell
                    if (ka != k1) kk = K;                            // (reported as a mismatch)
                }, sub);
            }
            else for (uint32_t j = 0; j <= K; ++j) sub[j] = 0.0f;
            children.resize(children.size() + W, 0u);
            uint32_t* rec = children.data() + static_cast<size_t>(numChildren) * W;
            std::memcpy(rec, sub, 4 * (K + 1));
            for (uint32_t j = 0; j < K; ++j) if (!((subMask >> j) & 1u)) rec[j] |= 0x80000000u;
            rec[K + 1] = subMask;
            ++numChildren;
        }
    }
    if (numRecords) *numRecords = h + numChildren;
    if (outSketch && capacityRecords >= h + numChildren) {
        std::memcpy(outSketch, rows.data(), 4 * rows.size());
        if (!children.empty()) std::memcpy(static_cast<uint32_t*>(outSketch) + rows.size(), children.data(), 4 * children.size());
    }
    return good;
}

void gfxh_env_make_sky(uint32_t w, uint32_t h, float sunElevationDeg, float sunAzimuthDeg, float sunRadiance, float* texels) {
    const float d2r = 3.14159265358979323846f / 180.0f;
    const float se = sunElevationDeg * d2r, sa = sunAzimuthDeg * d2r;
    const V3 sun = { -std::sin(sa) * std::cos(se), std::sin(se), std::cos(sa) * std::cos(se) };
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            const float theta = 3.14159265358979323846f * (y + 0.5f) / h, phi = 2 * 3.14159265358979323846f * (x + 0.5f) / w;
            const V3 d = { -std::sin(phi) * std::sin(theta), std::cos(theta), std::cos(phi) * std::sin(theta) };   // fromPolarYUp
            const float up = std::max(d.y, 0.0f);
            float r = 0.25f + 0.5f * (1 - up), g = 0.35f + 0.45f * (1 - up), b = 0.7f + 0.2f * (1 - up);
            if (d.y < 0) { r = g = b = 0.05f; }
            const float c = dot(d, sun);
            if (c > 0.9995f) { r += sunRadiance; g += sunRadiance * 0.95f; b += sunRadiance * 0.85f; }
            else if (c > 0.99f) { const float k = (c - 0.99f) / 0.0095f; r += 4 * k; g += 3.6f * k; b += 3 * k; }
            float* t = texels + 4 * (static_cast<size_t>(y) * w + x);
            t[0] = r; t[1] = g; t[2] = b; t[3] = 1.0f;
        }
}

void gfxh_spatial_neighbor_deltas(float* out) {
    auto halton = [](uint32_t base, uint32_t idx) {
        const float recBase = 1.0f / base;
        float ret = 0.0f, scale = 1.0f;
        while (idx) { scale *= recBase; ret += (idx % base) * scale; idx /= base; }
        return ret;
    };
    for (uint32_t i = 0; i < 1024; ++i) {
        const float u0 = halton(2, i), u1 = halton(3, i);
        float dx = 0, dy = 0;
        const float sx = 2 * u0 - 1, sy = 2 * u1 - 1;
        if (!(sx == 0 && sy == 0)) {
            float r, theta;
            if (sx >= -sy) {
                if (sx > sy) { r = sx; theta = sy / sx; }
                else { r = sy; theta = 2 - sx / sy; }
            }
            else {
                if (sx > sy) { r = -sy; theta = 6 + sx / sy; }
                else { r = -sx; theta = 4 + sy / sx; }
            }
            theta *= 3.14159265358979323846f / 4;
            float s, c;
            host_sincos(theta, &s, &c);
            dx = r * c; dy = r * s;
        }
        out[2 * i] = dx; out[2 * i + 1] = dy;
    }
}

} // extern "C"
