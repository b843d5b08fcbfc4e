// taa_ref.cpp -- TEST INFRASTRUCTURE: CPU restatement of the temporal anti-aliasing pass (gfx_taa_apply), written from the
// specification in the header comment of gfxexp_amd/csrc/denoise/taa.hip (steps 1-5), not from the kernel.  Stateless: the caller
// passes the history the call reprojects and receives the one it writes, so a test can compare both with the GPU's (gfx_taa_history).
// Build: g++ -O2 -march=x86-64-v3 -ffp-contract=off -fno-fast-math -shared -fPIC (tests/taa_ref.py compiles it).
#include <cmath>
#include <cstdint>

namespace {

float mn(float a, float b) { return a < b ? a : b; }
float mx(float a, float b) { return a > b ? a : b; }
int cl(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

struct Img4 {
    const float* d;
    int W;
    const float* at(int x, int y) const { return d + 4 * (static_cast<int64_t>(y) * W + x); }
};

} // namespace

extern "C" int taa_ref_run(int W, int H, uint32_t N, const float* color, const float* flow, int isFirstFrame, const float* prevHistory,
                           float* out, float* history) {
    if (W <= 0 || H <= 0 || N < 1 || N > 256) return 1;
    const Img4 C{color, W}, Hp{prevHistory, W};
    const float a = 1.0f / static_cast<float>(N);
    const float b = 1.0f - a;
    for (int y = 0; y < H; ++y) {
        for (int x = 0; x < W; ++x) {
            const int64_t p = static_cast<int64_t>(y) * W + x;
            // 1. current colour, alpha copied
            const float* cp = C.at(x, y);
            float c[3] = {cp[0], cp[1], cp[2]};
            float o[4] = {c[0], c[1], c[2], cp[3]};
            // 3. reprojection (needed first to know whether step 4 blends)
            bool blend = isFirstFrame == 0;
            float Px = 0.0f, Py = 0.0f;
            if (blend) {
                Px = (static_cast<float>(x) + 0.5f) - flow[2 * p];
                Py = (static_cast<float>(y) + 0.5f) - flow[2 * p + 1];
                const bool onScreen = Px >= 0.0f && Px < static_cast<float>(W) && Py >= 0.0f && Py < static_cast<float>(H);
                blend = onScreen;
            }
            if (blend) {
                const int qx = static_cast<int>(Px), qy = static_cast<int>(Py);
                const float fx = Px - (static_cast<float>(qx) + 0.5f);
                const float fy = Py - (static_cast<float>(qy) + 0.5f);
                const int dx = fx < 0.0f ? -1 : 1, dy = fy < 0.0f ? -1 : 1;
                const float s = std::fabs(fx), t = std::fabs(fy);
                const float* h0 = Hp.at(qx, qy);
                const float* h1 = Hp.at(cl(qx + dx, W), qy);
                const float* h2 = Hp.at(qx, cl(qy + dy, H));
                const float* h3 = Hp.at(cl(qx + dx, W), cl(qy + dy, H));
                const float w0 = (1.0f - s) * (1.0f - t);
                const float w1 = s * (1.0f - t);
                const float w2 = (1.0f - s) * t;
                const float w3 = s * t;
                float sw = w0;
                sw = sw + w1;
                sw = sw + w2;
                sw = sw + w3;
                float prev[3];
                for (int k = 0; k < 3; ++k) {
                    float S = w0 * h0[k];
                    S = S + w1 * h1[k];
                    S = S + w2 * h2[k];
                    S = S + w3 * h3[k];
                    prev[k] = sw != 0.0f ? S / sw : 0.0f;
                }
                // 2. neighbourhood: box (8 neighbours + centre) and cross (4 edge neighbours + centre)
                float bMin[3], bMax[3], xMin[3], xMax[3];
                for (int k = 0; k < 3; ++k) bMin[k] = bMax[k] = xMin[k] = xMax[k] = c[k];
                for (int i = -1; i <= 1; ++i) {
                    for (int j = -1; j <= 1; ++j) {
                        if (i == 0 && j == 0) continue;
                        const float* v = C.at(cl(x + j, W), cl(y + i, H));
                        for (int k = 0; k < 3; ++k) {
                            bMin[k] = mn(bMin[k], v[k]);
                            bMax[k] = mx(bMax[k], v[k]);
                            if (i == 0 || j == 0) {
                                xMin[k] = mn(xMin[k], v[k]);
                                xMax[k] = mx(xMax[k], v[k]);
                            }
                        }
                    }
                }
                // 4. blend with the clamped history
                for (int k = 0; k < 3; ++k) {
                    const float nbMin = 0.5f * (bMin[k] + xMin[k]);
                    const float nbMax = 0.5f * (bMax[k] + xMax[k]);
                    const float h = mn(mx(prev[k], nbMin), nbMax);
                    const float bh = b * h;
                    const float ac = a * c[k];
                    o[k] = bh + ac;
                }
            }
            // 5. output and history
            for (int k = 0; k < 4; ++k) {
                out[4 * p + k] = o[k];
                history[4 * p + k] = o[k];
            }
        }
    }
    return 0;
}
