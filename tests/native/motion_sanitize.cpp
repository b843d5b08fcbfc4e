// motion_sanitize.cpp -- a stand-alone program (its own main, nothing loaded into Python, nothing near the GPU library) that runs the
// host side of the motion of displaced instances under sanitizers: make_cur_to_prev (gfxexp_amd/csrc/tfdm/tfdm_instance.hip.h) and
// displaced_gbuffer with a motion table (gfxexp_amd/csrc/tfdm/displaced_surface.hip.h).  Build and run from the repository root:
//   g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -ffp-contract=off -fno-fast-math -Wall -fsanitize=address,undefined
//       -fno-sanitize-recover=all -Igfxexp_amd/csrc -Iinclude tests/native/motion_sanitize.cpp -o motion_sanitize && ./motion_sanitize
// It prints "ok" and exits 0, or says what differs and exits 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "tfdm/displaced_surface.hip.h"

using namespace gfx::tfdm;

static uint32_t g_state = 12345u;
static float rnd(float lo, float hi) {
    g_state = g_state * 1664525u + 1013904223u;
    return lo + (hi - lo) * static_cast<float>(g_state >> 8) * (1.0f / 16777216.0f);
}

int main() {
    static const float ident[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
    int bad = 0;
    // heap copies of exactly 12 floats: a read or a write past either end is an AddressSanitizer report
    for (int it = 0; it < 2000; ++it) {
        std::vector<float> prev(12), cur(12), out(12, -1.0f);
        for (int i = 0; i < 12; ++i) { cur[i] = rnd(-2.0f, 2.0f); prev[i] = cur[i] + rnd(-0.25f, 0.25f); }
        for (int d = 0; d < 3; ++d) { cur[5 * d] += 3.0f; prev[5 * d] += 3.0f; }       // diagonally dominant: invertible
        if (it % 7 == 0) prev = cur;
        if (it % 11 == 0) prev[it % 12] = (it % 2) ? NAN : INFINITY;
        if (it % 13 == 0) for (int i = 0; i < 4; ++i) cur[4 + i] = cur[i];             // two equal rows: singular
        if (it % 17 == 0) for (int i = 0; i < 12; ++i) { cur[i] *= 1e-30f; prev[i] *= 1e30f; }   // the product overflows a float
        const char* err = make_cur_to_prev(prev.data(), cur.data(), out.data());
        const bool same = std::memcmp(prev.data(), cur.data(), 48) == 0;
        if (same && (err || std::memcmp(out.data(), ident, 48) != 0)) { std::printf("case %d: equal transforms do not give the identity\n", it); ++bad; }
        if (!same && it % 11 == 0 && !err) { std::printf("case %d: a previous transform that is not finite was accepted\n", it); ++bad; }
        if (!err) for (int i = 0; i < 12; ++i) if (!std::isfinite(out[i])) { std::printf("case %d: accepted with entry %d not finite\n", it, i); ++bad; break; }
        if (err) continue;
        // the G-buffer words with this matrix as instance 2 of a three-instance table
        std::vector<float> motion(36);
        for (int k = 0; k < 3; ++k) std::memcpy(motion.data() + 12 * k, k == 2 ? out.data() : ident, 48);
        std::vector<InstanceRecord> table(3);
        std::memset(table.data(), 0, sizeof(InstanceRecord) * 3);
        for (int k = 0; k < 3; ++k) for (int i = 0; i < 12; ++i) table[k].objToWorld[i] = table[k].worldToObj[i] = ident[i];
        SceneHit h;
        h.dist = rnd(1.0f, 9.0f); h.bcB = rnd(0.0f, 0.5f); h.bcC = rnd(0.0f, 0.5f); h.index = 5u; h.normal = v3(0.0f, 0.0f, 1.0f); h.where = (2u << 1) | 1u;
        BaseVertex v[3];
        for (int k = 0; k < 3; ++k) { v[k].texCoord0Dir = v3(1.0f, 0.0f, 0.0f); v[k].u = rnd(0.0f, 1.0f); v[k].v = rnd(0.0f, 1.0f); }
        gfx_camera cam;
        std::memset(&cam, 0, sizeof(cam));
        cam.orientation[0] = cam.orientation[4] = cam.orientation[8] = 1.0f;
        cam.position[2] = -4.0f; cam.fovY = 0.7f; cam.aspect = 1.5f;
        const DisplacedPoint p = displaced_point(table[2], h, v3(rnd(-1.0f, 1.0f), rnd(-1.0f, 1.0f), -4.0f), v3(0.0f, 0.0f, 1.0f), v[0], v[1], v[2]);
        const DisplacedGBuffer a = displaced_gbuffer(p, h, 7u, 3u, cam, 10, 20, 96.0f, 64.0f, false, motion.data() + 12 * (h.where >> 1));
        const DisplacedGBuffer b = displaced_gbuffer(p, h, 7u, 3u, cam, 10, 20, 96.0f, 64.0f, false);
        const DisplacedGBuffer c = displaced_gbuffer(p, h, 7u, 3u, cam, 10, 20, 96.0f, 64.0f, false, ident);
        if (std::memcmp(&b, &c, sizeof(b)) != 0) { std::printf("case %d: the identity changes the words\n", it); ++bad; }
        if (std::memcmp(a.g0, b.g0, 16) != 0 || std::memcmp(a.position, b.position, 12) != 0 || std::memcmp(a.g3, b.g3, 16) != 0) {
            std::printf("case %d: the motion changes more than the motion vector\n", it); ++bad;
        }
    }
    if (bad) std::printf("%d failures\n", bad);
    else std::printf("ok\n");
    return bad ? 1 : 0;
}
