// shell_shapes.cpp -- shell meshes for gfx_shell_create on the host layer: the placing transform of a loaded mesh into the unit
// tile (nrtdsm_main.cpp:835-845) and the reference's "One Box" (:778-798).
#include <cmath>
#include <vector>
#include "host_scene.h"

extern "C" {

int gfxh_shell_fit(const float* positions, uint32_t n, int yUp, float* out) {
    std::string& err = gfx_host::host_error();
    if (!positions || !out || n == 0) { err = "gfxh_shell_fit: no points"; return 1; }
    double lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    std::vector<double> p(3 * static_cast<size_t>(n));
    for (uint32_t i = 0; i < n; ++i) {
        const double x = positions[3 * i], y = positions[3 * i + 1], z = positions[3 * i + 2];
        if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z)) { err = "gfxh_shell_fit: a point is not finite"; return 1; }
        // rotate3DX(+90 degrees): (x, y, z) -> (x, -z, y)
        p[3 * i] = x; p[3 * i + 1] = yUp ? -z : y; p[3 * i + 2] = yUp ? y : z;
        for (int k = 0; k < 3; ++k) { lo[k] = std::fmin(lo[k], p[3 * i + k]); hi[k] = std::fmax(hi[k], p[3 * i + k]); }
    }
    const double extent = std::fmax(hi[0] - lo[0], hi[1] - lo[1]);
    if (!(extent > 0.0)) { err = "gfxh_shell_fit: the points have no extent in x and y"; return 1; }
    const double s = 1.0 / extent, cx = 0.5 * (lo[0] + hi[0]), cy = 0.5 * (lo[1] + hi[1]);
    for (uint32_t i = 0; i < n; ++i) {
        // a float just outside the tile after rounding would be refused by gfx_shell_create: clamp u and v
        const double u = 0.5 + s * (p[3 * i] - cx), v = 0.5 + s * (p[3 * i + 1] - cy);
        out[3 * i] = static_cast<float>(std::fmin(std::fmax(u, 0.0), 1.0));
        out[3 * i + 1] = static_cast<float>(std::fmin(std::fmax(v, 0.0), 1.0));
        out[3 * i + 2] = static_cast<float>(s * (p[3 * i + 2] - lo[2]));
    }
    return 0;
}

int gfxh_shell_box(float* positions, uint32_t* triangles) {
    if (!positions || !triangles) { gfx_host::host_error() = "gfxh_shell_box: null argument"; return 1; }
    for (uint32_t i = 0; i < 8u; ++i) {        // bit 0: u, bit 1: v, bit 2: h
        positions[3 * i] = (i & 1u) ? 0.8f : 0.2f;
        positions[3 * i + 1] = (i & 2u) ? 0.8f : 0.2f;
        positions[3 * i + 2] = (i & 4u) ? 0.08f : 0.0f;
    }
    // two triangles per face, wound so that they face outward in right-handed (u, v, h)
    static const uint32_t kFaces[36] = { 0, 2, 3, 0, 3, 1,  4, 5, 7, 4, 7, 6,  0, 4, 6, 0, 6, 2,  1, 3, 7, 1, 7, 5,  0, 1, 5, 0, 5, 4,  2, 6, 7, 2, 7, 3 };
    for (int i = 0; i < 36; ++i) triangles[i] = kFaces[i];
    return 0;
}

} // extern "C"
