// tfdm_sanitize_main.cpp -- a stand-alone program around the host compilation of csrc/tfdm/tfdm_core.hip.h for the sanitizers
// (tools/sanitize_tfdm_core.sh builds it with -fsanitize=address,undefined and runs it; nothing is loaded into Python).  The flat
// unit quad under a 16 x 16 two-sine map, hScale 0.1, in each local intersection mode: 1500 rays toward the quad, rays from far
// away, rays in the base plane and along texel edges, a zero direction.  Checks what needs no reference: any-hit answers where
// closest-hit does, nothing in a hit is not finite, a miss reports tmax.  Exit status 0 and "ok" = clean.
#include <cmath>
#include <cstdio>
#include "../tests/tfdm_host.cpp"

namespace {
struct Rng { uint64_t s; double next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return static_cast<double>(s >> 11) * (1.0 / 9007199254740992.0); } };
}

int main() {
    const uint32_t size = 16;
    std::vector<float> map(size * size);
    for (uint32_t y = 0; y < size; ++y)
        for (uint32_t x = 0; x < size; ++x) {
            const double a = 2.0 * M_PI / size;
            const double h = 0.5 + 0.25 * std::sin(a * 3 * x) * std::cos(a * 2 * y) + 0.2 * std::sin(a * (5 * x + 7 * y));
            map[y * size + x] = static_cast<float>(std::round(std::fmin(std::fmax(h, 0.0), 1.0) * 255.0)) / 255.0f;
        }
    gfx_vertex v[4];
    std::memset(v, 0, sizeof(v));
    const float pos[4][2] = { { 0, 0 }, { 1, 0 }, { 1, 1 }, { 0, 1 } };
    for (int i = 0; i < 4; ++i) { v[i].position[0] = pos[i][0]; v[i].position[1] = pos[i][1]; v[i].normal[2] = 1.0f; v[i].texCoord[0] = pos[i][0]; v[i].texCoord[1] = pos[i][1]; }
    const uint32_t tris[6] = { 0, 1, 2, 0, 2, 3 };
    const float* level0 = map.data();
    std::vector<float> levels(tfdm_host_total_texels(size));
    tfdm_host_levels(&level0, 1, size, levels.data());
    std::vector<F2> pyramid(levels.size());
    tfdm_host_pyramid(levels.data(), size, pyramid.data());

    std::vector<float> org, dir;
    auto ray = [&](double ox, double oy, double oz, double dx, double dy, double dz, float tmin, float tmax) {
        const float o[4] = { static_cast<float>(ox), static_cast<float>(oy), static_cast<float>(oz), tmin };
        const float d[4] = { static_cast<float>(dx), static_cast<float>(dy), static_cast<float>(dz), tmax };
        org.insert(org.end(), o, o + 4); dir.insert(dir.end(), d, d + 4);
    };
    Rng r{ 7 };
    for (int i = 0; i < 1500; ++i) {
        const double ox = -0.5 + 2.0 * r.next(), oy = -0.5 + 2.0 * r.next(), oz = 0.15 + 0.85 * r.next();
        const double dx = r.next() - ox, dy = r.next() - oy, dz = 0.05 - oz;
        const double back = i % 3 == 0 ? 64.0 / std::sqrt(dx * dx + dy * dy + dz * dz) : 0.0;
        ray(ox - back * dx, oy - back * dy, oz - back * dz, dx, dy, dz, 0.0f, i % 5 == 0 ? 0.9f + static_cast<float>(back) : 3.0e38f);
    }
    for (int k = 0; k <= 16; ++k) {
        ray(k / 16.0, -0.5, 0.05, 0, 1, 0, 0.0f, 3.0e38f);
        ray(-0.5, k / 16.0, 0.0, 1, 0, 0, 0.0f, 3.0e38f);
        ray(k / 16.0, k / 16.0, 0.5, 0, 0, -1, 0.0f, 3.0e38f);
    }
    ray(0.5, 0.5, 0.05, 0, 0, 0, 0.0f, 3.0e38f);
    const uint32_t n = static_cast<uint32_t>(org.size() / 4);

    for (uint32_t local : { 0u, 1u, 4u }) {
        gfx_tfdm_params g;
        std::memset(&g, 0, sizeof(g));
        g.hScale = 0.1f; g.texScale[0] = g.texScale[1] = 1.0f; g.localIntersection = local;
        Params p;
        tfdm_host_params(&g, size, &p);
        TriRecord rec[2];
        tfdm_host_records(v, tris, 2, &g, size, rec);
        float boxes[12];
        tfdm_host_aabbs(rec, 2, pyramid.data(), &p, boxes);
        Node nodes[4];
        const uint32_t numNodes = tfdm_host_tree(boxes, 2, nodes, 4);
        if (numNodes > 4) { std::printf("tree of %u nodes\n", numNodes); return 1; }
        std::vector<gfx_tfdm_hit> hits(n);
        std::vector<uint32_t> occ(n);
        uint64_t counters[4] = { 0, 0, 0, 0 };
        tfdm_host_trace(nodes, rec, levels.data(), pyramid.data(), &p, 0, org.data(), dir.data(), n, hits.data(), counters);
        tfdm_host_trace(nodes, rec, levels.data(), pyramid.data(), &p, 1, org.data(), dir.data(), n, occ.data(), nullptr);
        uint32_t numHits = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const gfx_tfdm_hit& h = hits[i];
            const bool hit = h.primIndex != 0xFFFFFFFFu;
            numHits += hit ? 1u : 0u;
            const bool finite = std::isfinite(h.dist) && std::isfinite(h.bcB) && std::isfinite(h.bcC) && std::isfinite(h.normal[0]) && std::isfinite(h.normal[1]) && std::isfinite(h.normal[2]);
            if (!finite || (occ[i] != 0u) != hit || (!hit && h.dist != dir[4 * i + 3])) { std::printf("mode %u: ray %u is wrong\n", local, i); return 1; }
        }
        std::printf("mode %u: %u of %u rays hit, %.2f texel box tests and %.2f leaf tests per ray\n", local, numHits, n, static_cast<double>(counters[0]) / n, static_cast<double>(counters[1]) / n);
        if (numHits < n / 4) { std::printf("mode %u: the ray set barely hits\n", local); return 1; }
    }
    std::printf("ok\n");
    return 0;
}
