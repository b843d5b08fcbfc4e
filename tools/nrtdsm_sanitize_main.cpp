// nrtdsm_sanitize_main.cpp -- a stand-alone program around the host compilation of csrc/nrtdsm/nrtdsm_core.hip.h for the
// sanitizers (tools/sanitize_nrtdsm_core.sh builds it with -fsanitize=address,undefined and runs it; nothing is loaded into
// Python).  A 3 x 3-quad spherical cap with shared radial normals under a 16 x 16 two-sine map, plain and under a wrapped and
// rotated texture transform: 1500 rays toward the cap, rays from far away, rays along base edges, rays that are NaN, infinite
// or of zero direction.  Checks what needs no reference: any-hit answers where closest-hit does, nothing in a hit is not finite,
// a miss reports tmax, the descent stays below its ceiling.  Then the same object as two NRTDSM instances of a scene (the host
// compilation of csrc/nrtdsm/nrtdsm_instance.hip.h, tests/scene_nrtdsm_host.cpp), as it is and under a mirrored, non-uniformly
// scaled transform, over the same rays: the walk with the world-box cull equals the walk without it, and any-hit answers where
// closest-hit does.  Exit status 0 and "ok" = clean.
#include <cmath>
#include <cstdio>
#include <limits>
#include "../tests/tfdm_host.cpp"
#include "../tests/nrtdsm_host.cpp"
#include "../tests/scene_nrtdsm_host.cpp"

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
    const int q = 3;
    gfx_vertex v[(q + 1) * (q + 1)];
    std::memset(v, 0, sizeof(v));
    for (int j = 0; j <= q; ++j)
        for (int i = 0; i <= q; ++i) {
            const double a = (2.0 * i / q - 1.0) * 0.4, b = (2.0 * j / q - 1.0) * 0.4;
            gfx_vertex& w = v[j * (q + 1) + i];
            const double p[3] = { std::sin(a) * std::cos(b), std::sin(b), std::cos(a) * std::cos(b) };
            for (int k = 0; k < 3; ++k) { w.position[k] = static_cast<float>(p[k]); w.normal[k] = static_cast<float>(p[k]); }
            w.texCoord[0] = 0.05f + 0.9f * i / q; w.texCoord[1] = 0.05f + 0.9f * j / q;
        }
    std::vector<uint32_t> tris;
    for (int j = 0; j < q; ++j)
        for (int i = 0; i < q; ++i) {
            const uint32_t v00 = j * (q + 1) + i, v10 = v00 + 1, v01 = v00 + q + 1, v11 = v01 + 1;
            const uint32_t t[6] = { v00, v10, v11, v00, v11, v01 };
            tris.insert(tris.end(), t, t + 6);
        }
    const uint32_t numTris = static_cast<uint32_t>(tris.size() / 3);
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
        const double ox = -1.0 + 2.0 * r.next(), oy = -1.0 + 2.0 * r.next(), oz = 1.2 + r.next();
        const double dx = -0.4 + 0.8 * r.next() - ox, dy = -0.4 + 0.8 * r.next() - oy, dz = 0.95 - oz;
        const double back = i % 3 == 0 ? 64.0 / std::sqrt(dx * dx + dy * dy + dz * dz) : 0.0;
        ray(ox - back * dx, oy - back * dy, oz - back * dz, dx, dy, dz, 0.0f, i % 5 == 0 ? 0.9f + static_cast<float>(back) : 3.0e38f);
    }
    for (int k = 0; k <= q; ++k) {                          // down the vertex normals and along base edges
        const gfx_vertex& w = v[k * (q + 1) + k];
        ray(2.0 * w.position[0], 2.0 * w.position[1], 2.0 * w.position[2], -w.position[0], -w.position[1], -w.position[2], 0.0f, 3.0e38f);
        ray(-1.0, w.position[1], w.position[2], 1, 0, 0, 0.0f, 3.0e38f);
    }
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    ray(0, 0, 2, 0, 0, 0, 0.0f, 3.0e38f);
    ray(nan, 0, 2, 0, 0, -1, 0.0f, 3.0e38f);
    ray(0, inf, 2, 0, 0, -1, 0.0f, 3.0e38f);
    ray(0, 0, 2, 0, nan, -1, 0.0f, 3.0e38f);
    ray(0, 0, 2, -inf, 0, -1, 0.0f, 3.0e38f);
    ray(0, 0, 2, 0, 0, -1, nan, 3.0e38f);
    const uint32_t n = static_cast<uint32_t>(org.size() / 4), numBad = 6;

    for (int xf = 0; xf < 2; ++xf) {
        gfx_tfdm_params g;
        std::memset(&g, 0, sizeof(g));
        g.hScale = 0.05f; g.texScale[0] = g.texScale[1] = 1.0f; g.localIntersection = 1u;
        if (xf) { g.hOffset = 0.01f; g.hBias = 0.25f; g.texScale[0] = 2.5f; g.texScale[1] = 1.5f; g.texRotation = 30.0f; g.texOffset[0] = 0.3f; g.texOffset[1] = -0.2f; }
        char msg[128];
        if (nrtdsm_host_refuse(&g, msg, sizeof(msg))) { std::printf("refused: %s\n", msg); return 1; }
        Params p;
        tfdm_host_params(&g, size, &p);
        std::vector<nr::PrismRecord> rec(numTris);
        std::vector<float> boxes(6 * numTris);
        nrtdsm_host_records(v, tris.data(), numTris, &g, size, pyramid.data(), &p, rec.data(), boxes.data());
        std::vector<Node> nodes(2 * numTris);
        const uint32_t numNodes = tfdm_host_tree(boxes.data(), numTris, nodes.data(), 2 * numTris);
        if (numNodes > 2 * numTris) { std::printf("tree of %u nodes\n", numNodes); return 1; }
        std::vector<gfx_tfdm_hit> hits(n);
        std::vector<uint32_t> occ(n), iters(n);
        uint64_t counters[4] = { 0, 0, 0, 0 };
        nrtdsm_host_trace(nodes.data(), rec.data(), levels.data(), pyramid.data(), &p, 0, org.data(), dir.data(), n, hits.data(), counters, iters.data());
        nrtdsm_host_trace(nodes.data(), rec.data(), levels.data(), pyramid.data(), &p, 1, org.data(), dir.data(), n, occ.data(), nullptr, nullptr);
        uint32_t numHits = 0, worst = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const gfx_tfdm_hit& h = hits[i];
            const bool hit = h.primIndex != 0xFFFFFFFFu;
            numHits += hit ? 1u : 0u;
            worst = iters[i] > worst ? iters[i] : worst;
            const bool finite = !hit || (std::isfinite(h.dist) && std::isfinite(h.bcB) && std::isfinite(h.bcC) && std::isfinite(h.normal[0]) && std::isfinite(h.normal[1]) && std::isfinite(h.normal[2]));
            const bool missKeepsTmax = hit || std::memcmp(&h.dist, &dir[4 * i + 3], 4) == 0;
            if (!finite || (occ[i] != 0u) != hit || !missKeepsTmax || (i >= n - numBad && (hit || iters[i] != 0u))) { std::printf("transform %d: ray %u is wrong\n", xf, i); return 1; }
        }
        std::printf("transform %d: %u of %u rays hit, %.2f box tests and %.2f leaf tests per ray, at most %u descent iterations\n", xf, numHits, n,
                    static_cast<double>(counters[0]) / n, static_cast<double>(counters[1]) / n, worst);
        if (numHits < n / 4 || worst >= nrtdsm_host_max_descent()) { std::printf("transform %d: the ray set barely hits, or the descent reached its ceiling\n", xf); return 1; }
        // ... as two instances of a scene
        const float ident[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 }, mirrored[12] = { -0.5f, 0, 0, 0.25f, 0, 0, 2, -1.5f, 0, 1, 0, 0.125f };
        const uint64_t ptrs[4] = { reinterpret_cast<uint64_t>(nodes.data()), reinterpret_cast<uint64_t>(rec.data()), reinterpret_cast<uint64_t>(levels.data()),
                                   reinterpret_cast<uint64_t>(pyramid.data()) };
        InstanceRecord table[2];
        if (scene_nrtdsm_host_make_instance(nr::kKindNrtdsm, ident, &nodes[0], ptrs, &p, 1, &table[0], msg, sizeof(msg)) ||
            scene_nrtdsm_host_make_instance(nr::kKindNrtdsm, mirrored, &nodes[0], ptrs, &p, 2, &table[1], msg, sizeof(msg))) { std::printf("make_instance: %s\n", msg); return 1; }
        std::vector<gfx_scene_hit> culled(n), full(n);
        std::vector<uint32_t> occluded(n);
        scene_nrtdsm_host_trace(table, 2, nullptr, 0, org.data(), dir.data(), n, culled.data(), nullptr, 1);
        scene_nrtdsm_host_trace(table, 2, nullptr, 0, org.data(), dir.data(), n, full.data(), nullptr, 0);
        scene_nrtdsm_host_trace(table, 2, nullptr, 1, org.data(), dir.data(), n, occluded.data(), nullptr, 1);
        uint32_t sceneHits = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const bool hit = culled[i].where != 0xFFFFFFFFu;
            sceneHits += hit ? 1u : 0u;
            if (std::memcmp(&culled[i], &full[i], sizeof(gfx_scene_hit)) != 0 || (occluded[i] != 0u) != hit || (hit && (culled[i].where >> 1) > 1u)) { std::printf("transform %d: scene ray %u is wrong\n", xf, i); return 1; }
        }
        std::printf("transform %d: %u of %u rays hit one of the two instances\n", xf, sceneHits, n);
        if (sceneHits < numHits) { std::printf("transform %d: the scene of two instances is hit less often than the object alone\n", xf); return 1; }
    }
    std::printf("ok\n");
    return 0;
}
