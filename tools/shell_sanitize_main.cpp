// shell_sanitize_main.cpp -- a stand-alone program around the host compilation of csrc/nrtdsm/shell_core.hip.h and shell_build.h
// for the sanitizers (tools/sanitize_shell_core.sh builds it with -fsanitize=address,undefined and runs it; nothing is loaded into
// Python).  A 3 x 3-quad spherical cap with shared radial normals under two shell meshes (a box, and the box plus a pyramid) at
// three texture transforms: many small tiles, wrapped and rotated tiles with negative indices, and one tile that holds the whole
// cap.  1500 rays toward the cap, rays from far away, rays along base edges, rays that are NaN, infinite or of zero direction, and
// the builder's refusals.  Checks what needs no reference: any-hit answers where closest-hit does, nothing in a hit is not finite,
// the indices of a hit exist, a miss reports tmax, the iterations stay below their ceiling.  Then two instances of a scene (the host
// compilation of csrc/nrtdsm/shell_instance.hip.h, tests/scene_shell_host.cpp) over the same rays: the shell object under a
// mirrored, non-uniformly scaled transform and an NRTDSM object of the same base mesh under a 16 x 16 map as it is -- the walk with
// the world-box cull equals the walk without it, shell part included, any-hit answers where closest-hit does, and the shell part is
// set only where the shell member wins.  Exit status 0 and "ok" = clean.
#include <cmath>
#include <cstdio>
#include <limits>
#include "../tests/tfdm_host.cpp"
#include "../tests/shell_host.cpp"
#include "../tests/nrtdsm_host.cpp"
#include "../tests/scene_shell_host.cpp"

namespace {
struct Rng { uint64_t s; double next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return static_cast<double>(s >> 11) * (1.0 / 9007199254740992.0); } };
}

int main() {
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

    // the shell meshes
    float boxPos[24];
    for (uint32_t i = 0; i < 8u; ++i) { boxPos[3 * i] = (i & 1u) ? 0.8f : 0.2f; boxPos[3 * i + 1] = (i & 2u) ? 0.8f : 0.2f; boxPos[3 * i + 2] = (i & 4u) ? 0.08f : 0.0f; }
    const uint32_t boxTri[36] = { 0, 2, 3, 0, 3, 1, 4, 5, 7, 4, 7, 6, 0, 4, 6, 0, 6, 2, 1, 3, 7, 1, 7, 5, 0, 1, 5, 0, 5, 4, 2, 6, 7, 2, 7, 3 };
    const float pyrPos[15] = { 0.84f, 0.84f, 0.0f, 0.98f, 0.84f, 0.0f, 0.98f, 0.98f, 0.0f, 0.84f, 0.98f, 0.0f, 0.91f, 0.91f, 0.12f };
    const uint32_t pyrTri[12] = { 0, 1, 4, 1, 2, 4, 2, 3, 4, 3, 0, 4 };
    gfx_shell_geom geoms[9];
    geoms[0] = { boxPos, 12u, 8u, boxTri, 12u };
    geoms[1] = { pyrPos, 12u, 5u, pyrTri, 4u };
    for (int k = 2; k < 9; ++k) geoms[k] = geoms[0];

    // what the builder refuses
    {
        uint32_t nn = 0, nt = 0;
        char msg[160];
        float badPos[24];
        std::memcpy(badPos, boxPos, sizeof(badPos));
        badPos[4] = std::numeric_limits<float>::quiet_NaN();
        gfx_shell_geom bad = geoms[0];
        bad.positions = badPos;
        uint32_t badTri[36];
        std::memcpy(badTri, boxTri, sizeof(badTri));
        badTri[7] = 8u;
        gfx_shell_geom badIndex = geoms[0];
        badIndex.triangles = badTri;
        gfx_shell_geom empty = geoms[0];
        empty.numTriangles = 0u;
        if (!shell_host_build(geoms, 0, nullptr, nullptr, &nn, &nt, msg, sizeof(msg)) || !shell_host_build(geoms, 9, nullptr, nullptr, &nn, &nt, msg, sizeof(msg)) ||
            !shell_host_build(&bad, 1, nullptr, nullptr, &nn, &nt, msg, sizeof(msg)) || !shell_host_build(&badIndex, 1, nullptr, nullptr, &nn, &nt, msg, sizeof(msg)) ||
            !shell_host_build(&empty, 1, nullptr, nullptr, &nn, &nt, msg, sizeof(msg))) { std::printf("a bad shell mesh was accepted\n"); return 1; }
        badPos[4] = 1.5f;
        if (!shell_host_build(&bad, 1, nullptr, nullptr, &nn, &nt, msg, sizeof(msg))) { std::printf("a vertex outside the tile was accepted\n"); return 1; }
    }

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

    // the NRTDSM member of the scene walk: the same base mesh under a 16 x 16 two-sine map
    const uint32_t size = 16;
    std::vector<float> map(size * size);
    for (uint32_t y = 0; y < size; ++y)
        for (uint32_t x = 0; x < size; ++x) {
            const double a = 2.0 * M_PI / size;
            const double h = 0.5 + 0.25 * std::sin(a * 3 * x) * std::cos(a * 2 * y) + 0.2 * std::sin(a * (5 * x + 7 * y));
            map[y * size + x] = static_cast<float>(std::round(std::fmin(std::fmax(h, 0.0), 1.0) * 255.0)) / 255.0f;
        }
    const float* level0 = map.data();
    std::vector<float> levels(tfdm_host_total_texels(size));
    tfdm_host_levels(&level0, 1, size, levels.data());
    std::vector<F2> pyramid(levels.size());
    tfdm_host_pyramid(levels.data(), size, pyramid.data());
    gfx_tfdm_params ng;
    std::memset(&ng, 0, sizeof(ng));
    ng.hScale = 0.05f; ng.texScale[0] = ng.texScale[1] = 1.0f; ng.localIntersection = 1u;
    Params np;
    tfdm_host_params(&ng, size, &np);
    std::vector<nr::PrismRecord> nrec(numTris);
    std::vector<float> nboxes(6 * numTris);
    nrtdsm_host_records(v, tris.data(), numTris, &ng, size, pyramid.data(), &np, nrec.data(), nboxes.data());
    std::vector<Node> nnodes(2 * numTris);
    if (tfdm_host_tree(nboxes.data(), numTris, nnodes.data(), 2 * numTris) > 2 * numTris) { std::printf("tree of the NRTDSM member\n"); return 1; }

    for (int xf = 0; xf < 3; ++xf) {
        const uint32_t numGeoms = xf == 1 ? 2u : 1u;
        gfx_tfdm_params g;
        std::memset(&g, 0, sizeof(g));
        g.hScale = 4.0f; g.texScale[0] = g.texScale[1] = 12.0f;
        if (xf == 1) { g.hOffset = 0.01f; g.hBias = 0.02f; g.texScale[0] = 9.0f; g.texScale[1] = 7.0f; g.texRotation = 30.0f; g.texOffset[0] = -2.3f; g.texOffset[1] = -1.6f; }
        if (xf == 2) { g.hScale = 1.0f; g.texScale[0] = g.texScale[1] = 0.8f; g.texOffset[0] = g.texOffset[1] = 0.1f; }
        char msg[160];
        if (shell_host_refuse(&g, msg, sizeof(msg))) { std::printf("refused: %s\n", msg); return 1; }
        uint32_t numShellNodes = 0, numShellTris = 0;
        if (shell_host_build(geoms, numGeoms, nullptr, nullptr, &numShellNodes, &numShellTris, msg, sizeof(msg))) { std::printf("refused: %s\n", msg); return 1; }
        std::vector<Node> shellNodes(numShellNodes);
        std::vector<sh::ShellTri> shellTris(numShellTris);
        shell_host_build(geoms, numGeoms, shellNodes.data(), shellTris.data(), &numShellNodes, &numShellTris, msg, sizeof(msg));
        Params p;
        shell_host_params(&g, &p);
        std::vector<nr::PrismRecord> rec(numTris);
        std::vector<float> boxes(6 * numTris);
        if (shell_host_records(v, tris.data(), numTris, &g, shellNodes.data(), shellTris.data(), rec.data(), boxes.data())) { std::printf("tile coordinates out of range\n"); return 1; }
        std::vector<Node> nodes(2 * numTris);
        const uint32_t numNodes = tfdm_host_tree(boxes.data(), numTris, nodes.data(), 2 * numTris);
        if (numNodes > 2 * numTris) { std::printf("tree of %u nodes\n", numNodes); return 1; }
        std::vector<int32_t> ids(4 * 4096);
        std::vector<float> walked(6 * 4096);
        for (uint32_t t = 0; t < numTris; ++t) shell_host_walk(&rec[t], shellNodes.data(), ids.data(), walked.data(), 4096);
        std::vector<gfx_shell_hit> hits(n);
        std::vector<uint32_t> occ(n), iters(n);
        uint64_t counters[4] = { 0, 0, 0, 0 };
        shell_host_trace(nodes.data(), rec.data(), shellNodes.data(), shellTris.data(), &p, 0, org.data(), dir.data(), n, hits.data(), counters, iters.data());
        shell_host_trace(nodes.data(), rec.data(), shellNodes.data(), shellTris.data(), &p, 1, org.data(), dir.data(), n, occ.data(), nullptr, nullptr);
        uint32_t numHits = 0, worst = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const gfx_shell_hit& h = hits[i];
            const bool hit = h.primIndex != 0xFFFFFFFFu;
            numHits += hit ? 1u : 0u;
            worst = iters[i] > worst ? iters[i] : worst;
            const bool finite = !hit || (std::isfinite(h.dist) && std::isfinite(h.bcB) && std::isfinite(h.bcC) && std::isfinite(h.normal[0]) && std::isfinite(h.normal[1]) && std::isfinite(h.normal[2]));
            const bool indices = hit ? (h.primIndex < numTris && h.shellTriangle < numShellTris && h.shellGeom < numGeoms && shellTris[h.shellTriangle].geom == h.shellGeom)
                                     : (h.shellTriangle == 0u && h.shellGeom == 0u && h.tile[0] == 0 && h.tile[1] == 0);
            const bool missKeepsTmax = hit || std::memcmp(&h.dist, &dir[4 * i + 3], 4) == 0;
            if (!finite || !indices || (occ[i] != 0u) != hit || !missKeepsTmax || (i >= n - numBad && (hit || iters[i] != 0u))) { std::printf("transform %d: ray %u is wrong\n", xf, i); return 1; }
        }
        std::printf("transform %d: %u of %u rays hit, %.2f box tests and %.2f leaf tests per ray, at most %u iterations\n", xf, numHits, n,
                    static_cast<double>(counters[0]) / n, static_cast<double>(counters[1]) / n, worst);
        if (numHits < n / 8 || worst >= shell_host_max_descent()) { std::printf("transform %d: the ray set barely hits, or the traversal reached its ceiling\n", xf); return 1; }
        // ... as two instances of a scene: the shell mirrored and non-uniformly scaled, the NRTDSM object as it is
        const float ident[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 }, mirrored[12] = { -1.25f, 0, 0, 0.1f, 0, 0.75f, 0, 0.05f, 0, 0, 1.5f, -0.5f };      // the cap stays under the rays
        const uint64_t shellPtrs[4] = { reinterpret_cast<uint64_t>(nodes.data()), reinterpret_cast<uint64_t>(rec.data()), reinterpret_cast<uint64_t>(shellNodes.data()),
                                        reinterpret_cast<uint64_t>(shellTris.data()) };
        const uint64_t nrtdsmPtrs[4] = { reinterpret_cast<uint64_t>(nnodes.data()), reinterpret_cast<uint64_t>(nrec.data()), reinterpret_cast<uint64_t>(levels.data()),
                                         reinterpret_cast<uint64_t>(pyramid.data()) };
        InstanceRecord table[2];
        if (scene_shell_host_make_instance(sh::kKindShell, mirrored, &nodes[0], shellPtrs, &p, 1, &table[0], msg, sizeof(msg)) ||
            scene_shell_host_make_instance(nr::kKindNrtdsm, ident, &nnodes[0], nrtdsmPtrs, &np, 2, &table[1], msg, sizeof(msg))) { std::printf("make_instance: %s\n", msg); return 1; }
        std::vector<gfx_scene_hit> culled(n), full(n);
        std::vector<gfx_scene_shell_part> culledPart(n), fullPart(n);
        std::vector<uint32_t> occluded(n);
        scene_shell_host_trace(table, 2, nullptr, 0, org.data(), dir.data(), n, culled.data(), culledPart.data(), nullptr, 1);
        scene_shell_host_trace(table, 2, nullptr, 0, org.data(), dir.data(), n, full.data(), fullPart.data(), nullptr, 0);
        scene_shell_host_trace(table, 2, nullptr, 1, org.data(), dir.data(), n, occluded.data(), nullptr, nullptr, 1);
        uint32_t sceneHits[2] = { 0, 0 };
        for (uint32_t i = 0; i < n; ++i) {
            const bool hit = culled[i].where != 0xFFFFFFFFu;
            const uint32_t member = culled[i].where >> 1;
            const gfx_scene_shell_part& sp = culledPart[i];
            const bool onShell = hit && member == 0u;
            const bool partOk = onShell ? (sp.shellTriangle < numShellTris && sp.shellGeom < numGeoms && shellTris[sp.shellTriangle].geom == sp.shellGeom)
                                        : (sp.shellTriangle == 0u && sp.shellGeom == 0u && sp.tile[0] == 0 && sp.tile[1] == 0);
            if (std::memcmp(&culled[i], &full[i], sizeof(gfx_scene_hit)) != 0 || std::memcmp(&sp, &fullPart[i], sizeof(sp)) != 0 || (occluded[i] != 0u) != hit ||
                (hit && member > 1u) || !partOk) { std::printf("transform %d: scene ray %u is wrong\n", xf, i); return 1; }
            if (hit) ++sceneHits[member];
        }
        std::printf("transform %d: %u rays end on the mirrored shell instance, %u on the NRTDSM instance\n", xf, sceneHits[0], sceneHits[1]);
        if (sceneHits[0] == 0u || sceneHits[1] < n / 8) { std::printf("transform %d: a member of the scene of two instances is not seen\n", xf); return 1; }
    }
    std::printf("ok\n");
    return 0;
}
