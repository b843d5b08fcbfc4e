// tfdm_update_sanitize_main.cpp -- a stand-alone program around the host model of gfx_tfdm_update_heights (tests/tfdm_update_host.cpp)
// for the sanitizers (tools/sanitize_tfdm_update.sh builds it with -fsanitize=address,undefined and runs it; nothing is loaded into
// Python, no GPU).  Every rectangle of a 1, 2, 4 and 8 texel map and 300 seeded rectangles of a 32 texel map through the region
// update against a full build; the whole update (regions, prim_aabb for all triangles, refit) of the unit quad and of a 300-box tree
// with a tenth of its boxes empty; the level table on nodes that are no tree.  Exit status 0 and "ok" = clean.
#include <cstdio>
#include "../tests/tfdm_host.cpp"
#include "../tests/tfdm_update_host.cpp"

namespace {
struct Rng { uint64_t s; double next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return static_cast<double>(s >> 11) * (1.0 / 9007199254740992.0); } };
int fail(const char* what) { std::printf("FAILED: %s\n", what); return 1; }
}

int main() {
    Rng r{ 11 };
    for (uint32_t size : { 1u, 2u, 4u, 8u }) {
        std::vector<float> a(size * size), b(size * size);
        for (float& f : a) f = static_cast<float>(r.next());
        for (float& f : b) f = static_cast<float>(r.next());
        uint32_t n = 0, first[5] = { 0, 0, 0, 0, 0 };
        if (tfdm_update_host_check_all(size, a.data(), b.data(), &n, first) != 0u) return fail("a region update differs from a full build");
    }
    {
        const uint32_t size = 32;
        std::vector<float> a(size * size), b(size * size);
        for (float& f : a) f = static_cast<float>(r.next());
        for (float& f : b) f = static_cast<float>(r.next());
        for (int k = 0; k < 300; ++k) {
            const uint32_t x0 = static_cast<uint32_t>(r.next() * size), y0 = static_cast<uint32_t>(r.next() * size);
            const uint32_t w = 1u + static_cast<uint32_t>(r.next() * (size - x0)), h = 1u + static_cast<uint32_t>(r.next() * (size - y0));
            if (tfdm_update_host_check_rect(size, a.data(), b.data(), x0, y0, w, h) != 0u) return fail("a sampled region update differs from a full build");
        }
    }
    {   // the whole update on the unit quad under a 16 x 16 map
        const uint32_t size = 16;
        std::vector<float> map(size * size), neu(size * size);
        for (float& f : map) f = static_cast<float>(r.next());
        for (float& f : neu) f = static_cast<float>(r.next());
        gfx_vertex v[4];
        std::memset(v, 0, sizeof(v));
        const float pos[4][2] = { { 0, 0 }, { 1, 0 }, { 1, 1 }, { 0, 1 } };
        for (int i = 0; i < 4; ++i) { v[i].position[0] = pos[i][0]; v[i].position[1] = pos[i][1]; v[i].normal[2] = 1.0f; v[i].texCoord[0] = pos[i][0]; v[i].texCoord[1] = pos[i][1]; }
        const uint32_t tris[6] = { 0, 1, 2, 0, 2, 3 };
        gfx_tfdm_params g;
        std::memset(&g, 0, sizeof(g));
        g.hScale = 0.1f; g.texScale[0] = g.texScale[1] = 1.0f; g.localIntersection = 1u;
        Params p;
        tfdm_host_params(&g, size, &p);
        const float* level0 = map.data();
        std::vector<float> levels(tfdm_host_total_texels(size));
        tfdm_host_levels(&level0, 1, size, levels.data());
        std::vector<F2> pyramid(levels.size());
        tfdm_host_pyramid(levels.data(), size, pyramid.data());
        TriRecord recs[2];
        tfdm_host_records(v, tris, 2, &g, size, recs);
        float boxes[12];
        tfdm_host_aabbs(recs, 2, pyramid.data(), &p, boxes);
        Node nodes[4];
        const uint32_t numNodes = tfdm_host_tree(boxes, 2, nodes, 4);
        if (numNodes != 3u) return fail("the quad's tree has three nodes");
        if (tfdm_update_host_update(levels.data(), pyramid.data(), size, neu.data() + 3 * size + 2, size, 2, 3, 9, 7, recs, 2, &p, boxes, nodes, numNodes) != 0)
            return fail("the quad's refit met an empty leaf");
        for (int k = 0; k < 3; ++k)
            if (nodes[0].lo[k] != std::fmin(nodes[1].lo[k], nodes[2].lo[k]) || nodes[0].hi[k] != std::fmax(nodes[1].hi[k], nodes[2].hi[k])) return fail("the root is not the union of its children");
    }
    {   // a 300-box tree, a tenth of the boxes empty; then nodes that are no tree
        const uint32_t n = 300;
        std::vector<float> boxes(6 * n);
        for (uint32_t i = 0; i < n; ++i)
            for (int k = 0; k < 3; ++k) {
                const float c = static_cast<float>(2.0 * r.next() - 1.0), e = static_cast<float>(0.001 + 0.1 * r.next());
                boxes[6 * i + k] = i % 10 == 3 ? INFINITY : c - e;
                boxes[6 * i + 3 + k] = i % 10 == 3 ? -INFINITY : c + e;
            }
        std::vector<Node> nodes(2 * n);
        const uint32_t numNodes = tfdm_host_tree(boxes.data(), n, nodes.data(), 2 * n);
        for (uint32_t i = 0; i < n; ++i)
            if (i % 10 != 3) for (int k = 0; k < 3; ++k) { boxes[6 * i + k] -= 0.01f; boxes[6 * i + 3 + k] += 0.02f; }
        uint32_t depths = 0;
        if (tfdm_update_host_refit(nodes.data(), numNodes, boxes.data(), &depths) != 0 || depths > 21u) return fail("the refit of 300 boxes");
        nodes[0].first = numNodes;                     // a child beyond the array
        if (tfdm_update_host_refit(nodes.data(), numNodes, boxes.data(), nullptr) != -1) return fail("nodes that are no tree were taken");
        nodes[0].first = 0;                            // a cycle
        if (tfdm_update_host_refit(nodes.data(), numNodes, boxes.data(), nullptr) != -1) return fail("a cycle was taken");
        float none[6] = { INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY };
        Node one[1];
        if (tfdm_host_tree(none, 1, one, 1) != 1u || tfdm_update_host_refit(one, 1, none, nullptr) != 1) return fail("the nothing-to-hit tree");
    }
    std::printf("ok\n");
    return 0;
}
