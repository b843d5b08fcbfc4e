// street_scene.cpp -- gfxh_scene_make_street: the procedural "street" scene standing in for Bistro Exterior (not present offline),
// the workload of bench.py.  tests/golden/street_digest.json pins every byte of what it builds.
#include <cstring>
#include <random>
#include "host_scene.h"

using namespace gfx_host;

namespace {

// ---- primitive meshes for the procedural scene
void add_quad(Geom& g, V3 p0, V3 p1, V3 p2, V3 p3) { // CCW p0..p3
    const V3 n = normalize(cross(p1 - p0, p3 - p0));
    const V3 t = normalize(p1 - p0);
    const uint32_t b = static_cast<uint32_t>(g.v.size());
    g.v.push_back(make_vertex(p0, n, t, 0, 0));
    g.v.push_back(make_vertex(p1, n, t, 1, 0));
    g.v.push_back(make_vertex(p2, n, t, 1, 1));
    g.v.push_back(make_vertex(p3, n, t, 0, 1));
    const uint32_t idx[6] = { b, b + 1, b + 2, b, b + 2, b + 3 };
    g.t.insert(g.t.end(), idx, idx + 6);
}
void add_box(Geom& g, V3 lo, V3 hi) {
    const V3 c[8] = { { lo.x, lo.y, lo.z }, { hi.x, lo.y, lo.z }, { hi.x, hi.y, lo.z }, { lo.x, hi.y, lo.z },
                      { lo.x, lo.y, hi.z }, { hi.x, lo.y, hi.z }, { hi.x, hi.y, hi.z }, { lo.x, hi.y, hi.z } };
    add_quad(g, c[1], c[0], c[3], c[2]);  // -z
    add_quad(g, c[4], c[5], c[6], c[7]);  // +z
    add_quad(g, c[0], c[4], c[7], c[3]);  // -x
    add_quad(g, c[5], c[1], c[2], c[6]);  // +x
    add_quad(g, c[3], c[7], c[6], c[2]);  // +y
    add_quad(g, c[0], c[1], c[5], c[4]);  // -y
}
// grid of quads on the plane spanned by (ex, ey) from origin o, displaced along the normal by h(i,j)
template <typename H>
void add_grid(Geom& g, V3 o, V3 ex, V3 ey, uint32_t nx, uint32_t ny, H height) {
    const V3 n = normalize(cross(ex, ey));
    const V3 t = normalize(ex);
    const uint32_t b = static_cast<uint32_t>(g.v.size());
    for (uint32_t j = 0; j <= ny; ++j)
        for (uint32_t i = 0; i <= nx; ++i) {
            const float u = static_cast<float>(i) / nx, v = static_cast<float>(j) / ny;
            const V3 p = o + ex * u + ey * v + n * height(i, j);
            g.v.push_back(make_vertex(p, n, t, u, v));
        }
    for (uint32_t j = 0; j < ny; ++j)
        for (uint32_t i = 0; i < nx; ++i) {
            const uint32_t a = b + j * (nx + 1) + i, c = a + 1, d = a + nx + 1, e = d + 1;
            const uint32_t idx[6] = { a, c, e, a, e, d };
            g.t.insert(g.t.end(), idx, idx + 6);
        }
}
void make_icosphere(Geom& g, uint32_t subdiv, float radius) {
    const float t = (1.0f + std::sqrt(5.0f)) / 2.0f;
    std::vector<V3> p = { { -1, t, 0 }, { 1, t, 0 }, { -1, -t, 0 }, { 1, -t, 0 }, { 0, -1, t }, { 0, 1, t },
                          { 0, -1, -t }, { 0, 1, -t }, { t, 0, -1 }, { t, 0, 1 }, { -t, 0, -1 }, { -t, 0, 1 } };
    for (V3& v : p) v = normalize(v);
    std::vector<uint32_t> f = { 0, 11, 5, 0, 5, 1, 0, 1, 7, 0, 7, 10, 0, 10, 11, 1, 5, 9, 5, 11, 4, 11, 10, 2, 10, 7, 6, 7, 1, 8,
                                3, 9, 4, 3, 4, 2, 3, 2, 6, 3, 6, 8, 3, 8, 9, 4, 9, 5, 2, 4, 11, 6, 2, 10, 8, 6, 7, 9, 8, 1 };
    for (uint32_t s = 0; s < subdiv; ++s) {
        std::map<std::pair<uint32_t, uint32_t>, uint32_t> mid;
        auto midpoint = [&](uint32_t a, uint32_t b) {
            const auto key = std::make_pair(std::min(a, b), std::max(a, b));
            auto it = mid.find(key);
            if (it != mid.end()) return it->second;
            p.push_back(normalize((p[a] + p[b]) * 0.5f));
            const uint32_t idx = static_cast<uint32_t>(p.size() - 1);
            mid[key] = idx;
            return idx;
        };
        std::vector<uint32_t> nf;
        for (size_t i = 0; i < f.size(); i += 3) {
            const uint32_t a = f[i], b = f[i + 1], c = f[i + 2];
            const uint32_t ab = midpoint(a, b), bc = midpoint(b, c), ca = midpoint(c, a);
            const uint32_t tri[12] = { a, ab, ca, b, bc, ab, c, ca, bc, ab, bc, ca };
            nf.insert(nf.end(), tri, tri + 12);
        }
        f.swap(nf);
    }
    const uint32_t b = static_cast<uint32_t>(g.v.size());
    for (const V3& n : p) {
        const V3 tg = normalize(tangent_from_normal(n));
        const float u = 0.5f + std::atan2(n.z, n.x) / (2 * 3.14159265f), v = 0.5f - std::asin(std::min(1.0f, std::max(-1.0f, n.y))) / 3.14159265f;
        g.v.push_back(make_vertex(n * radius, n, tg, u, v));
    }
    for (uint32_t idx : f) g.t.push_back(b + idx);
}

struct Rng {
    std::mt19937 gen;
    explicit Rng(uint32_t seed) : gen(seed) {}
    float uni() { return (gen() >> 8) * (1.0f / 16777216.0f); }
    float range(float a, float b) { return a + (b - a) * uni(); }
};

} // namespace

extern "C" int gfxh_scene_make_street(gfxh_scene* s, const gfxh_street_params* p) {
    Rng rng(p->seed);
    const float E = p->extent;
    auto mat = [&](float r, float g, float b, float sr, float sm, float e0 = 0, float e1 = 0, float e2 = 0) {
        const float d[3] = { r, g, b }, sp[3] = { sr, sr, sr }, em[3] = { e0, e1, e2 };
        return gfxh_scene_add_material_traditional(s, d, sp, sm, em);
    };
    const float ident[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
    uint32_t groundMat = 0, groundGeom = 0, crateMat = 0;
    std::vector<uint32_t> wallMats, signMats;
    // ---- ground: cobbled street (height noise) as one big static instance
    {
        Geom g; g.mat = mat(0.35f, 0.33f, 0.30f, 0.2f, 0.2f);
        groundMat = g.mat;
        std::mt19937 hgen(p->seed * 7919u + 1);
        std::vector<float> h((p->groundTess + 1) * (p->groundTess + 1));
        for (float& v : h) v = ((hgen() >> 8) * (1.0f / 16777216.0f)) * 0.02f;
        const uint32_t nt = p->groundTess;
        add_grid(g, { -E, 0, E }, { 2 * E, 0, 0 }, { 0, 0, -2 * E }, nt, nt, [&](uint32_t i, uint32_t j) { return h[j * (nt + 1) + i]; });
        s->geoms.push_back(std::move(g));
        const uint32_t gs = static_cast<uint32_t>(s->geoms.size() - 1);
        groundGeom = gs;
        gfxh_scene_add_instance(s, gfxh_scene_add_group(s, &gs, 1), ident);
    }
    // ---- buildings: a few facade prototypes (wall grid with recessed windows + roof box), instanced
    const uint32_t numProto = 6;
    std::vector<uint32_t> protoGroups;
    std::vector<V3> protoSize;
    for (uint32_t k = 0; k < numProto; ++k) {
        const float w = rng.range(6, 14), hgt = rng.range(8, 22), dpt = rng.range(6, 12);
        Geom wall; wall.mat = mat(rng.range(0.4f, 0.8f), rng.range(0.35f, 0.7f), rng.range(0.3f, 0.6f), 0.04f, 0.1f);
        wallMats.push_back(wall.mat);
        Geom glass; glass.mat = mat(0.05f, 0.06f, 0.08f, 0.6f, 0.85f);
        const uint32_t ft = p->facadeTess;
        // four facades: displaced grids (window recesses) facing outward
        const V3 o[4] = { { -w / 2, 0, dpt / 2 }, { w / 2, 0, dpt / 2 }, { w / 2, 0, -dpt / 2 }, { -w / 2, 0, -dpt / 2 } };
        const V3 ex[4] = { { w, 0, 0 }, { 0, 0, -dpt }, { -w, 0, 0 }, { 0, 0, dpt } };
        for (int f = 0; f < 4; ++f) {
            add_grid(wall, o[f], ex[f], { 0, hgt, 0 }, ft, ft, [&](uint32_t i, uint32_t j) {
                const bool window = (i % 4 == 1 || i % 4 == 2) && (j % 4 == 1 || j % 4 == 2) && j > 3;
                return window ? -0.25f : 0.0f;
            });
        }
        add_box(wall, { -w / 2, hgt, -dpt / 2 }, { w / 2, hgt + 0.4f, dpt / 2 });
        // glass panes inside the recesses of the front facade
        for (uint32_t j = 5; j + 2 < ft; j += 4)
            for (uint32_t i = 1; i + 2 < ft; i += 4) {
                const float x0 = -w / 2 + w * (i + 0.1f) / ft, x1 = -w / 2 + w * (i + 1.9f) / ft;
                const float y0 = hgt * (j + 0.1f) / ft, y1 = hgt * (j + 1.9f) / ft;
                add_quad(glass, { x0, y0, dpt / 2 - 0.2f }, { x1, y0, dpt / 2 - 0.2f }, { x1, y1, dpt / 2 - 0.2f }, { x0, y1, dpt / 2 - 0.2f });
            }
        s->geoms.push_back(std::move(wall));
        s->geoms.push_back(std::move(glass));
        const uint32_t gs[2] = { static_cast<uint32_t>(s->geoms.size() - 2), static_cast<uint32_t>(s->geoms.size() - 1) };
        protoGroups.push_back(gfxh_scene_add_group(s, gs, 2));
        protoSize.push_back({ w, hgt, dpt });
    }
    struct Placed { V3 pos; float yaw; uint32_t proto; };
    std::vector<Placed> placed;
    for (uint32_t b = 0; b < p->numBuildings; ++b) {
        // two rows along the street (z axis), facing the street
        const bool left = (b & 1) != 0;
        const float z = -E * 0.9f + (2 * E * 0.9f) * (static_cast<float>(b / 2) + 0.5f) / std::max(1u, (p->numBuildings + 1) / 2);
        const uint32_t proto = rng.gen() % numProto;
        const float x = (left ? -1.0f : 1.0f) * (E * 0.35f + protoSize[proto].z * 0.5f);
        const float yaw = left ? 90.0f : -90.0f;
        const float pos[3] = { x, 0, z };
        float xfm[12];
        gfxh_make_transform(1.0f, 0, 0, yaw, pos, xfm);
        gfxh_scene_add_instance(s, protoGroups[proto], xfm);
        placed.push_back({ { x, 0, z }, yaw, proto });
    }
    // ---- props: icospheres (planters / bollards) and crates, instanced with random scale
    {
        Geom sphere; sphere.mat = mat(0.55f, 0.25f, 0.2f, 0.1f, 0.5f);
        make_icosphere(sphere, p->propSubdiv, 0.5f);
        Geom crate; crate.mat = mat(0.45f, 0.32f, 0.18f, 0.03f, 0.2f);
        crateMat = crate.mat;
        add_box(crate, { -0.5f, 0, -0.5f }, { 0.5f, 1, 0.5f });
        s->geoms.push_back(std::move(sphere));
        const uint32_t gsph = static_cast<uint32_t>(s->geoms.size() - 1);
        s->geoms.push_back(std::move(crate));
        const uint32_t gcr = static_cast<uint32_t>(s->geoms.size() - 1);
        const uint32_t grpS = gfxh_scene_add_group(s, &gsph, 1), grpC = gfxh_scene_add_group(s, &gcr, 1);
        for (uint32_t k = 0; k < p->numProps; ++k) {
            const bool sph = (k % 3) != 0;
            const float sc = rng.range(0.3f, 1.2f);
            const float pos[3] = { rng.range(-E * 0.33f, E * 0.33f), sph ? sc * 0.5f : 0.0f, rng.range(-E * 0.95f, E * 0.95f) };
            float xfm[12];
            gfxh_make_transform(sc, 0, 0, rng.range(0, 360), pos, xfm);
            gfxh_scene_add_instance(s, sph ? grpS : grpC, xfm);
        }
    }
    // ---- lamps: pole + small emissive box head; a handful of colour temperatures
    {
        Geom pole; pole.mat = mat(0.1f, 0.1f, 0.1f, 0.3f, 0.6f);
        add_box(pole, { -0.05f, 0, -0.05f }, { 0.05f, 3.5f, 0.05f });
        s->geoms.push_back(std::move(pole));
        const uint32_t gpole = static_cast<uint32_t>(s->geoms.size() - 1);
        std::vector<uint32_t> lampGroups;
        const float tints[4][3] = { { 1.0f, 0.85f, 0.6f }, { 1.0f, 0.95f, 0.85f }, { 0.8f, 0.9f, 1.0f }, { 1.0f, 0.7f, 0.4f } };
        for (int k = 0; k < 4; ++k) {
            Geom head; head.mat = mat(0.01f, 0.01f, 0.01f, 0, 0.3f, p->lampEmittance * tints[k][0], p->lampEmittance * tints[k][1], p->lampEmittance * tints[k][2]);
            add_box(head, { -0.15f, 3.5f, -0.15f }, { 0.15f, 3.7f, 0.15f });
            s->geoms.push_back(std::move(head));
            const uint32_t gs[2] = { gpole, static_cast<uint32_t>(s->geoms.size() - 1) };
            lampGroups.push_back(gfxh_scene_add_group(s, gs, 2));
        }
        for (uint32_t k = 0; k < p->numLamps; ++k) {
            const float pos[3] = { rng.range(-E * 0.34f, E * 0.34f), 0, rng.range(-E * 0.95f, E * 0.95f) };
            float xfm[12];
            gfxh_make_transform(rng.range(0.8f, 1.2f), 0, 0, rng.range(0, 360), pos, xfm);
            gfxh_scene_add_instance(s, lampGroups[rng.gen() % 4], xfm);
        }
    }
    // ---- signs: emissive quads mounted on facades
    {
        std::vector<uint32_t> signGroups;
        const float cols[5][3] = { { 1, 0.2f, 0.2f }, { 0.2f, 1, 0.3f }, { 0.2f, 0.4f, 1 }, { 1, 0.9f, 0.2f }, { 1, 0.3f, 0.9f } };
        for (int k = 0; k < 5; ++k) {
            Geom sign; sign.mat = mat(0.01f, 0.01f, 0.01f, 0, 0.3f, p->signEmittance * cols[k][0], p->signEmittance * cols[k][1], p->signEmittance * cols[k][2]);
            signMats.push_back(sign.mat);
            add_grid(sign, { -0.6f, -0.2f, 0 }, { 1.2f, 0, 0 }, { 0, 0.4f, 0 }, 4, 2, [](uint32_t, uint32_t) { return 0.0f; });
            s->geoms.push_back(std::move(sign));
            const uint32_t gs = static_cast<uint32_t>(s->geoms.size() - 1);
            signGroups.push_back(gfxh_scene_add_group(s, &gs, 1));
        }
        for (uint32_t k = 0; k < p->numSigns && !placed.empty(); ++k) {
            const Placed& b = placed[rng.gen() % placed.size()];
            const V3 sz = protoSize[b.proto];
            // local position on the front facade (+z of the prototype), slightly in front of it
            const float lp[3] = { rng.range(-sz.x * 0.4f, sz.x * 0.4f), rng.range(2.5f, std::max(3.0f, sz.y * 0.8f)), sz.z * 0.5f + 0.05f };
            float bx[12];
            const float bpos[3] = { b.pos.x, b.pos.y, b.pos.z };
            gfxh_make_transform(1.0f, 0, 0, b.yaw, bpos, bx);
            float wp[3];
            xfm_point(bx, lp, wp);
            float xfm[12];
            gfxh_make_transform(rng.range(0.7f, 1.6f), 0, 0, b.yaw, wp, xfm);
            gfxh_scene_add_instance(s, signGroups[rng.gen() % 5], xfm);
        }
    }
    // ---- depth complexity (p->numTrees, p->numWires, p->numRailings): what Bistro's vegetation, cables and balcony railings
    // do to a ray tracer -- clumps of small randomly oriented leaf cards (thousands of overlapping boxes a ray grazes without
    // hitting anything), and long thin boxes whose bounding volumes cover mostly air.  Own RNG stream: scenes without these
    // parameters are unchanged.
    if (p->numTrees || p->numWires || p->numRailings) {
        Rng crng(p->seed * 747796405u + 2891336453u);
        const uint32_t leafMat = mat(0.12f, 0.32f, 0.08f, 0.04f, 0.3f), barkMat = mat(0.25f, 0.18f, 0.12f, 0.02f, 0.1f), metalMat = mat(0.3f, 0.3f, 0.32f, 0.5f, 0.7f);
        if (p->numTrees) {
            std::vector<uint32_t> treeGroups;
            for (int proto = 0; proto < 3; ++proto) {
                Geom trunk; trunk.mat = barkMat;
                const float th = crng.range(2.5f, 3.5f);
                add_box(trunk, { -0.12f, 0, -0.12f }, { 0.12f, th, 0.12f });
                Geom leaves; leaves.mat = leafMat;
                const float rx = crng.range(1.4f, 2.2f), ry = crng.range(1.2f, 2.0f), rz = crng.range(1.4f, 2.2f);
                for (uint32_t k = 0; k < p->leavesPerTree; ++k) {
                    // a point inside the crown ellipsoid (rejection), a random card orientation, 12-30 cm
                    V3 c;
                    do { c = { crng.range(-1, 1), crng.range(-1, 1), crng.range(-1, 1) }; } while (c.x * c.x + c.y * c.y + c.z * c.z > 1.0f);
                    c = { c.x * rx, th + ry * 0.8f + c.y * ry, c.z * rz };
                    V3 u = normalize({ crng.range(-1, 1), crng.range(-1, 1), crng.range(-1, 1) });
                    V3 w = normalize(cross(u, { crng.range(-1, 1), crng.range(-1, 1) + 1.5f, crng.range(-1, 1) }));
                    const float hs = crng.range(0.06f, 0.15f);
                    const V3 a = { u.x * hs, u.y * hs, u.z * hs }, b = { w.x * hs, w.y * hs, w.z * hs };
                    add_quad(leaves, c - a - b, c + a - b, c + a + b, c - a + b);
                }
                s->geoms.push_back(std::move(trunk));
                s->geoms.push_back(std::move(leaves));
                const uint32_t gs[2] = { static_cast<uint32_t>(s->geoms.size() - 2), static_cast<uint32_t>(s->geoms.size() - 1) };
                treeGroups.push_back(gfxh_scene_add_group(s, gs, 2));
            }
            for (uint32_t k = 0; k < p->numTrees; ++k) {   // two rows along the kerbs
                const float side = (k & 1u) ? 1.0f : -1.0f;
                const float pos[3] = { side * E * crng.range(0.22f, 0.3f), 0, -E * 0.92f + 2 * E * 0.92f * (static_cast<float>(k / 2) + crng.range(0.2f, 0.8f)) / std::max(1u, (p->numTrees + 1) / 2) };
                float xfm[12];
                gfxh_make_transform(crng.range(0.8f, 1.3f), 0, 0, crng.range(0, 360), pos, xfm);
                gfxh_scene_add_instance(s, treeGroups[crng.gen() % 3], xfm);
            }
        }
        if (p->numWires) {   // cables across the street between the facade rows, slightly sagging: 8 thin segments each
            Geom wires; wires.mat = metalMat;
            for (uint32_t k = 0; k < p->numWires; ++k) {
                const float z0 = crng.range(-E * 0.9f, E * 0.9f), z1 = z0 + crng.range(-6.0f, 6.0f), y = crng.range(5.0f, 9.0f);
                const float x0 = -E * 0.36f, x1 = E * 0.36f, r = 0.015f;
                for (int sgm = 0; sgm < 8; ++sgm) {
                    const float t0 = sgm / 8.0f, t1 = (sgm + 1) / 8.0f;
                    const float xa = x0 + (x1 - x0) * t0, xb = x0 + (x1 - x0) * t1, za = z0 + (z1 - z0) * t0, zb = z0 + (z1 - z0) * t1;
                    const float ya = y - 1.2f * 4 * t0 * (1 - t0), yb = y - 1.2f * 4 * t1 * (1 - t1);
                    // a box around the segment, axis-aligned in x (the sag and the skew make its BVH box mostly empty)
                    add_quad(wires, { xa, ya - r, za - r }, { xb, yb - r, zb - r }, { xb, yb + r, zb - r }, { xa, ya + r, za - r });
                    add_quad(wires, { xa, ya + r, za + r }, { xb, yb + r, zb + r }, { xb, yb - r, zb + r }, { xa, ya - r, za + r });
                    add_quad(wires, { xa, ya + r, za - r }, { xb, yb + r, zb - r }, { xb, yb + r, zb + r }, { xa, ya + r, za + r });
                    add_quad(wires, { xa, ya - r, za + r }, { xb, yb - r, zb + r }, { xb, yb - r, zb - r }, { xa, ya - r, za - r });
                }
            }
            s->geoms.push_back(std::move(wires));
            const uint32_t gs = static_cast<uint32_t>(s->geoms.size() - 1);
            gfxh_scene_add_instance(s, gfxh_scene_add_group(s, &gs, 1), ident);
        }
        if (p->numRailings) {   // a railing segment = two rails + 24 thin bars, instanced along the kerbs
            Geom rail; rail.mat = metalMat;
            add_box(rail, { -1.5f, 0.95f, -0.02f }, { 1.5f, 1.0f, 0.02f });
            add_box(rail, { -1.5f, 0.1f, -0.02f }, { 1.5f, 0.14f, 0.02f });
            for (int b = 0; b < 24; ++b) { const float x = -1.5f + 3.0f * (b + 0.5f) / 24; add_box(rail, { x - 0.008f, 0.14f, -0.008f }, { x + 0.008f, 0.95f, 0.008f }); }
            s->geoms.push_back(std::move(rail));
            const uint32_t gs = static_cast<uint32_t>(s->geoms.size() - 1);
            const uint32_t grp = gfxh_scene_add_group(s, &gs, 1);
            for (uint32_t k = 0; k < p->numRailings; ++k) {
                const float side = (k & 1u) ? 1.0f : -1.0f;
                const float pos[3] = { side * E * 0.2f, 0, -E * 0.95f + 2 * E * 0.95f * (static_cast<float>(k / 2) + 0.5f) / std::max(1u, (p->numRailings + 1) / 2) };
                float xfm[12];
                gfxh_make_transform(1.0f, 0, 0, 90.0f, pos, xfm);
                gfxh_scene_add_instance(s, grp, xfm);
            }
        }
    }
    // ---- textures (p->textured): the geometry above is unchanged, materials get maps instead of constants --
    // cobbled ground and plastered / bricked facades with albedo, smoothness and normal maps, wooden crates, and
    // signs whose emittance is a float texture (lettering-like stripes), so every texture fetch of the reference
    // path is exercised: setupBSDFBody's three reads, the normal map under bump mapping, and the emittance reads of
    // sampleLight, the shading pass and computeTriangleImportance.
    if (p->textured) {
        std::mt19937 tgen(p->seed * 2654435761u + 17u);
        auto hash01 = [](uint32_t x, uint32_t y, uint32_t k) {   // integer hash -> [0, 1)
            uint32_t h = x * 0x9E3779B1u ^ (y * 0x85EBCA77u + k * 0xC2B2AE3Du);
            h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15;
            return (h >> 8) * (1.0f / 16777216.0f);
        };
        auto to8 = [](float v) { return static_cast<uint8_t>(std::min(255.0f, std::max(0.0f, v * 255.0f + 0.5f))); };
        // height field of a tiling pattern: cells of (cw x ch) texels with a groove of `gap` texels, per-cell tint
        auto tile_maps = [&](uint32_t N, uint32_t cw, uint32_t ch, uint32_t gap, bool stagger, const float base[3], float tintAmp, uint32_t salt,
                             std::vector<uint8_t>& albedo, std::vector<uint8_t>& normal, std::vector<uint8_t>& smooth) {
            std::vector<float> height(static_cast<size_t>(N) * N);
            albedo.resize(4ull * N * N); normal.resize(4ull * N * N); smooth.resize(static_cast<size_t>(N) * N);
            for (uint32_t y = 0; y < N; ++y)
                for (uint32_t x = 0; x < N; ++x) {
                    const uint32_t row = y / ch;
                    const uint32_t xs = stagger && (row & 1u) ? x + cw / 2 : x;
                    const uint32_t col = (xs / cw) % (N / cw);
                    const uint32_t ix = xs % cw, iy = y % ch;
                    const bool groove = ix < gap || iy < gap;
                    const float grain = hash01(x, y, salt);
                    const float tint = 1.0f + tintAmp * (hash01(col, row, salt + 1) - 0.5f);
                    height[static_cast<size_t>(y) * N + x] = groove ? 0.0f : 0.7f + 0.3f * grain;
                    uint8_t* a = albedo.data() + 4ull * (static_cast<size_t>(y) * N + x);
                    for (int c = 0; c < 3; ++c) a[c] = to8((groove ? 0.45f : 1.0f) * base[c] * tint * (0.9f + 0.2f * grain));
                    a[3] = 255;
                    smooth[static_cast<size_t>(y) * N + x] = to8(groove ? 0.05f : 0.15f + 0.25f * hash01(col, row, salt + 2));
                }
            for (uint32_t y = 0; y < N; ++y)
                for (uint32_t x = 0; x < N; ++x) {
                    const float hx = height[static_cast<size_t>(y) * N + (x + 1) % N] - height[static_cast<size_t>(y) * N + (x + N - 1) % N];
                    const float hy = height[static_cast<size_t>((y + 1) % N) * N + x] - height[static_cast<size_t>((y + N - 1) % N) * N + x];
                    const V3 n = normalize({ -1.5f * hx, -1.5f * hy, 1.0f });
                    uint8_t* o = normal.data() + 4ull * (static_cast<size_t>(y) * N + x);
                    o[0] = to8(0.5f * n.x + 0.5f); o[1] = to8(0.5f * n.y + 0.5f); o[2] = to8(0.5f * n.z + 0.5f); o[3] = 255;
                }
        };
        auto texture_material = [&](uint32_t matSlot, uint32_t N, uint32_t cw, uint32_t ch, uint32_t gap, bool stagger, const float base[3], float tintAmp) {
            std::vector<uint8_t> albedo, normal, smooth;
            tile_maps(N, cw, ch, gap, stagger, base, tintAmp, tgen(), albedo, normal, smooth);
            gfx_material& m = s->materials[matSlot];
            m.texA = gfxh_scene_add_texture(s, N, N, GFX_TEX_RGBA8_SRGB, albedo.data());
            m.texSmoothness = gfxh_scene_add_texture(s, N, N, GFX_TEX_R8_UNORM, smooth.data());
            m.texNormal = gfxh_scene_add_texture(s, N, N, GFX_TEX_RGBA8_UNORM, normal.data());
            m.bumpMapType = GFX_BUMP_NORMAL_MAP;
        };
        const float cobble[3] = { 0.62f, 0.58f, 0.52f };
        texture_material(groundMat, 256, 32, 32, 3, true, cobble, 0.5f);
        for (gfx_vertex& v : s->geoms[groundGeom].v) { v.texCoord[0] *= 0.5f * E; v.texCoord[1] *= 0.5f * E; }   // one tile = 4 m
        for (size_t k = 0; k < wallMats.size(); ++k) {
            const gfx_material& wm = s->materials[wallMats[k]];
            // bricks for every other prototype, large plaster panels for the rest; tinted by the prototype's own colour
            const float base[3] = { std::min(1.0f, 0.35f + 1.2f * wm.a[0]), std::min(1.0f, 0.3f + 1.2f * wm.a[1]), std::min(1.0f, 0.28f + 1.2f * wm.a[2]) };
            if (k & 1u) texture_material(wallMats[k], 256, 32, 16, 2, true, base, 0.35f);
            else texture_material(wallMats[k], 128, 64, 64, 1, false, base, 0.12f);
        }
        {
            const float wood[3] = { 0.72f, 0.52f, 0.30f };
            texture_material(crateMat, 128, 128, 16, 1, false, wood, 0.4f);
        }
        for (size_t k = 0; k < signMats.size(); ++k) {   // float emittance map: bright strokes on a dim panel
            const uint32_t W = 64, H = 32;
            gfx_material& m = s->materials[signMats[k]];
            std::vector<float> e(4ull * W * H);
            const uint32_t salt = tgen();
            for (uint32_t y = 0; y < H; ++y)
                for (uint32_t x = 0; x < W; ++x) {
                    const bool border = x < 2 || y < 2 || x >= W - 2 || y >= H - 2;
                    const bool stroke = y > 8 && y < 24 && ((x / 4) % 2 == 0) && hash01(x / 4, y / 8, salt) > 0.25f;
                    const float level = border ? 1.0f : stroke ? 1.6f : 0.25f;
                    float* o = e.data() + 4ull * (static_cast<size_t>(y) * W + x);
                    for (int c = 0; c < 3; ++c) o[c] = level * m.emittance[c];
                    o[3] = 1.0f;
                }
            m.texEmittance = gfxh_scene_add_texture(s, W, H, GFX_TEX_RGBA32F, e.data());
        }
    }
    return 0;
}
