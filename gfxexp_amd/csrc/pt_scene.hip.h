// pt_scene.hip.h -- the path tracers over a scene with a bound displaced-instance set (gfx_scene_bind_displaced).  Part of
// pathtrace.hip's translation unit.
#pragma once
#include "pt_vertex.hip.h"

namespace gfx {

// Sibling kernels of k_pt_first / k_pt_bounce for a scene whose traces are the scene query (tfdm/tfdm_set.hip): a lane on a plain
// pixel / hit runs pt_first_setup / pt_next_setup (pt_vertex.hip.h), a lane on a displaced one takes its surface point from tfdm/displaced_surface.hip.h.  Ray-origin
// offset, front-face test, Russian roulette, NEE and BSDF sampling are the same code; a displaced surface never emits
// (gfx_scene_bind_displaced refuses such a material) and has no bump mapping, as in the reference.
GFX_DEV tfdm::BaseVertex pt_base_vertex(const DevVertex& v) {
    tfdm::BaseVertex b;
    b.texCoord0Dir = tfdm::v3(v.tx, v.ty, v.tz); b.u = v.u; b.v = v.v;
    return b;
}
struct PtBaseTriangle { tfdm::BaseVertex a, b, c; uint32_t materialSlot; };
GFX_DEV PtBaseTriangle pt_base_triangle(const PtArgs& a, uint32_t geomInstSlot, uint32_t primIndex) {
    const DevGeomInst g = a.scene.geomInsts[geomInstSlot];
    const uint32_t* tri = a.scene.triangles + 3ull * (g.triangleOffset + primIndex);
    PtBaseTriangle t;
    t.a = pt_base_vertex(load_vertex(a.scene.vertices + g.vertexOffset + tri[0]));
    t.b = pt_base_vertex(load_vertex(a.scene.vertices + g.vertexOffset + tri[1]));
    t.c = pt_base_vertex(load_vertex(a.scene.vertices + g.vertexOffset + tri[2]));
    t.materialSlot = g.materialSlot;
    return t;
}
// The first vertex on a displaced pixel: position and normals restored from G-buffers 2 / 3 (tfdm/gpu_kernels/
// optix_pathtracing_kernels.cu:119-126), tangent and texture coordinate from the base triangle.
// SHELL (a binding of gfx_scene_bind_displaced_kinds over a set with a shell member): gbuffer0.geomInstSlot
// carries the shell geometry in its upper four bits, so the geometry table is indexed with the masked word, and the material is the
// one the G-buffer pass chose (gbuffer3.matSlot), not the bound geometry's.
template <bool SHELL>
GFX_DEV void pt_first_setup_displaced(const PtArgs& a, const DisplacedArgs& d, size_t p, uint4 g0, PtPath& path, PtSetup& su) {
    const uint32_t bufIdx = a.f.bufferIndex;
    reset_vertex_out(path.o);
    path.alpha = f3(1.0f);
    path.dirPDensity = 0.0f;
    const float bcB = decode_bc(g0.w & 0xFFFF), bcC = decode_bc(g0.w >> 16);
    const PtBaseTriangle t = pt_base_triangle(a, SHELL ? tfdm::geom_word_slot(g0.y) : g0.y, g0.z);
    const float4 g2 = static_cast<const float4*>(a.s.gbuffer2[bufIdx])[p];
    const uint4 g3 = static_cast<const uint4*>(a.s.gbuffer3[bufIdx])[p];
    const tfdm::V3 ngv = tfdm::ds_decode_dir(f2bits(g2.w));
    tfdm::V3 nsv = tfdm::ds_decode_dir(g3.x), tcv;
    float tu, tv;
    tfdm::displaced_frame(d.table[g0.x & ~GFX_GBUFFER_DISPLACED], t.a, t.b, t.c, bcB, bcC, nsv, tcv, tu, tv);
    const f3 ng(ngv.x, ngv.y, ngv.z), ns(nsv.x, nsv.y, nsv.z), tc0(tcv.x, tcv.y, tcv.z);
    f3 pos(g2.x, g2.y, g2.z);
    const Camera cam = load_camera(a.f.camera);
    path.rng.state = static_cast<const uint64_t*>(a.s.rngBuffer)[p];
    const gfx_material& mat = a.scene.materials[SHELL ? g3.w : t.materialSlot];
    const f3 vOut = unit(cam.pos - pos);
    const float frontHit = dot(vOut, ng) >= 0.0f ? 1.0f : -1.0f;
    path.pos = offset_ray_origin(pos, frontHit * ng);
    su.frame = Frame(ns, tc0);
    su.vOutLocal = su.frame.to_local(vOut);
    path.contribution = f3(0.0f);
    su.bsdf.setup(a.scene, mat, tu, tv);
    su.shade = true;
}
// REGIR (a binding that carries GFX_DISPLACED_REGIR): the vertex's NEE comes from its grid cell, on a plain and on
// a displaced pixel alike (the cell of the offset shading position); every lane reaches shade_vertex, as the cell-access count wants.
template <bool SHELL, bool REGIR>
GFX_DEV void pt_first_scene(const PtArgs& a, const DisplacedArgs& d) {
    const PixelId px = pixel_of_thread(a.px);
    const size_t p = px.p;
    PtPath path;
    PtSetup su;
    uint4 g0 = make_uint4(0xFFFFFFFFu, 0, 0, 0);
    if (px.valid) g0 = static_cast<const uint4*>(a.s.gbuffer0[a.f.bufferIndex])[p];
    bool surface;
    if (g0.x != 0xFFFFFFFFu && (g0.x & GFX_GBUFFER_DISPLACED)) { pt_first_setup_displaced<SHELL>(a, d, p, g0, path, su); surface = true; }
    else surface = pt_first_setup<REGIR>(a, px, path, su);
    const EnvMap env = load_env(a.s);
    const bool envEnabled = env.present() && a.f.enableEnvLight;
    shade_vertex<REGIR>(a, su.shade, env, envEnabled, path.pos, su.vOutLocal, su.frame, su.bsdf, path.rng, path.alpha, path.contribution, path.dirPDensity, path.o);
    if (surface) static_cast<uint64_t*>(a.s.rngBuffer)[p] = path.rng.state;
    if (px.valid) {
        a.state[2 * p] = make_float4(path.alpha.x, path.alpha.y, path.alpha.z, path.dirPDensity);
        a.state[2 * p + 1] = make_float4(path.contribution.x, path.contribution.y, path.contribution.z, 0.0f);
    }
    push_vertex(a, static_cast<uint32_t>(p), path.pos, path.o);
}
__global__ __launch_bounds__(kPtBlock) void k_pt_first_scene(PtArgs a, DisplacedArgs d) { pt_first_scene<false, false>(a, d); }
__global__ __launch_bounds__(kPtBlock) void k_pt_first_scene_shell(PtArgs a, DisplacedArgs d) { pt_first_scene<true, false>(a, d); }
__global__ __launch_bounds__(kPtBlock) void k_pt_regir_first_scene(PtArgs a, DisplacedArgs d) { pt_first_scene<false, true>(a, d); }
__global__ __launch_bounds__(kPtBlock) void k_pt_regir_first_scene_shell(PtArgs a, DisplacedArgs d) { pt_first_scene<true, true>(a, d); }
// A later vertex on a displaced surface: everything from the hit (optix_pathtracing_kernels.cu:289-301).
// materialSlot: the material the hit is shaded with, where it is not the bound geometry's (a shell member's, by shell geometry);
// GFX_INVALID_SLOT: the bound geometry's.
GFX_DEV uint32_t pt_next_setup_displaced(const PtArgs& a, const DisplacedArgs& d, const tfdm::SceneHit& sh, f3 rayOrg, f3 rayDir, const uint64_t* rngBuf, PtPath& path,
                                         PtSetup& su, uint32_t materialSlot = GFX_INVALID_SLOT) {
    reset_vertex_out(path.o);
    const uint32_t k = sh.where >> 1;
    const PtBaseTriangle t = pt_base_triangle(a, d.geomSlots[k], sh.index);
    const tfdm::DisplacedPoint sp = tfdm::displaced_point(d.table[k], sh, tfdm::v3(rayOrg.x, rayOrg.y, rayOrg.z), tfdm::v3(rayDir.x, rayDir.y, rayDir.z), t.a, t.b, t.c);
    const f3 ng(sp.normal.x, sp.normal.y, sp.normal.z), tc0(sp.tangent.x, sp.tangent.y, sp.tangent.z);
    const gfx_material& mat = a.scene.materials[materialSlot != GFX_INVALID_SLOT ? materialSlot : t.materialSlot];
    const f3 vOut = unit(-rayDir);
    const float frontHit = dot(vOut, ng) >= 0.0f ? 1.0f : -1.0f;
    su.frame = Frame(ng, tc0);
    path.pos = offset_ray_origin(f3(sp.position.x, sp.position.y, sp.position.z), frontHit * ng);
    su.vOutLocal = su.frame.to_local(vOut);
    if (rngBuf) path.rng.state = *rngBuf;
    // Russian roulette; initImportance = sRGB_calcLuminance(RGB(1))
    const float continueProb = fminf(luminance_srgb(path.alpha) / luminance_srgb(f3(1.0f)), 1.0f);
    su.shade = false;
    if (!(path.rng.uniform() >= continueProb || a.maxLengthTerminate != 0u)) {
        path.alpha = path.alpha / continueProb;
        su.bsdf.setup(a.scene, mat, sp.u, sp.v);
        su.shade = true;
    }
    return kPtHitSurface;
}
// REGIR: a plain hit as pt_next_setup<true> takes it (no environment term at a miss, hypothetical light density 0); a displaced hit adds
// neither, so its branch is the baseline's; the Russian roulette of the ReGIR loop head is shade_vertex<true>'s.
template <bool SHELL, bool REGIR>
GFX_DEV void pt_bounce_scene(const PtArgs& a, const DisplacedArgs& d, const DisplacedShellArgs& e) {
    const uint32_t i = blockIdx.x * kPtBlock + threadIdx.x;
    const uint32_t count = *a.extCountIn;
    PtPath path;
    path.alpha = f3(0.0f); path.contribution = f3(0.0f); path.dirPDensity = 0.0f; path.rng.state = 0;
    uint32_t pixel = 0;
    gfx_hit h; h.dist = 0.0f; h.bcB = 0.0f; h.bcC = 0.0f; h.triIndex = GFX_INVALID_SLOT;
    tfdm::SceneHit sh = tfdm::scene_miss(0.0f);
    uint32_t shellGeom = 0u;
    f3 rayOrg(0.0f), rayDir(0.0f);
    const bool active = i < count;
    if (active) {
        pixel = a.extOwnerIn[i];
        const float4 h0 = d.hits[2ull * i], h1 = d.hits[2ull * i + 1];          // a gfx_scene_hit: two 16-byte loads
        sh.dist = h0.x; sh.bcB = h0.y; sh.bcC = h0.z; sh.index = f2bits(h0.w); sh.normal = tfdm::v3(h1.x, h1.y, h1.z); sh.where = f2bits(h1.w);
        if (SHELL) shellGeom = f2bits(e.shellPart[i].y);                           // a gfx_scene_shell_part: one more 16-byte load
        h.dist = h0.x; h.bcB = h0.y; h.bcC = h0.z; h.triIndex = sh.index;        // a miss carries GFX_INVALID_SLOT there
        const float4 ro4 = a.extOrgIn[i], rd4 = a.extDirIn[i];
        rayOrg = f3(ro4.x, ro4.y, ro4.z); rayDir = f3(rd4.x, rd4.y, rd4.z);
        const float4 s0 = a.state[2ull * pixel], s1 = a.state[2ull * pixel + 1];
        path.alpha = f3(s0.x, s0.y, s0.z);
        path.dirPDensity = s0.w;
        path.contribution = f3(s1.x, s1.y, s1.z);
    }
    const uint64_t* rngBuf = static_cast<const uint64_t*>(a.s.rngBuffer) + pixel;
    PtSetup su;
    uint32_t what;
    if (active && sh.where != GFX_INVALID_SLOT && sh.where != GFX_SCENE_PLAIN) {
        if (SHELL) {
            // the material of a shell member's hit is its shell geometry's; of another member's, its bound geometry's (the sentinel)
            const uint32_t k = sh.where >> 1;
            const uint32_t mat = tfdm::displaced_material(nrtdsm::instance_kind(d.table[k]), k, shellGeom, e.shellMats, GFX_INVALID_SLOT);
            what = pt_next_setup_displaced(a, d, sh, rayOrg, rayDir, rngBuf, path, su, mat);
        }
        else what = pt_next_setup_displaced(a, d, sh, rayOrg, rayDir, rngBuf, path, su);
    }
    else what = pt_next_setup<REGIR>(a, active, h, rayOrg, rayDir, rngBuf, path, su);
    const EnvMap env = load_env(a.s);
    const bool envEnabled = env.present() && a.f.enableEnvLight;
    shade_vertex<REGIR>(a, su.shade, env, envEnabled, path.pos, su.vOutLocal, su.frame, su.bsdf, path.rng, path.alpha, path.contribution, path.dirPDensity, path.o);
    if (what & kPtHitSurface) {
        static_cast<uint64_t*>(a.s.rngBuffer)[pixel] = path.rng.state;
        a.state[2ull * pixel] = make_float4(path.alpha.x, path.alpha.y, path.alpha.z, path.dirPDensity);
    }
    if (what & (kPtHitSurface | kPtMissAdded)) a.state[2ull * pixel + 1] = make_float4(path.contribution.x, path.contribution.y, path.contribution.z, 0.0f);
    push_vertex(a, pixel, path.pos, path.o);
}
__global__ __launch_bounds__(kPtBlock) void k_pt_bounce_scene(PtArgs a, DisplacedArgs d) {
    DisplacedShellArgs none;
    none.shellPart = nullptr; none.shellMats = nullptr;
    pt_bounce_scene<false, false>(a, d, none);
}
__global__ __launch_bounds__(kPtBlock) void k_pt_bounce_scene_shell(PtArgs a, DisplacedArgs d, DisplacedShellArgs e) { pt_bounce_scene<true, false>(a, d, e); }
__global__ __launch_bounds__(kPtBlock) void k_pt_regir_bounce_scene(PtArgs a, DisplacedArgs d) {
    DisplacedShellArgs none;
    none.shellPart = nullptr; none.shellMats = nullptr;
    pt_bounce_scene<false, true>(a, d, none);
}
__global__ __launch_bounds__(kPtBlock) void k_pt_regir_bounce_scene_shell(PtArgs a, DisplacedArgs d, DisplacedShellArgs e) { pt_bounce_scene<true, true>(a, d, e); }

} // namespace gfx
