// pt_vertex.hip.h -- one vertex of a path: its surface point (from the G-buffer, or where an extension ray hit), the environment term
// of a miss, next-event estimation and BSDF sampling (shade_vertex), the two rays it asks for (push_vertex).  pt_first_* / pt_next_* put
// them together for the baseline and ReGIR tracers; the NRC tracers (nrc_render.hip.h) call the same routines.
#pragma once
#include "regir.hip.h"

namespace gfx {

struct PtVertexOut {              // what one shaded vertex hands to the queues
    bool wantNee; f3 neeDir; float neeTmax; f3 pending;
    bool wantExt; f3 extDir;
    f3 neeRet;                    // unshadowed NEE estimate (NRC: initial training target)
    f3 localThroughput;           // BSDF sampling throughput of this vertex
    uint32_t trainIdx;            // NRC: training record tied to the NEE ray
    bool neeFromOrg; f3 neeOrg;   // the NEE ray starts at neeOrg instead of the vertex (ReSTIR-driven first vertex: the G-buffer's shading point)
};

// What the ReSTIR DI passes of the frame left for pixel p (GFX_PT_PATH_TRACE_NRC_RESTIR): the direct term of the shading pass,
// recPDFEstimate x unshadowed performDirectLighting of the final reservoir sample at the G-buffer's shading point (restir.hip
// k_shade_prepare; optix_restir_di_kernels.cu:574-606), and the shadow ray that decides it.
struct ReservoirNee { f3 ret; f3 org; LightSample ls; };
GFX_DEV ReservoirNee restir_reservoir_nee(const PtArgs& a, uint32_t bufIdx, size_t p) {
    ReservoirNee r;
    r.ret = f3(0.0f); r.org = f3(0.0f);
    r.ls.emittance = f3(0.0f); r.ls.position = f3(0.0f); r.ls.normal = f3(0.0f); r.ls.atInfinity = 0;
    const size_t numPixels = static_cast<size_t>(a.s.imageSizeX) * a.s.imageSizeY;
    const Camera cam = load_camera(a.f.camera);
    ShadingPoint sp;
    make_shading_point(a, bufIdx, p, cam.pos, true, sp);
    const Reservoir reservoir = load_reservoir(a.s.reservoirBuffer[a.curRes], numPixels, p);
    const float recPDF = static_cast<const float2*>(a.s.reservoirInfoBuffer[a.curRes])[p].x;
    r.org = sp.pos; r.ls = reservoir.sample;
    if (recPDF > 0 && is_finite(recPDF)) r.ret = recPDF * direct_lighting(sp.pos, sp.vOutLocal, sp.frame, sp.bsdf, reservoir.sample);
    return r;
}

// performNextEventEstimation (optix_pathtracing_kernels.cu:18-72) without the trace: returns the
// unshadowed estimate and the shadow ray; + BSDF sampling of the next direction (:140-147, :283-295)
// and the head of the path extension loop.  Every lane of the wave must call it (`active` = lanes
// that shade a vertex) because the ReGIR variant merges its cell-access atomics across the wave.
// REGIR: NEE from the grid cell (sampleFromCell); REGIR_LOOP: Russian roulette at the loop head as pathTraceReGIR does
// (the NRC tracer with ReGIR NEE keeps its own Russian roulette: REGIR = true, REGIR_LOOP = false).
// `given`: the vertex's next-event estimation is already made (the ReSTIR-driven first vertex of the NRC tracer): no light is
// sampled and no random number drawn for it here.
template <bool REGIR, bool REGIR_LOOP = REGIR>
GFX_DEV void shade_vertex(const PtArgs& a, bool active, const EnvMap& env, bool envEnabled, f3 pos, f3 vOutLocal, const Frame& frame,
                          const Bsdf& bsdf, Pcg32& rng, f3& alpha, f3& contribution, float& dirPDensity, PtVertexOut& o,
                          const ReservoirNee* given = nullptr, int nextMaxLengthTerminate = -1 /* -1: a.nextMaxLengthTerminate */) {
    f3 ret(0.0f);
    LightSample ls;
    ls.emittance = f3(0.0f); ls.position = f3(0.0f); ls.normal = f3(0.0f); ls.atInfinity = 0;
    if (given) {
        if (!active) return;
        ret = given->ret; ls = given->ls;
    }
    else if (REGIR) {
        float recPDF;
        const f3 unshadowed = regir_sample_from_cell(a, active, pos, vOutLocal, frame, bsdf, rng, ls, recPDF);
        if (!active) return;
        if (recPDF > 0.0f) ret = unshadowed * (1.0f * recPDF);     // visibility * recProbDensityEstimate (:100)
    }
    else {
        if (!active) return;
        float ul = rng.uniform();
        bool selectEnv = false;
        float probCurType = 1.0f;
        if (envEnabled) {
            if (*a.scene.lightInstIntegral > 0.0f) {
                if (ul < 0.25f) { probCurType = 0.25f; ul = ul / probCurType; selectEnv = true; }
                else { probCurType = 1.0f - 0.25f; ul = (ul - 0.25f) / probCurType; }
            }
            else selectEnv = true;
        }
        float areaPDensity;
        const float u0 = rng.uniform();
        const float u1 = rng.uniform();
        if (a.f.useSolidAngleSampling) sample_light_solid_angle(a.scene, env, a.f.envLightRotation, a.f.envLightPowerCoeff, pos, ul, selectEnv, u0, u1, ls, areaPDensity);
        else sample_light(a.scene, env, a.f.envLightRotation, a.f.envLightPowerCoeff, ul, selectEnv, u0, u1, ls, areaPDensity);
        areaPDensity *= probCurType;
        const ShadowRay sr = shadow_ray(pos, ls);
        float misWeight;
        {
            const f3 vInLocal = frame.to_local(sr.dir);
            const float lpCos = fabsf(dot(sr.dir, ls.normal));
            float bsdfPDensity = bsdf.evaluate_pdf(vOutLocal, vInLocal) * lpCos / sr.dist2;
            if (!is_finite(bsdfPDensity)) bsdfPDensity = 0.0f;
            misWeight = (areaPDensity * areaPDensity) / (bsdfPDensity * bsdfPDensity + areaPDensity * areaPDensity);
        }
        if (areaPDensity > 0.0f) ret = direct_lighting(pos, vOutLocal, frame, bsdf, ls) * (misWeight / areaPDensity);
    }
    const ShadowRay sr = shadow_ray(given ? given->org : pos, ls);
    if (given) { o.neeFromOrg = true; o.neeOrg = given->org; }
    o.wantNee = ret.x != 0.0f || ret.y != 0.0f || ret.z != 0.0f;
    o.neeDir = sr.dir; o.neeTmax = sr.tmax;
    o.pending = alpha * ret;
    o.neeRet = ret;
    if (!o.wantNee) contribution = contribution + o.pending;   // nothing to trace: the add happens here

    f3 vInLocal;
    const float b0 = rng.uniform();
    const float b1 = rng.uniform();
    o.localThroughput = bsdf.sample_throughput(vOutLocal, b0, b1, vInLocal, dirPDensity);
    alpha = alpha * o.localThroughput;
    o.extDir = frame.from_local(vInLocal);
    // loop head of the ray-generation program (:163-166): only valid samples are extended
    o.wantExt = dirPDensity > 0.0f && is_finite(dirPDensity);
    if (REGIR_LOOP && o.wantExt) {   // regir/gpu_kernels/optix_pathtracing_kernels.cu:247-256
        if (nextMaxLengthTerminate < 0 ? a.nextMaxLengthTerminate != 0u : nextMaxLengthTerminate != 0) o.wantExt = false;
        else {
            const float continueProb = fminf(luminance_srgb(alpha) / luminance_srgb(f3(1.0f)), 1.0f);
            if (rng.uniform() >= continueProb) o.wantExt = false;
            else alpha = alpha / continueProb;
        }
    }
}

GFX_DEV void push_vertex(const PtArgs& a, uint32_t pixel, f3 pos, const PtVertexOut& o) {
    // the vertex's NEE (any-hit) ray and extension (closest-hit) ray: both queue heads in one block-level step
    const bool want[2] = { o.wantNee, o.wantExt };
    uint32_t* const counters[2] = { a.neeCount, a.extCountOut };
    uint32_t slots[2];
    queue_reserve_each<2>(want, counters, slots);
    const uint32_t ns = slots[0], es = slots[1];
    queue_write(ns, o.neeFromOrg ? o.neeOrg : pos, o.neeDir, 0.0f, o.neeTmax, a.neeOrg, a.neeDir);
    if (o.wantNee) {
        a.neePending[ns] = make_float4(o.pending.x, o.pending.y, o.pending.z, bits2f(pixel));
        if (a.neeTrainIdx) a.neeTrainIdx[ns] = o.trainIdx;
    }
    queue_write(es, pos, o.extDir, 0.0f, 3.402823466e+38f, a.extOrgOut, a.extDirOut);
    if (o.wantExt) a.extOwnerOut[es] = pixel;
}

// One path in registers between two vertices: throughput, radiance so far, the density its last direction was sampled with, the
// pixel's RNG, the vertex position and what the vertex asked for (its NEE ray and its extension ray).
struct PtPath {
    f3 alpha, contribution; float dirPDensity;
    Pcg32 rng;
    f3 pos;
    PtVertexOut o;
};
GFX_DEV void reset_vertex_out(PtVertexOut& o) {
    o.wantNee = false; o.wantExt = false; o.neeDir = f3(0.0f); o.extDir = f3(0.0f); o.neeTmax = 0; o.pending = f3(0.0f);
    o.neeRet = f3(0.0f); o.localThroughput = f3(0.0f); o.trainIdx = 0x007FFFFFu; o.neeFromOrg = false; o.neeOrg = f3(0.0f);
}
// A vertex ready to be shaded: what pt_first_setup / pt_next_setup leave for shade_vertex (the path's own state lives in PtPath).
struct PtSetup {
    f3 vOutLocal; Frame frame; Bsdf bsdf; bool shade;
    GFX_DEV PtSetup() : vOutLocal(0.0f), frame(f3(0, 0, 1), f3(1, 0, 0)), shade(false) {}
};

// A surface point before the view direction is known: position (not yet offset along ng), geometric and shading normal, tangent,
// texture coordinate and material.  pt_hit_surface adds the hypothetical light density of the point.
struct PtSurface {
    f3 pos, ng, tc0, ns;
    float bcA, bcB, bcC, uA, vA, uB, vB, uC, vC;      // the texture coordinate is interpolated where the caller asks for it
    uint32_t materialSlot;
    float hypAreaPDensity;
    GFX_DEV float tu() const { return bcA * uA + bcB * uB + bcC * uC; }
    GFX_DEV float tv() const { return bcA * vA + bcB * vB + bcC * vC; }
};

// The surface point of a pixel from its G-buffer 0 word g0 (instance, geometry, primitive, barycentrics) -- computeSurfacePoint,
// path_tracing_shared.h:582-621: the tangent is orthogonalised against ns, a non-finite ns falls back to the z axis, a non-finite
// tangent to any one perpendicular to ns.  The ONE copy: pt_first_setup, k_nrc_pt_first and k_nrc_visualize call it.
GFX_DEV PtSurface pt_gbuffer_surface(const PtArgs& a, const uint4& g0) {
    PtSurface sp;
    const float bcB = decode_bc(g0.w & 0xFFFF), bcC = decode_bc(g0.w >> 16);
    const DevInstance* inst = a.scene.insts + g0.x;
    const DevGeomInst g = a.scene.geomInsts[g0.y];
    const uint32_t* tri = a.scene.triangles + 3ull * (g.triangleOffset + g0.z);
    const DevVertex vA = load_vertex(a.scene.vertices + g.vertexOffset + tri[0]);
    const DevVertex vB = load_vertex(a.scene.vertices + g.vertexOffset + tri[1]);
    const DevVertex vC = load_vertex(a.scene.vertices + g.vertexOffset + tri[2]);
    const float bcA = 1 - (bcB + bcC);
    const f3 pAo(vA.px, vA.py, vA.pz), pBo(vB.px, vB.py, vB.pz), pCo(vC.px, vC.py, vC.pz);
    const m34 xfm = load_m34(inst->transform);
    const m33 nrm = load_m33_rows(inst->normalMatrix);
    sp.pos = xfm_point(xfm, bcA * pAo + bcB * pBo + bcC * pCo);
    f3 ng = unit(mul(nrm, cross(pBo - pAo, pCo - pAo)));
    const f3 nsObj = bcA * f3(vA.nx, vA.ny, vA.nz) + bcB * f3(vB.nx, vB.ny, vB.nz) + bcC * f3(vC.nx, vC.ny, vC.nz);
    const f3 tcObj = bcA * f3(vA.tx, vA.ty, vA.tz) + bcB * f3(vB.tx, vB.ty, vB.tz) + bcC * f3(vC.tx, vC.ty, vC.tz);
    f3 ns = unit(mul(nrm, nsObj));
    f3 tc0 = xfm_vector(xfm, tcObj);
    tc0 = unit(tc0 - dot(ns, tc0) * ns);
    if (!all_finite(ns)) { ng = f3(0, 0, 1); ns = f3(0, 0, 1); tc0 = f3(1, 0, 0); }
    if (!all_finite(tc0)) { f3 bt; make_coordinate_system(ns, tc0, bt); }
    sp.ng = ng; sp.ns = ns; sp.tc0 = tc0;
    sp.bcA = bcA; sp.bcB = bcB; sp.bcC = bcC; sp.uA = vA.u; sp.vA = vA.v; sp.uB = vB.u; sp.vB = vB.v; sp.uC = vC.u; sp.vC = vC.v;
    sp.materialSlot = g.materialSlot;
    sp.hypAreaPDensity = 0.0f;
    return sp;
}

// pt_first_vertex up to the shading of the vertex (shade_vertex): the surface point of the pixel from the G-buffer, emission, BSDF.
template <bool REGIR>
GFX_DEV bool pt_first_setup(const PtArgs& a, const PixelId& px, PtPath& path, PtSetup& su) {
    const size_t p = px.p;
    const uint32_t bufIdx = a.f.bufferIndex;
    PtVertexOut& o = path.o;
    reset_vertex_out(o);
    f3& pos = path.pos;
    pos = f3(0.0f);
    f3& vOutLocal = su.vOutLocal;
    vOutLocal = f3(0.0f);
    Frame& frame = su.frame;
    frame = Frame(f3(0, 0, 1), f3(1, 0, 0));
    Bsdf& bsdf = su.bsdf;
    Pcg32& rng = path.rng; rng.state = 0;
    const EnvMap env = load_env(a.s);
    const bool envEnabled = env.present() && a.f.enableEnvLight;
    f3& contribution = path.contribution;
    f3& alpha = path.alpha;
    float& dirPDensity = path.dirPDensity;
    contribution = f3(0.001f, 0.001f, 0.001f);
    alpha = f3(1.0f);
    dirPDensity = 0.0f;
    bool surface = false;
    uint4 g0 = make_uint4(0xFFFFFFFFu, 0, 0, 0);
    if (px.valid) g0 = static_cast<const uint4*>(a.s.gbuffer0[bufIdx])[p];
    surface = g0.x != 0xFFFFFFFFu;
    if (surface) {
        const PtSurface sp = pt_gbuffer_surface(a, g0);
        const Camera cam = load_camera(a.f.camera);
        rng.state = static_cast<const uint64_t*>(a.s.rngBuffer)[p];
        const gfx_material& mat = a.scene.materials[sp.materialSlot];
        const f3 vOut = unit(cam.pos - sp.pos);
        const float frontHit = dot(vOut, sp.ng) >= 0.0f ? 1.0f : -1.0f;
        pos = offset_ray_origin(sp.pos, frontHit * sp.ng);
        const float tu = sp.tu(), tv = sp.tv();
        frame = Frame(sp.ns, sp.tc0);
        if (a.f.enableBumpMapping) apply_bump_mapping(read_modified_normal(a.scene, mat, tu, tv), frame);
        vOutLocal = frame.to_local(vOut);
        contribution = f3(0.0f);
        if (vOutLocal.z > 0 && mat.hasEmittance)
            contribution = contribution + alpha * material_emittance(a.scene, mat, tu, tv) / kPi;
        bsdf.setup(a.scene, mat, tu, tv);
    }
    else if (px.valid && envEnabled) {
        contribution = a.f.envLightPowerCoeff * env.fetch(decode_bc(g0.w & 0xFFFF), decode_bc(g0.w >> 16));
    }
    su.shade = surface;
    return surface;
}
// pathTrace_rayGen_generic up to the path extension loop (optix_pathtracing_kernels.cu:74-160)
// The first vertex from the G-buffer.  Returns whether the pixel shows a surface (its RNG state moved).  EVERY lane must call
// (ReGIR merges its cell-access atomics across the wave).
template <bool REGIR>
GFX_DEV bool pt_first_vertex(const PtArgs& a, const PixelId& px, PtPath& path) {
    PtSetup su;
    const bool surface = pt_first_setup<REGIR>(a, px, path, su);
    const EnvMap env = load_env(a.s);
    const bool envEnabled = env.present() && a.f.enableEnvLight;
    shade_vertex<REGIR>(a, su.shade, env, envEnabled, path.pos, su.vOutLocal, su.frame, su.bsdf, path.rng, path.alpha, path.contribution, path.dirPDensity, path.o);
    return surface;
}

// The surface point an extension ray hit (h: a hit of the BVH8) -- computeSurfacePoint<true, false>, path_tracing_shared.h:485-580:
// world-space vertices, ng from their cross product (its length is twice the area), the tangent NOT orthogonalised, and the density
// with which light sampling would have produced this point, per area or -- useSolidAngleSampling -- per solid angle seen from the
// ray origin.  REGIR: pathTraceReGIR reads that density uninitialised in the reference (undefined); this build defines it as 0
// there.  The ONE copy: pt_next_setup and k_nrc_pt_bounce call it.
template <bool REGIR>
GFX_DEV void pt_hit_surface(const PtArgs& a, const gfx_hit& h, f3 rayOrg, bool envEnabled, PtSurface& sp) {
    f3& pos = sp.pos; f3& ng = sp.ng; f3& ns = sp.ns; f3& tc0 = sp.tc0;
    const Bvh8Tri* tr = a.tris + h.triIndex;
    const uint32_t instSlot = tr->instSlot, geomInstSlot = tr->geomInstSlot, primIndex = tr->primIndex;
    const DevInstance* inst = a.scene.insts + instSlot;
    const DevGeomInst g = a.scene.geomInsts[geomInstSlot];
    const uint32_t* tri = a.scene.triangles + 3ull * (g.triangleOffset + primIndex);
    const DevVertex vA = load_vertex(a.scene.vertices + g.vertexOffset + tri[0]);
    const DevVertex vB = load_vertex(a.scene.vertices + g.vertexOffset + tri[1]);
    const DevVertex vC = load_vertex(a.scene.vertices + g.vertexOffset + tri[2]);
    const m34 xfm = load_m34(inst->transform);
    const m33 nrm = load_m33_rows(inst->normalMatrix);
    const f3 pA = xfm_point(xfm, f3(vA.px, vA.py, vA.pz));
    const f3 pB = xfm_point(xfm, f3(vB.px, vB.py, vB.pz));
    const f3 pC = xfm_point(xfm, f3(vC.px, vC.py, vC.pz));
    const float bcB = h.bcB, bcC = h.bcC;
    const float bcA = 1 - (bcB + bcC);
    pos = bcA * pA + bcB * pB + bcC * pC;
    const f3 nsObj = bcA * f3(vA.nx, vA.ny, vA.nz) + bcB * f3(vB.nx, vB.ny, vB.nz) + bcC * f3(vC.nx, vC.ny, vC.nz);
    const f3 tcObj = bcA * f3(vA.tx, vA.ty, vA.tz) + bcB * f3(vB.tx, vB.ty, vB.tz) + bcC * f3(vC.tx, vC.ty, vC.tz);
    ng = cross(pB - pA, pC - pA);
    const float area = 0.5f * len(ng);
    ng = ng / (2 * area);
    ns = unit(mul(nrm, nsObj));
    tc0 = unit(xfm_vector(xfm, tcObj));
    if (!all_finite(ns)) { ns = f3(0, 0, 1); tc0 = f3(1, 0, 0); }
    if (!all_finite(tc0)) { f3 bt; make_coordinate_system(ns, tc0, bt); }
    float hypAreaPDensity = 0.0f;
    if (!REGIR) {
        float lightProb = 1.0f;
        if (envEnabled) lightProb *= (1 - 0.25f);
        const float instImportance = inst->distIntegral;
        lightProb *= (inst->uniformScale * inst->uniformScale * instImportance) / *a.scene.lightInstIntegral;
        lightProb *= g.distIntegral / instImportance;
        if (is_finite(lightProb)) {
            float pmf = 0.0f;
            if (g.distOffset != 0xFFFFFFFFu && g.distIntegral != 0.0f) pmf = a.scene.lightWeights[g.distOffset + primIndex] / g.distIntegral;
            lightProb *= pmf;
            if (a.f.useSolidAngleSampling) {   // path_tracing_shared.h:550-568, reference point = the ray origin
                const SphericalTriangle st = spherical_triangle(pA, pB, pC, rayOrg);
                const float dirPDF = 1.0f / st.sphArea;
                f3 refDir = rayOrg - pos;
                const float dist2ToRef = len2(refDir);
                refDir = refDir / sqrtf(dist2ToRef);
                const float lpCosRef = dot(refDir, ng);
                hypAreaPDensity = (lpCosRef > 0 && is_finite(dirPDF)) ? lightProb * (dirPDF * lpCosRef / dist2ToRef) : 0.0f;
            }
            else hypAreaPDensity = lightProb / area;
        }
    }
    sp.bcA = bcA; sp.bcB = bcB; sp.bcC = bcC; sp.uA = vA.u; sp.vA = vA.v; sp.uB = vB.u; sp.vB = vB.v; sp.uC = vC.u; sp.vC = vC.v;
    sp.materialSlot = g.materialSlot;
    sp.hypAreaPDensity = hypAreaPDensity;
}

// The environment term of a miss: what an extension ray that left the scene sees, and the MIS weight of having found it by BSDF
// sampling (prevDirPDensity) against light sampling, which picks the environment among the light types with probability 0.25 where
// an instance emits and else with probNoEmitter -- the caller's, because the reference's two miss programs differ in it (1 in the
// baseline's, 0.25 in the NRC tracer's).  The callers multiply luminance and weight into their sums in their own order.
GFX_DEV void pt_miss_environment(const PtArgs& a, const EnvMap& env, const f3& rayDir, float prevDirPDensity, float probNoEmitter, f3& luminance, float& misWeight) {
    const f3 rd = unit(rayDir);
    float posPhi, theta;
    to_polar_yup(rd, posPhi, theta);
    float phi = posPhi + a.f.envLightRotation;
    phi = phi - floorf(phi / (2 * kPi)) * 2 * kPi;
    const float tu = phi / (2 * kPi), tv = theta / kPi;
    luminance = a.f.envLightPowerCoeff * env.fetch(tu, tv);
    const float uvPDF = env.evaluate_pdf(tu, tv);
    const float hypAreaPDensity = uvPDF / (2 * kPi * kPi * gm_sin(theta));
    const float lightPDensity = (*a.scene.lightInstIntegral > 0.0f ? 0.25f : probNoEmitter) * hypAreaPDensity;
    misWeight = (prevDirPDensity * prevDirPDensity) / (prevDirPDensity * prevDirPDensity + lightPDensity * lightPDensity);
}

constexpr uint32_t kPtHitSurface = 1u, kPtMissAdded = 2u;
// pt_next_vertex up to the shading of the vertex: what the extension ray found (implicit light / environment with MIS), Russian roulette, the
// surface point and its BSDF when the path goes on (su.shade).
template <bool REGIR>
GFX_DEV uint32_t pt_next_setup(const PtArgs& a, bool active, const gfx_hit& h, f3 rayOrg, f3 rayDir, const uint64_t* rngBuf, PtPath& path, PtSetup& su,
                               int maxLengthTerminate = -1) {
    PtVertexOut& o = path.o;
    reset_vertex_out(o);
    f3& pos = path.pos;
    pos = f3(0.0f);
    f3& vOutLocal = su.vOutLocal;
    vOutLocal = f3(0.0f);
    Frame& frame = su.frame;
    frame = Frame(f3(0, 0, 1), f3(1, 0, 0));
    Bsdf& bsdf = su.bsdf;
    Pcg32& rng = path.rng;
    const EnvMap env = load_env(a.s);
    const bool envEnabled = env.present() && a.f.enableEnvLight;
    f3& alpha = path.alpha;
    f3& contribution = path.contribution;
    float& dirPDensity = path.dirPDensity;
    bool hitSurface = false, shade = false, missAdded = false;
    if (active) {
        const float prevDirPDensity = dirPDensity;
        if (h.triIndex == GFX_INVALID_SLOT) {
            if (envEnabled && !REGIR) {   // the ReGIR ray type has an empty miss program (regir_main.cpp:250)
                // the probability of the environment among the light types: 1 where no instance emits.  (The NRC tracer's miss program
                // uses 0.25 there as well, k_nrc_pt_bounce: the difference is the reference's.)
                f3 luminance;
                float misWeight;
                pt_miss_environment(a, env, rayDir, prevDirPDensity, 1.0f, luminance, misWeight);
                contribution = contribution + alpha * luminance * misWeight;
                missAdded = true;
            }
        }
        else {
            hitSurface = true;
            PtSurface sp;
            pt_hit_surface<REGIR>(a, h, rayOrg, envEnabled, sp);
            const gfx_material& mat = a.scene.materials[sp.materialSlot];
            const f3 vOut = unit(-rayDir);
            const float frontHit = dot(vOut, sp.ng) >= 0.0f ? 1.0f : -1.0f;
            const float tu = sp.tu(), tv = sp.tv();
            frame = Frame(sp.ns, sp.tc0);
            if (a.f.enableBumpMapping) apply_bump_mapping(read_modified_normal(a.scene, mat, tu, tv), frame);
            pos = offset_ray_origin(sp.pos, frontHit * sp.ng);
            vOutLocal = frame.to_local(vOut);
            if (vOutLocal.z > 0 && mat.hasEmittance) {
                const f3 emittance = material_emittance(a.scene, mat, tu, tv);
                const float dist2 = len2(rayOrg - pos);
                const float lightPDensity = sp.hypAreaPDensity * dist2 / vOutLocal.z;
                const float misWeight = (prevDirPDensity * prevDirPDensity) / (prevDirPDensity * prevDirPDensity + lightPDensity * lightPDensity);
                contribution = contribution + alpha * emittance * (misWeight / kPi);
            }
            if (rngBuf) rng.state = *rngBuf;
            // Russian roulette; initImportance = sRGB_calcLuminance(RGB(1))
            const float continueProb = fminf(luminance_srgb(alpha) / luminance_srgb(f3(1.0f)), 1.0f);
            if (!(rng.uniform() >= continueProb || (maxLengthTerminate < 0 ? a.maxLengthTerminate != 0u : maxLengthTerminate != 0))) {
                alpha = alpha / continueProb;
                bsdf.setup(a.scene, mat, tu, tv);
                shade = true;
            }
        }
    }
    su.shade = shade;
    return (hitSurface ? kPtHitSurface : 0u) | (missAdded ? kPtMissAdded : 0u);
}
// closest-hit + miss programs of one path vertex, then the loop head of the ray-generation program
// (optix_pathtracing_kernels.cu:210-296, :306-341, :161-201; ReGIR: regir/.../optix_pathtracing_kernels.cu:302-392)
// What the extension ray of the previous vertex found (h; `active`: the lane holds such a ray, with path.alpha / contribution /
// dirPDensity as that vertex left them): implicit light or environment with its MIS weight, Russian roulette, the next vertex.
// rngBuf: where the pixel's RNG state is read when the ray hit a surface (the wavefront kernels), or null: path.rng holds it.
// Returns kPtHitSurface (the RNG state moved and the whole state changed) | kPtMissAdded (only the contribution changed).
// EVERY lane must call (ReGIR merges its cell-access atomics across the wave).
template <bool REGIR>
GFX_DEV uint32_t pt_next_vertex(const PtArgs& a, bool active, const gfx_hit& h, f3 rayOrg, f3 rayDir, const uint64_t* rngBuf, PtPath& path,
                                int maxLengthTerminate = -1, int nextMaxLengthTerminate = -1 /* -1: the launch's (a.*) */) {
    PtSetup su;
    const uint32_t what = pt_next_setup<REGIR>(a, active, h, rayOrg, rayDir, rngBuf, path, su, maxLengthTerminate);
    const EnvMap env = load_env(a.s);
    const bool envEnabled = env.present() && a.f.enableEnvLight;
    shade_vertex<REGIR>(a, su.shade, env, envEnabled, path.pos, su.vOutLocal, su.frame, su.bsdf, path.rng, path.alpha, path.contribution, path.dirPDensity, path.o, nullptr, nextMaxLengthTerminate);
    return what;
}

} // namespace gfx
