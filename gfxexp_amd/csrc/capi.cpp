// capi.cpp -- extern "C" entry points declared in include/gfxexp.h.
// Error model: every HIP failure becomes a non-zero return + gfx_last_error() text (the reference
// throws std::runtime_error from CUDADRV_CHECK, utils/cuda_util.cpp:58-69; a C++ shim above this
// ABI can re-throw).
#include <cstdlib>
#include <cstring>
#include <memory>
#include "internal.h"
#include "denoise/denoise.h"
#include "denoise/taa.h"
#include "bc/bc_decode.hip.h"
#include "bc/bc_textures.h"
#include "host/tex_format.h"
#include "tfdm/tfdm.h"
#include "tfdm/tfdm_set.h"
#include "nrtdsm/nrtdsm.h"
#include "nrtdsm/shell.h"

using namespace gfx;

struct gfx_ctx {
    Context c;
    DevBuf scenePlain;      // gfx_hit[numRays]: the plain phase of a closest-hit gfx_trace_scene without an instance set (tfdm_set.hip)
};
struct gfx_denoiser { Denoiser d; };
struct gfx_taa { TemporalAA t; };
struct gfx_tfdm { TfdmObject o; };
struct gfx_tfdm_set { TfdmSet s; gfx_ctx* ctx; };
struct gfx_nrtdsm { NrtdsmObject o; };
struct gfx_shell { ShellObject o; };

static thread_local std::string g_createError;

// Every entry point runs on the context's device and leaves the calling thread's current device as it found it
// (a process may drive several GPUs: torch, several contexts).
namespace {
struct DeviceGuard {
    int prev = -1; bool switched = false;
    explicit DeviceGuard(int device) {
        GFX_HIP(hipGetDevice(&prev));
        if (prev != device) { GFX_HIP(hipSetDevice(device)); switched = true; }
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};
int env_int(const char* name, int fallback, int lo, int hi) {
    const char* e = getenv(name);
    if (!e || !*e) return fallback;
    const int v = atoi(e);
    return (v < lo || v > hi) ? fallback : v;
}

// ---- the displaced-surface objects (gfx_tfdm, gfx_nrtdsm, gfx_shell; tfdm/displaced_object.h): what their entry points share
gfx_tfdm_params displaced_defaults(const gfx_tfdm_params* given, bool shell) {
    gfx_tfdm_params p;
    if (given) p = *given;
    else { tfdm_default_params(&p); if (shell) p.localIntersection = 0u; }
    return p;
}
// `init(object)` fills the new object; one that it leaves half made is released
template <typename Handle, typename Init> void displaced_create(gfx_ctx* ctx, const char* who, Handle** out, Init init) {
    if (!out) throw HipError(std::string(who) + ": null output handle");
    *out = nullptr;
    std::unique_ptr<Handle> t(new Handle());
    t->o.device = ctx->c.device;
    try { init(t->o); }
    catch (...) { displaced_release(t->o); throw; }
    *out = t.release();
}
template <typename Handle> int displaced_destroy(Handle* obj) {
    if (!obj) return 1;
    int prev = -1;
    const bool switched = hipGetDevice(&prev) == hipSuccess && prev != obj->o.device && hipSetDevice(obj->o.device) == hipSuccess;
    (void)hipDeviceSynchronize();
    displaced_release(obj->o);
    if (switched) (void)hipSetDevice(prev);
    delete obj;
    return 0;
}
// the guard of a call that launches on the object; `alsoGiven`: the other pointer the call needs, named by `also`
template <typename Handle> void displaced_guard(const gfx_ctx* ctx, const Handle* obj, const char* who, const char* also = "", const void* alsoGiven = "") {
    if (!obj || !alsoGiven) throw HipError(std::string(who) + ": null object" + also);
    if (obj->o.device != ctx->c.device) throw HipError(std::string(who) + ": the object belongs to another device");
}
}
#define GFX_TRY(ctx) if (!(ctx)) return 1; try { DeviceGuard deviceGuard__((ctx)->c.device);
#define GFX_CATCH(ctx) \
    return 0; } \
    catch (const std::exception& e) { (ctx)->c.lastError = e.what(); return 1; } \
    catch (...) { (ctx)->c.lastError = "unknown error"; return 1; }

extern "C" {

const char* gfx_version(void) { return "gfxexp_amd 0.1 gfx950"; }

int gfx_ctx_create(int device, gfx_ctx** out) {
    *out = nullptr;
    try {
        int count = 0;
        GFX_HIP(hipGetDeviceCount(&count));
        if (device < 0 || device >= count) throw HipError("gfx_ctx_create: no such HIP device");
        GFX_HIP(hipSetDevice(device));
        std::unique_ptr<gfx_ctx> ctx(new gfx_ctx());
        ctx->c.device = device;
        hipDeviceProp_t prop;
        GFX_HIP(hipGetDeviceProperties(&prop, device));
        ctx->c.numCUs = prop.multiProcessorCount;
        Tunables& t = ctx->c.tune;
        t.pixelMap = env_int("GFX_PIXEL_MAP", t.pixelMap, 0, 2);
        t.superShiftX = env_int("GFX_SUPER_X", t.superShiftX, 0, 6);
        t.superShiftY = env_int("GFX_SUPER_Y", t.superShiftY, 0, 6);
        t.traceBlocksPerCU = env_int("GFX_TRACE_BLOCKS_PER_CU", t.traceBlocksPerCU, 1, 8);
        t.traceRefill = env_int("GFX_TRACE_REFILL", t.traceRefill, 1, 64);
        t.traceBatch = env_int("GFX_TRACE_BATCH", t.traceBatch, 1, 65536);
        t.temporalHints = env_int("GFX_TEMPORAL_HINTS", t.temporalHints, 0, 1);
        t.ptOverlap = env_int("GFX_PT_OVERLAP", t.ptOverlap, 0, 1);
        t.ptRegen = env_int("GFX_PT_REGEN", t.ptRegen, 0, 8);
        t.ptRegenMin = env_int("GFX_PT_REGEN_MIN", t.ptRegenMin, 1, 64);
        t.candidateSplit = env_int("GFX_CANDIDATE_SPLIT", t.candidateSplit, 0, 4);
        t.fusePasses = env_int("GFX_FUSE_PASSES", t.fusePasses, 0, 2);
        t.blockOrder = env_int("GFX_BLOCK_ORDER", t.blockOrder, 0, 1);
        t.nrcStagedInfer = env_int("GFX_NRC_STAGED_INFER", t.nrcStagedInfer, 0, 3);
        if (t.candidateSplit == 3) t.candidateSplit = 2;
        ctx->c.dTraceCounters.reserve(64);
        GFX_HIP(hipMemset(ctx->c.dTraceCounters.p, 0, 64));
        *out = ctx.release();
        return 0;
    }
    catch (const std::exception& e) { g_createError = e.what(); return 1; }
}

void gfx_ctx_destroy(gfx_ctx* ctx) {
    if (!ctx) return;
    (void)hipDeviceSynchronize();
    bc_textures_drop(ctx->c);
    ctx->scenePlain.release();
    delete ctx;
}

const char* gfx_last_error(gfx_ctx* ctx) { return ctx ? ctx->c.lastError.c_str() : g_createError.c_str(); }

int gfx_material_set(gfx_ctx* ctx, uint32_t matSlot, const gfx_material* mat) {
    GFX_TRY(ctx)
    if (!mat) throw HipError("gfx_material_set: null material");
    if (matSlot >= (1u << 24)) throw HipError("gfx_material_set: material slot out of range");   // also keeps matSlot + 1 from wrapping
    if (ctx->c.materials.size() <= matSlot) {
        gfx_material zero; std::memset(&zero, 0, sizeof(zero));
        ctx->c.materials.resize(matSlot + 1, zero);
    }
    ctx->c.materials[matSlot] = *mat;
    ctx->c.sceneDirty = true;
    GFX_CATCH(ctx)
}

int gfx_texture_set(gfx_ctx* ctx, uint32_t texSlot, uint32_t width, uint32_t height, uint32_t format, const void* texels) {
    GFX_TRY(ctx)
    if (texSlot == 0 || texSlot > (1u << 20)) throw HipError("gfx_texture_set: texture slots are 1-based");
    if (width == 0 || height == 0 || width > 16384 || height > 16384) throw HipError("gfx_texture_set: bad size");   // TexDimInfo: 14 bits
    const size_t bpp = tex_bytes_per_texel(format);
    if (!bpp) throw HipError("gfx_texture_set: unknown format");
    if (!texels) throw HipError("gfx_texture_set: null texels");
    if (ctx->c.textures.size() <= texSlot) ctx->c.textures.resize(texSlot + 1);
    HostTexture& t = ctx->c.textures[texSlot];
    t.width = width; t.height = height; t.format = format;
    t.texels.assign(static_cast<const uint8_t*>(texels), static_cast<const uint8_t*>(texels) + bpp * width * height);
    bc_texture_forget(ctx->c, texSlot);
    ctx->c.sceneDirty = true;
    GFX_CATCH(ctx)
}

int gfx_texture_set_bc(gfx_ctx* ctx, uint32_t texSlot, uint32_t width, uint32_t height, uint32_t bcFormat, const void* blocks, uint32_t format) {
    GFX_TRY(ctx)
    if (texSlot == 0 || texSlot > (1u << 20)) throw HipError("gfx_texture_set_bc: texture slots are 1-based");
    if (width == 0 || height == 0 || width > 16384 || height > 16384) throw HipError("gfx_texture_set_bc: bad size");
    const uint32_t blockBytes = bc::block_bytes(bcFormat);
    if (blockBytes == 0) throw HipError("gfx_texture_set_bc: unknown block-compressed format");
    if (format == GFX_TEX_RGBA32F) throw HipError("gfx_texture_set_bc: blocks expand into an 8-bit format, not GFX_TEX_RGBA32F");
    if (format != GFX_TEX_RGBA8_SRGB && format != GFX_TEX_RGBA8_UNORM && format != GFX_TEX_R8_UNORM && format != GFX_TEX_RG8_UNORM)
        throw HipError("gfx_texture_set_bc: unknown format");
    if (!blocks) throw HipError("gfx_texture_set_bc: null blocks");
    // the blocks reach the device before the slot changes: a failure here leaves the slot as it was
    bc_texture_store(ctx->c, texSlot, bcFormat, blocks, static_cast<size_t>((width + 3) / 4) * ((height + 3) / 4) * blockBytes);
    if (ctx->c.textures.size() <= texSlot) ctx->c.textures.resize(texSlot + 1);
    HostTexture& t = ctx->c.textures[texSlot];
    t.width = width; t.height = height; t.format = format;
    std::vector<uint8_t>().swap(t.texels);      // no texels on the host: scene_upload reserves the region and expands into it
    ctx->c.sceneDirty = true;
    GFX_CATCH(ctx)
}

int gfx_texture_read(gfx_ctx* ctx, void* stream, uint32_t texSlot, void* hostOut, size_t bytes) {
    GFX_TRY(ctx)
    Context& c = ctx->c;
    if (texSlot == 0 || texSlot >= c.textures.size() || c.textures[texSlot].width == 0) throw HipError("gfx_texture_read: texture slot was never set");
    const HostTexture& t = c.textures[texSlot];
    if (!hostOut || bytes != tex_bytes_per_texel(t.format) * t.width * t.height) throw HipError("gfx_texture_read: the buffer must hold the slot's texels exactly");
    hipStream_t s = static_cast<hipStream_t>(stream);
    scene_upload(c, s);
    DevTexture d;
    GFX_HIP(hipMemcpyAsync(&d, c.dTextures.as<DevTexture>() + texSlot, sizeof(d), hipMemcpyDeviceToHost, s));
    GFX_HIP(hipStreamSynchronize(s));
    if (d.width != t.width || d.height != t.height || d.format != t.format) throw HipError("gfx_texture_read: the device descriptor does not match the slot");
    GFX_HIP(hipMemcpyAsync(hostOut, c.dTexelPool.as<uint32_t>() + d.offset, bytes, hipMemcpyDeviceToHost, s));
    GFX_HIP(hipStreamSynchronize(s));
    GFX_CATCH(ctx)
}

int gfx_texture_sample(gfx_ctx* ctx, void* stream, uint32_t texSlot, const void* dUv, uint32_t n, void* dOut, int gather) {
    GFX_TRY(ctx)
    texture_sample(ctx->c, static_cast<hipStream_t>(stream), texSlot, dUv, n, dOut, gather);
    GFX_CATCH(ctx)
}

int gfx_geom_create(gfx_ctx* ctx, const void* vertices, uint32_t vertexStride, uint32_t numVertices,
                    const uint32_t* triangles, uint32_t numTriangles, uint32_t matSlot, uint32_t* geomInstSlot) {
    GFX_TRY(ctx)
    if (vertexStride < sizeof(gfx_vertex)) throw HipError("gfx_geom_create: vertexStride smaller than gfx_vertex");
    HostGeom g;
    g.vertices.resize(numVertices);
    for (uint32_t i = 0; i < numVertices; ++i) {
        gfx_vertex v;
        std::memcpy(&v, static_cast<const uint8_t*>(vertices) + static_cast<size_t>(vertexStride) * i, sizeof(v));
        DevVertex& d = g.vertices[i];
        d.px = v.position[0]; d.py = v.position[1]; d.pz = v.position[2];
        d.nx = v.normal[0]; d.ny = v.normal[1]; d.nz = v.normal[2];
        d.tx = v.texCoord0Dir[0]; d.ty = v.texCoord0Dir[1]; d.tz = v.texCoord0Dir[2];
        d.u = v.texCoord[0]; d.v = v.texCoord[1]; d.pad = 0;
    }
    g.triangles.assign(triangles, triangles + 3ull * numTriangles);
    for (uint32_t idx : g.triangles) if (idx >= numVertices) throw HipError("gfx_geom_create: triangle index out of range");
    g.materialSlot = matSlot;
    *geomInstSlot = static_cast<uint32_t>(ctx->c.geoms.size());
    ctx->c.geoms.push_back(std::move(g));
    ctx->c.sceneDirty = true;
    GFX_CATCH(ctx)
}

int gfx_group_create(gfx_ctx* ctx, const uint32_t* geomInstSlots, uint32_t n, uint32_t* group) {
    GFX_TRY(ctx)
    for (uint32_t i = 0; i < n; ++i) if (geomInstSlots[i] >= ctx->c.geoms.size()) throw HipError("gfx_group_create: unknown geomInstSlot");
    *group = static_cast<uint32_t>(ctx->c.groups.size());
    ctx->c.groups.emplace_back(geomInstSlots, geomInstSlots + n);
    ctx->c.sceneDirty = true;
    GFX_CATCH(ctx)
}

int gfx_instance_create(gfx_ctx* ctx, uint32_t group, const float xfm[12], uint32_t* instSlot) {
    GFX_TRY(ctx)
    if (group >= ctx->c.groups.size()) throw HipError("gfx_instance_create: unknown group");
    HostInstance inst;
    inst.group = group;
    std::memcpy(inst.transform, xfm, sizeof(float) * 12);
    std::memcpy(inst.prevTransform, xfm, sizeof(float) * 12);
    *instSlot = static_cast<uint32_t>(ctx->c.insts.size());
    ctx->c.insts.push_back(inst);
    ctx->c.sceneDirty = true;
    GFX_CATCH(ctx)
}

static void instance_update(gfx_ctx* ctx, uint32_t instSlot, const float xfm[12], const float* normalMatrix) {
    if (instSlot >= ctx->c.insts.size()) throw HipError("gfx_instance_set_transform: unknown instSlot");
    HostInstance& inst = ctx->c.insts[instSlot];
    std::memcpy(inst.prevTransform, inst.transform, sizeof(float) * 12);
    std::memcpy(inst.transform, xfm, sizeof(float) * 12);
    instance_cur_to_prev(inst.prevTransform, inst.transform, inst.curToPrev);
    inst.animated = true;
    inst.hasNormalMatrix = normalMatrix != nullptr;
    if (normalMatrix) std::memcpy(inst.normalMatrix, normalMatrix, sizeof(float) * 9);
    if (inst.dynamic && !ctx->c.sceneDirty) {       // already in the animated subtree: transform-only update
        ctx->c.transformsDirty = true;
        ctx->c.movedInsts.push_back(instSlot);
    }
    else {                                          // first move: the instance changes subtree, full rebuild once
        inst.dynamic = true;
        ctx->c.sceneDirty = true;
    }
}

int gfx_instance_set_dynamic(gfx_ctx* ctx, uint32_t instSlot, int dynamic) {
    GFX_TRY(ctx)
    if (instSlot >= ctx->c.insts.size()) throw HipError("gfx_instance_set_dynamic: unknown instSlot");
    if (ctx->c.insts[instSlot].dynamic != (dynamic != 0)) {
        ctx->c.insts[instSlot].dynamic = dynamic != 0;
        ctx->c.sceneDirty = true;
    }
    GFX_CATCH(ctx)
}

int gfx_instance_set_transform(gfx_ctx* ctx, uint32_t instSlot, const float xfm[12]) {
    GFX_TRY(ctx)
    instance_update(ctx, instSlot, xfm, nullptr);
    GFX_CATCH(ctx)
}

int gfx_instance_set_transform_and_normal_matrix(gfx_ctx* ctx, uint32_t instSlot, const float xfm[12], const float normalMatrix[9]) {
    GFX_TRY(ctx)
    instance_update(ctx, instSlot, xfm, normalMatrix);
    GFX_CATCH(ctx)
}

int gfx_accel_build(gfx_ctx* ctx, void* stream, uint64_t* handle) {
    GFX_TRY(ctx)
    Accel* a = nullptr;
    if (*handle != 0 && *handle <= ctx->c.accels.size() && ctx->c.accels[*handle - 1]) a = ctx->c.accels[*handle - 1]; // rebuild in place
    else { a = new Accel(); ctx->c.accels.push_back(a); *handle = ctx->c.accels.size(); }
    if (!lbvh_update_dynamic(ctx->c, static_cast<hipStream_t>(stream), *a)) lbvh_build(ctx->c, static_cast<hipStream_t>(stream), *a);
    GFX_CATCH(ctx)
}

static Accel* find_accel(gfx_ctx* ctx, uint64_t handle) {
    if (handle == 0 || handle > ctx->c.accels.size() || !ctx->c.accels[handle - 1]) throw HipError("invalid accel handle");
    return ctx->c.accels[handle - 1];
}

int gfx_accel_stats(gfx_ctx* ctx, uint64_t handle, uint32_t stats[4]) {
    GFX_TRY(ctx)
    const Accel* a = find_accel(ctx, handle);
    stats[0] = a->numInputTris; stats[1] = a->numNodes; stats[2] = a->numTris; stats[3] = a->maxDepth;
    GFX_CATCH(ctx)
}

int gfx_accel_tri_ids(gfx_ctx* ctx, uint64_t handle, const void** dTriIds, uint32_t* count) {
    GFX_TRY(ctx)
    const Accel* a = find_accel(ctx, handle);
    *dTriIds = a->triIds.p; *count = a->numTris;
    GFX_CATCH(ctx)
}

int gfx_accel_set_max_leaf(gfx_ctx* ctx, uint32_t maxLeafTris) {
    GFX_TRY(ctx)
    ctx->c.maxLeafTris = maxLeafTris < 1 ? 1 : (maxLeafTris > 4 ? 4 : maxLeafTris);   // 8 children x 4 = one 32-bit triangle mask
    GFX_CATCH(ctx)
}

int gfx_lights_build_static(gfx_ctx* ctx, void* stream) {
    GFX_TRY(ctx)
    lights_build_static(ctx->c, static_cast<hipStream_t>(stream));
    GFX_CATCH(ctx)
}

int gfx_lights_build_instances(gfx_ctx* ctx, void* stream, uint32_t bufferIndex) {
    GFX_TRY(ctx)
    lights_build_instances(ctx->c, static_cast<hipStream_t>(stream), bufferIndex);
    GFX_CATCH(ctx)
}

int gfx_lights_read(gfx_ctx* ctx, uint32_t level, uint32_t index, float* weights, float* cdf,
                    uint32_t capacity, uint32_t* n, float* integral) {
    GFX_TRY(ctx)
    Context& c = ctx->c;
    GFX_HIP(hipDeviceSynchronize());
    uint32_t off = 0xFFFFFFFFu, count = 0;
    float integ = 0.0f;
    if (level == 0) {
        off = c.lightInstDistOffset; count = static_cast<uint32_t>(c.insts.size());
        GFX_HIP(hipMemcpy(&integ, c.dLightInstIntegral.p, sizeof(float), hipMemcpyDeviceToHost));
    }
    else if (level == 1) {
        if (index >= c.hInsts.size()) throw HipError("gfx_lights_read: bad instance index");
        DevInstance d;
        GFX_HIP(hipMemcpy(&d, c.dInsts.as<DevInstance>() + index, sizeof(d), hipMemcpyDeviceToHost));
        off = d.distOffset; count = off == 0xFFFFFFFFu ? 0 : d.numGeomInsts; integ = d.distIntegral;
    }
    else {
        if (index >= c.hGeomInsts.size()) throw HipError("gfx_lights_read: bad geomInst index");
        DevGeomInst d;
        GFX_HIP(hipMemcpy(&d, c.dGeomInsts.as<DevGeomInst>() + index, sizeof(d), hipMemcpyDeviceToHost));
        off = d.distOffset; count = off == 0xFFFFFFFFu ? 0 : d.distCount; integ = d.distIntegral;
    }
    *n = count; *integral = integ;
    const uint32_t m = count < capacity ? count : capacity;
    if (m && weights) GFX_HIP(hipMemcpy(weights, c.dLightW.as<float>() + off, sizeof(float) * m, hipMemcpyDeviceToHost));
    if (m && cdf) GFX_HIP(hipMemcpy(cdf, c.dLightCDF.as<float>() + off, sizeof(float) * m, hipMemcpyDeviceToHost));
    GFX_CATCH(ctx)
}

int gfx_lights_sample(gfx_ctx* ctx, void* stream, int mode, const float shadingPoint[3], const void* dU, uint32_t n, void* dOut) {
    GFX_TRY(ctx)
    lights_sample(ctx->c, static_cast<hipStream_t>(stream), mode, shadingPoint, dU, n, dOut);
    GFX_CATCH(ctx)
}

int gfx_math_eval(gfx_ctx* ctx, void* stream, int fn, const void* dA, const void* dB, uint32_t n, void* dOut) {
    GFX_TRY(ctx)
    math_eval(ctx->c, static_cast<hipStream_t>(stream), fn, dA, dB, n, dOut);
    GFX_CATCH(ctx)
}

int gfx_bsdf_eval(gfx_ctx* ctx, void* stream, int fn, const void* dMat, const void* dA, const void* dB, const void* dC, uint32_t n, void* dOut) {
    GFX_TRY(ctx)
    bsdf_eval(ctx->c, static_cast<hipStream_t>(stream), fn, dMat, dA, dB, dC, n, dOut);
    GFX_CATCH(ctx)
}

uint32_t gfx_bsdf_eval_words(int fn) {
    try { return bsdf_eval_words(fn); } catch (...) { return 0; }
}

int gfx_lights_table_info(gfx_ctx* ctx, uint32_t info[8]) {
    GFX_TRY(ctx)
    Context& c = ctx->c;
    GFX_HIP(hipDeviceSynchronize());
    uint32_t header[4] = { 0, 0, 0, 0 };
    if (c.dSpanHeader.p) GFX_HIP(hipMemcpy(header, c.dSpanHeader.p, sizeof(header), hipMemcpyDeviceToHost));
    info[0] = header[0]; info[1] = header[1]; info[2] = c.numEmitterRecs; info[3] = c.spanGuideCells;
    info[4] = c.numLightMatrices; info[5] = 0; info[6] = 0; info[7] = 0;
    if (header[0] && c.spanGuideCells && c.dSpanGuide.p) {
        std::vector<SpanGuide> guide(c.spanGuideCells);
        GFX_HIP(hipMemcpy(guide.data(), c.dSpanGuide.p, sizeof(SpanGuide) * guide.size(), hipMemcpyDeviceToHost));
        for (const SpanGuide& g : guide) if (g.a & kGuideInterior) ++info[5];
    }
    GFX_CATCH(ctx)
}

int gfx_trace(gfx_ctx* ctx, void* stream, uint64_t accel, int mode, const void* dRayOrgTmin, const void* dRayDirTmax,
              uint32_t numRays, void* dOut, void* dCounters) {
    return gfx_trace_counted(ctx, stream, accel, mode, dRayOrgTmin, dRayDirTmax, numRays, dOut, dCounters, nullptr);
}

int gfx_trace_counted(gfx_ctx* ctx, void* stream, uint64_t accel, int mode, const void* dRayOrgTmin, const void* dRayDirTmax,
                      uint32_t numRays, void* dOut, void* dCounters, void* dPerRayItems) {
    GFX_TRY(ctx)
    if (dPerRayItems && !dCounters) throw HipError("gfx_trace_counted: per-ray item counts need the counter buffer (the counting kernel)");
    const Accel* a = find_accel(ctx, accel);
    TraceLaunch t;
    t.accel = a->dev();
    t.rayOrgTmin = static_cast<const float4*>(dRayOrgTmin);
    t.rayDirTmax = static_cast<const float4*>(dRayDirTmax);
    t.numRays = numRays; t.numRaysPtr = nullptr; t.out = dOut; t.mode = mode;
    t.perRayItems = static_cast<uint32_t*>(dPerRayItems);
    // explicit counter buffer: count into the caller's u64[4]
    const bool savedEnabled = ctx->c.countersEnabled;
    DevBuf saved = ctx->c.dTraceCounters;
    if (dCounters) { ctx->c.countersEnabled = true; ctx->c.dTraceCounters.p = dCounters; ctx->c.countersSplit = false; }
    try { trace_launch(ctx->c, static_cast<hipStream_t>(stream), t); }
    catch (...) { ctx->c.dTraceCounters = saved; ctx->c.countersEnabled = savedEnabled; ctx->c.countersSplit = true; throw; }
    ctx->c.dTraceCounters = saved; ctx->c.countersEnabled = savedEnabled; ctx->c.countersSplit = true;
    GFX_CATCH(ctx)
}

int gfx_restir_copy_to_linear(gfx_ctx* ctx, void* stream, void* dLinearColor, void* dLinearAlbedo, void* dLinearNormal, void* dLinearMotionVector) {
    GFX_TRY(ctx)
    restir_copy_to_linear(ctx->c, static_cast<hipStream_t>(stream), dLinearColor, dLinearAlbedo, dLinearNormal, dLinearMotionVector);
    GFX_CATCH(ctx)
}
int gfx_visualize(gfx_ctx* ctx, void* stream, const void* dLinearBuffer, int bufferTypeToDisplay, float motionVectorOffset, float motionVectorScale,
                  uint32_t width, uint32_t height, void* dOutputFloat4) {
    GFX_TRY(ctx)
    restir_visualize(ctx->c, static_cast<hipStream_t>(stream), dLinearBuffer, bufferTypeToDisplay, motionVectorOffset, motionVectorScale, width, height, dOutputFloat4);
    GFX_CATCH(ctx)
}

int gfx_restir_copy_depth_to_linear(gfx_ctx* ctx, void* stream, void* dLinearDepth) {
    GFX_TRY(ctx)
    restir_copy_depth_to_linear(ctx->c, static_cast<hipStream_t>(stream), dLinearDepth);
    GFX_CATCH(ctx)
}

int gfx_restir_copy_emissive_to_linear(gfx_ctx* ctx, void* stream, void* dLinearEmissive) {
    GFX_TRY(ctx)
    restir_copy_emissive_to_linear(ctx->c, static_cast<hipStream_t>(stream), dLinearEmissive);
    GFX_CATCH(ctx)
}

int gfx_denoiser_default_settings(gfx_denoiser_settings* out) {
    if (!out) return 1;
    denoiser_default_settings(out);
    return 0;
}
int gfx_denoiser_create(gfx_ctx* ctx, uint32_t width, uint32_t height, const gfx_denoiser_settings* settings, gfx_denoiser** out) {
    GFX_TRY(ctx)
    if (!out) throw HipError("gfx_denoiser_create: null output handle");
    *out = nullptr;
    gfx_denoiser_settings st;
    if (settings) st = *settings;
    else denoiser_default_settings(&st);
    std::unique_ptr<gfx_denoiser> d(new gfx_denoiser());
    d->d.device = ctx->c.device;
    try { denoiser_init(d->d, width, height, st); }
    catch (...) { denoiser_release(d->d); throw; }
    *out = d.release();
    GFX_CATCH(ctx)
}
int gfx_denoiser_destroy(gfx_denoiser* den) {
    if (!den) return 1;
    int prev = -1;
    const bool switched = hipGetDevice(&prev) == hipSuccess && prev != den->d.device && hipSetDevice(den->d.device) == hipSuccess;
    (void)hipDeviceSynchronize();
    denoiser_release(den->d);
    if (switched) (void)hipSetDevice(prev);
    delete den;
    return 0;
}
int gfx_denoise(gfx_ctx* ctx, void* stream, gfx_denoiser* den, const gfx_denoiser_inputs* in, int isFirstFrame, void* dDenoisedFloat4) {
    GFX_TRY(ctx)
    if (!den || !in) throw HipError("gfx_denoise: null denoiser or inputs");
    if (!in->beauty || !in->albedo || !in->normal || !in->flow || !dDenoisedFloat4)
        throw HipError("gfx_denoise: beauty, albedo, normal, flow and the output are required");
    if (in->width != den->d.width || in->height != den->d.height)
        throw HipError("gfx_denoise: input size differs from gfx_denoiser_create's");
    if (den->d.device != ctx->c.device) throw HipError("gfx_denoise: the denoiser belongs to another device");
    denoise(den->d, static_cast<hipStream_t>(stream), *in, isFirstFrame != 0, dDenoisedFloat4);
    GFX_CATCH(ctx)
}
int gfx_denoiser_history(gfx_denoiser* den, gfx_denoiser_history_buffers* out) {
    if (!den || !out) return 1;
    const uint32_t k = den->d.cur;
    out->lighting = den->d.lighting[k].p;
    out->moments = den->d.moments[k].p;
    out->length = den->d.length[k].p;
    out->guide = den->d.guide[k].p;
    return 0;
}

int gfx_restir_copy_taa_flow_to_linear(gfx_ctx* ctx, void* stream, void* dLinearFlow) {
    GFX_TRY(ctx)
    restir_copy_taa_flow_to_linear(ctx->c, static_cast<hipStream_t>(stream), dLinearFlow);
    GFX_CATCH(ctx)
}

int gfx_taa_create(gfx_ctx* ctx, uint32_t width, uint32_t height, uint32_t historyLength, gfx_taa** out) {
    GFX_TRY(ctx)
    if (!out) throw HipError("gfx_taa_create: null output handle");
    *out = nullptr;
    std::unique_ptr<gfx_taa> t(new gfx_taa());
    t->t.device = ctx->c.device;
    try { taa_init(t->t, width, height, historyLength); }
    catch (...) { taa_release(t->t); throw; }
    *out = t.release();
    GFX_CATCH(ctx)
}
int gfx_taa_destroy(gfx_taa* taa) {
    if (!taa) return 1;
    int prev = -1;
    const bool switched = hipGetDevice(&prev) == hipSuccess && prev != taa->t.device && hipSetDevice(taa->t.device) == hipSuccess;
    (void)hipDeviceSynchronize();
    taa_release(taa->t);
    if (switched) (void)hipSetDevice(prev);
    delete taa;
    return 0;
}
int gfx_taa_set_history_length(gfx_taa* taa, uint32_t historyLength) {
    if (!taa || historyLength < 1 || historyLength > kTaaMaxHistoryLength) return 1;
    taa->t.historyLength = historyLength;
    return 0;
}
int gfx_taa_apply(gfx_ctx* ctx, void* stream, gfx_taa* taa, const gfx_taa_inputs* in, int isFirstFrame, void* dOutFloat4) {
    GFX_TRY(ctx)
    if (!taa || !in) throw HipError("gfx_taa_apply: null TAA object or inputs");
    if (!in->color || !in->flow || !dOutFloat4) throw HipError("gfx_taa_apply: color, flow and the output are required");
    if (in->width != taa->t.width || in->height != taa->t.height) throw HipError("gfx_taa_apply: input size differs from gfx_taa_create's");
    if (dOutFloat4 == in->color) throw HipError("gfx_taa_apply: the output must not be the color input (the pass reads neighbours)");
    if (dOutFloat4 == taa->t.history[0].p || dOutFloat4 == taa->t.history[1].p)
        throw HipError("gfx_taa_apply: the output must not be the object's own history");
    if (taa->t.device != ctx->c.device) throw HipError("gfx_taa_apply: the TAA object belongs to another device");
    taa_apply(taa->t, static_cast<hipStream_t>(stream), in->color, in->flow, isFirstFrame != 0, dOutFloat4);
    GFX_CATCH(ctx)
}
int gfx_taa_history(gfx_taa* taa, const void** dHistory) {
    if (!taa || !dHistory) return 1;
    *dHistory = taa->t.history[taa->t.cur].p;
    return 0;
}

int gfx_restir_set_params(gfx_ctx* ctx, void* /*stream*/, const gfx_restir_static_params* s, const gfx_restir_frame_params* f,
                          uint32_t currentReservoirIndex, uint32_t spatialNeighborBaseIndex) {
    GFX_TRY(ctx)
    // Parameters travel by value in the kernel arguments (the reference copies three structs to
    // the device with cuMemcpyHtoDAsync per frame, restir_di_main.cpp:2350-2359).
    if (s) ctx->c.restir.s = *s;
    if (f) ctx->c.restir.f = *f;
    ctx->c.restir.currentReservoirIndex = currentReservoirIndex & 1u;
    ctx->c.restir.spatialNeighborBaseIndex = spatialNeighborBaseIndex & 1023u;
    ctx->c.restir.valid = true;
    GFX_CATCH(ctx)
}

int gfx_restir_launch(gfx_ctx* ctx, void* stream, int pass, uint32_t width, uint32_t height) {
    GFX_TRY(ctx)
    restir_launch(ctx->c, static_cast<hipStream_t>(stream), pass, width, height, 0, height);
    GFX_CATCH(ctx)
}

int gfx_restir_launch_rows_gap(gfx_ctx* ctx, void* stream, int pass, uint32_t width, uint32_t height, uint32_t rowBegin, uint32_t rowEnd,
                               uint32_t gapBegin, uint32_t gapEnd) {
    GFX_TRY(ctx)
    if (rowBegin == 0 && rowEnd == 0) rowEnd = height;
    restir_launch(ctx->c, static_cast<hipStream_t>(stream), pass, width, height, rowBegin, rowEnd, gapBegin, gapEnd);
    GFX_CATCH(ctx)
}

int gfx_restir_launch_rows(gfx_ctx* ctx, void* stream, int pass, uint32_t width, uint32_t height, uint32_t rowBegin, uint32_t rowEnd) {
    GFX_TRY(ctx)
    if (rowBegin == 0 && rowEnd == 0) rowEnd = height;   // 0, 0 = every row, as in gfx_pt_launch
    restir_launch(ctx->c, static_cast<hipStream_t>(stream), pass, width, height, rowBegin, rowEnd);
    GFX_CATCH(ctx)
}

int gfx_regir_set_params(gfx_ctx* ctx, const gfx_regir_params* p) {
    GFX_TRY(ctx)
    if (!p) throw HipError("gfx_regir_set_params: null parameters");
    if (!p->gridDimension[0] || !p->gridDimension[1] || !p->gridDimension[2]) throw HipError("gfx_regir_set_params: empty grid");
    ctx->c.regir = *p;
    ctx->c.regirValid = true;
    GFX_CATCH(ctx)
}

int gfx_nrc_set_render_params(gfx_ctx* ctx, const gfx_nrc_params* p) {
    GFX_TRY(ctx)
    if (!p) throw HipError("gfx_nrc_set_render_params: null parameters");
    ctx->c.nrcRender = *p;
    ctx->c.nrcRenderValid = true;
    GFX_CATCH(ctx)
}

int gfx_pt_launch(gfx_ctx* ctx, void* stream, int pass, uint32_t width, uint32_t height, uint32_t maxPathLength,
                  uint32_t rowBegin, uint32_t rowEnd) {
    GFX_TRY(ctx)
    if (rowEnd == 0 && rowBegin == 0) rowEnd = height;
    pathtrace_launch(ctx->c, static_cast<hipStream_t>(stream), pass, width, height, maxPathLength, rowBegin, rowEnd);
    GFX_CATCH(ctx)
}

static NrcNet* nrc_of(gfx_ctx* ctx, uint64_t handle) {
    if (handle == 0 || handle > ctx->c.nrcNets.size() || !ctx->c.nrcNets[handle - 1]) throw HipError("gfx_nrc: invalid network handle");
    return ctx->c.nrcNets[handle - 1];
}
int gfx_nrc_create(gfx_ctx* ctx, int positionEncoding, uint32_t numHiddenLayers, float learningRate, uint64_t* outHandle) {
    GFX_TRY(ctx)
    ctx->c.nrcNets.push_back(nrc_create(ctx->c, positionEncoding, numHiddenLayers, learningRate));
    *outHandle = ctx->c.nrcNets.size();
    GFX_CATCH(ctx)
}
int gfx_nrc_destroy(gfx_ctx* ctx, uint64_t handle) {
    GFX_TRY(ctx)
    NrcNet* net = nrc_of(ctx, handle);
    GFX_HIP(hipDeviceSynchronize());
    nrc_destroy(net);
    ctx->c.nrcNets[handle - 1] = nullptr;
    GFX_CATCH(ctx)
}
int gfx_nrc_infer(gfx_ctx* ctx, void* stream, uint64_t handle, const void* dInputData, uint32_t numData, void* dPredictionData) {
    GFX_TRY(ctx)
    nrc_infer(ctx->c, static_cast<hipStream_t>(stream), nrc_of(ctx, handle), static_cast<const float*>(dInputData), numData, static_cast<float*>(dPredictionData));
    GFX_CATCH(ctx)
}
int gfx_nrc_infer_indirect(gfx_ctx* ctx, void* stream, uint64_t handle, const void* dInputData, const void* dNumData, uint32_t maxNumData, void* dPredictionData) {
    GFX_TRY(ctx)
    if (!dNumData) throw HipError("gfx_nrc_infer_indirect: null batch-size pointer");
    nrc_infer(ctx->c, static_cast<hipStream_t>(stream), nrc_of(ctx, handle), static_cast<const float*>(dInputData), maxNumData, static_cast<float*>(dPredictionData),
              static_cast<const uint32_t*>(dNumData));
    GFX_CATCH(ctx)
}
int gfx_nrc_query_count_ptr(gfx_ctx* ctx, void** dNumData) {
    GFX_TRY(ctx)
    if (!ctx->c.nrcQueryCount.p) { ctx->c.nrcQueryCount.reserve(256); GFX_HIP(hipMemset(ctx->c.nrcQueryCount.p, 0, 256)); }
    *dNumData = ctx->c.nrcQueryCount.p;
    GFX_CATCH(ctx)
}
int gfx_nrc_train(gfx_ctx* ctx, void* stream, uint64_t handle, const void* dInputData, const void* dTargetData, uint32_t numData, float* lossOnCPU) {
    GFX_TRY(ctx)
    nrc_train(ctx->c, static_cast<hipStream_t>(stream), nrc_of(ctx, handle), static_cast<const float*>(dInputData), static_cast<const float*>(dTargetData), numData, lossOnCPU);
    GFX_CATCH(ctx)
}
int gfx_nrc_num_params(gfx_ctx* ctx, uint64_t handle, uint32_t* outCount) {
    GFX_TRY(ctx)
    *outCount = nrc_num_params(nrc_of(ctx, handle));
    GFX_CATCH(ctx)
}
int gfx_nrc_set_params(gfx_ctx* ctx, uint64_t handle, const float* hostParams, uint32_t count) {
    GFX_TRY(ctx)
    nrc_set_params(ctx->c, nullptr, nrc_of(ctx, handle), hostParams, count);
    GFX_CATCH(ctx)
}
int gfx_nrc_get_params(gfx_ctx* ctx, uint64_t handle, int which, float* hostOut, uint32_t count) {
    GFX_TRY(ctx)
    nrc_get_params(nrc_of(ctx, handle), which, hostOut, count);
    GFX_CATCH(ctx)
}

int gfx_nrc_inference_image(gfx_ctx* ctx, uint64_t handle, int which, void** dPtr, uint64_t* bytes) {
    GFX_TRY(ctx)
    if (!dPtr || !bytes) throw HipError("gfx_nrc_inference_image: null output");
    nrc_inference_image(ctx->c, nrc_of(ctx, handle), which, dPtr, bytes);
    GFX_CATCH(ctx)
}

int gfx_nrc_inference_image_async(gfx_ctx* ctx, void* stream, uint64_t handle, int which, void** dPtr, uint64_t* bytes) {
    GFX_TRY(ctx)
    if (!dPtr || !bytes) throw HipError("gfx_nrc_inference_image_async: null output");
    nrc_inference_image(ctx->c, nrc_of(ctx, handle), which, dPtr, bytes, static_cast<hipStream_t>(stream), true);
    GFX_CATCH(ctx)
}

int gfx_nrc_params_checksum(gfx_ctx* ctx, void* stream, uint64_t handle, void* dOutU32) {
    GFX_TRY(ctx)
    if (!dOutU32) throw HipError("gfx_nrc_params_checksum: null output");
    nrc_params_checksum(ctx->c, static_cast<hipStream_t>(stream), nrc_of(ctx, handle), static_cast<uint32_t*>(dOutU32));
    GFX_CATCH(ctx)
}

int gfx_read_device(gfx_ctx* ctx, const void* dSrc, void* hostDst, size_t bytes) {
    GFX_TRY(ctx)
    GFX_HIP(hipDeviceSynchronize());
    GFX_HIP(hipMemcpy(hostDst, dSrc, bytes, hipMemcpyDeviceToHost));
    GFX_CATCH(ctx)
}

int gfx_timing_enable(gfx_ctx* ctx, int enable) {
    GFX_TRY(ctx)
    ctx->c.timingEnabled = enable != 0;
    GFX_CATCH(ctx)
}

int gfx_timing_collect(gfx_ctx* ctx, char names[][48], float* totalMs, uint32_t* calls, uint32_t capacity, uint32_t* n) {
    GFX_TRY(ctx)
    Context& c = ctx->c;
    for (auto& e : c.pendingEvents) {
        GFX_HIP(hipEventSynchronize(e.second.second));
        float ms = 0;
        GFX_HIP(hipEventElapsedTime(&ms, e.second.first, e.second.second));
        KernelTiming& t = c.timings[e.first];
        t.ms += ms; ++t.calls;
        (void)hipEventDestroy(e.second.first); (void)hipEventDestroy(e.second.second);
    }
    c.pendingEvents.clear();
    uint32_t i = 0;
    for (const auto& kv : c.timings) {
        if (i < capacity) {
            std::memset(names[i], 0, 48);
            std::strncpy(names[i], kv.first.c_str(), 47);
            totalMs[i] = static_cast<float>(kv.second.ms); calls[i] = kv.second.calls;
        }
        ++i;
    }
    *n = i;
    c.timings.clear();
    GFX_CATCH(ctx)
}

int gfx_tunable_set(gfx_ctx* ctx, const char* name, int value) {
    GFX_TRY(ctx)
    if (!name) throw HipError("gfx_tunable_set: null name");
    Tunables& t = ctx->c.tune;
    const std::string n(name);
    auto in = [&](int lo, int hi) { if (value < lo || value > hi) throw HipError("gfx_tunable_set: value out of range for " + n); return value; };
    if (n == "pixel_map") t.pixelMap = in(0, 2);
    else if (n == "super_x") t.superShiftX = in(0, 6);
    else if (n == "super_y") t.superShiftY = in(0, 6);
    else if (n == "trace_blocks_per_cu") t.traceBlocksPerCU = in(1, 8);
    else if (n == "trace_refill") t.traceRefill = in(1, 64);
    else if (n == "temporal_hints") t.temporalHints = in(0, 1);
    else if (n == "trace_batch") t.traceBatch = in(1, 65536);
    else if (n == "pt_overlap") t.ptOverlap = in(0, 1);
    else if (n == "pt_regen") t.ptRegen = in(0, 8);
    else if (n == "pt_diag") t.ptDiag = in(0, 1);
    else if (n == "pt_regen_min") t.ptRegenMin = in(1, 64);
    else if (n == "fuse_passes") t.fusePasses = in(0, 2);
    else if (n == "block_order") t.blockOrder = in(0, 1);
    else if (n == "candidate_prefilter") t.candidatePrefilter = in(0, 1);
    else if (n == "nrc_staged_infer") t.nrcStagedInfer = in(0, 3);
    else if (n == "candidate_split") { if (value == 3) throw HipError("gfx_tunable_set: candidate_split is 0 (automatic), 1, 2 or 4"); t.candidateSplit = in(0, 4); }
    else throw HipError("gfx_tunable_set: unknown tunable " + n);
    GFX_CATCH(ctx)
}

int gfx_stream_copy(gfx_ctx* ctx, void* dDst, const void* dSrc, size_t bytes, void* stream) {
    GFX_TRY(ctx)
    stream_copy(ctx->c, static_cast<hipStream_t>(stream), dDst, dSrc, bytes);
    GFX_CATCH(ctx)
}

int gfx_bc_expand(gfx_ctx* ctx, void* stream, uint32_t bcFormat, const void* dBlocks, uint32_t width, uint32_t height, uint32_t format, void* dTexels) {
    GFX_TRY(ctx)
    if (!dBlocks || !dTexels) throw HipError("gfx_bc_expand: null pointer");
    bc_expand_launch(static_cast<hipStream_t>(stream), bcFormat, dBlocks, width, height, format, dTexels);
    GFX_CATCH(ctx)
}

int gfx_tfdm_default_params(gfx_tfdm_params* out) {
    if (!out) return 1;
    tfdm_default_params(out);
    return 0;
}
int gfx_tfdm_create(gfx_ctx* ctx, void* stream, const void* vertices, uint32_t stride, uint32_t numVertices, const uint32_t* triangles, uint32_t numTriangles,
                    const float* const* heightLevels, uint32_t numLevels, uint32_t size, const gfx_tfdm_params* params, gfx_tfdm** out) {
    GFX_TRY(ctx)
    displaced_create(ctx, "gfx_tfdm_create", out, [&](TfdmObject& o) {
        tfdm_init(o, static_cast<hipStream_t>(stream), vertices, stride, numVertices, triangles, numTriangles, heightLevels, numLevels, size, displaced_defaults(params, false)); });
    GFX_CATCH(ctx)
}
int gfx_tfdm_set_params(gfx_ctx* ctx, void* stream, gfx_tfdm* obj, const gfx_tfdm_params* params) {
    GFX_TRY(ctx)
    displaced_guard(ctx, obj, "gfx_tfdm_set_params", " or parameters", params);
    tfdm_set_params(obj->o, static_cast<hipStream_t>(stream), *params);
    GFX_CATCH(ctx)
}
int gfx_tfdm_update_heights(gfx_ctx* ctx, void* stream, gfx_tfdm* obj, const float* dSrc, uint32_t srcPitch, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h) {
    GFX_TRY(ctx)
    displaced_guard(ctx, obj, "gfx_tfdm_update_heights");
    tfdm_update_heights(ctx->c, obj->o, static_cast<hipStream_t>(stream), dSrc, srcPitch, x0, y0, w, h);
    GFX_CATCH(ctx)
}
int gfx_tfdm_destroy(gfx_tfdm* obj) { return displaced_destroy(obj); }
int gfx_tfdm_trace(gfx_ctx* ctx, void* stream, gfx_tfdm* obj, int mode, const void* dRayOrgTmin, const void* dRayDirTmax, uint32_t numRays, void* dOut, void* dCounters) {
    GFX_TRY(ctx)
    displaced_guard(ctx, obj, "gfx_tfdm_trace");
    ScopedKernelTimer timer(ctx->c, static_cast<hipStream_t>(stream), "k_tfdm_trace");
    tfdm_trace(obj->o, static_cast<hipStream_t>(stream), mode, dRayOrgTmin, dRayDirTmax, numRays, dOut, dCounters);
    GFX_CATCH(ctx)
}
int gfx_tfdm_read(gfx_ctx* ctx, gfx_tfdm* obj, int what, uint32_t level, void* hostOut, size_t bytes) {
    GFX_TRY(ctx)
    if (!obj) throw HipError("gfx_tfdm_read: null object");
    displaced_read(obj->o, what, level, hostOut, bytes);
    GFX_CATCH(ctx)
}
int gfx_tfdm_size(gfx_ctx* ctx, gfx_tfdm* obj, int what, uint32_t level, size_t* bytes) {
    GFX_TRY(ctx)
    if (!obj || !bytes) throw HipError("gfx_tfdm_size: null object or output");
    *bytes = displaced_size(obj->o, what, level);
    GFX_CATCH(ctx)
}

int gfx_nrtdsm_create(gfx_ctx* ctx, void* stream, const void* vertices, uint32_t stride, uint32_t numVertices, const uint32_t* triangles, uint32_t numTriangles,
                      const float* const* heightLevels, uint32_t numLevels, uint32_t size, const gfx_tfdm_params* params, gfx_nrtdsm** out) {
    GFX_TRY(ctx)
    displaced_create(ctx, "gfx_nrtdsm_create", out, [&](NrtdsmObject& o) {
        nrtdsm_init(o, static_cast<hipStream_t>(stream), vertices, stride, numVertices, triangles, numTriangles, heightLevels, numLevels, size, displaced_defaults(params, false)); });
    GFX_CATCH(ctx)
}
int gfx_nrtdsm_set_params(gfx_ctx* ctx, void* stream, gfx_nrtdsm* obj, const gfx_tfdm_params* params) {
    GFX_TRY(ctx)
    displaced_guard(ctx, obj, "gfx_nrtdsm_set_params", " or parameters", params);
    nrtdsm_set_params(obj->o, static_cast<hipStream_t>(stream), *params);
    GFX_CATCH(ctx)
}
int gfx_nrtdsm_update_heights(gfx_ctx* ctx, void* stream, gfx_nrtdsm* obj, const float* dSrc, uint32_t srcPitch, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h) {
    GFX_TRY(ctx)
    displaced_guard(ctx, obj, "gfx_nrtdsm_update_heights");
    nrtdsm_update_heights(ctx->c, obj->o, static_cast<hipStream_t>(stream), dSrc, srcPitch, x0, y0, w, h);
    GFX_CATCH(ctx)
}
int gfx_nrtdsm_destroy(gfx_nrtdsm* obj) { return displaced_destroy(obj); }
int gfx_nrtdsm_trace(gfx_ctx* ctx, void* stream, gfx_nrtdsm* obj, int mode, const void* dRayOrgTmin, const void* dRayDirTmax, uint32_t numRays, void* dOut, void* dCounters) {
    GFX_TRY(ctx)
    displaced_guard(ctx, obj, "gfx_nrtdsm_trace");
    ScopedKernelTimer timer(ctx->c, static_cast<hipStream_t>(stream), "k_nrtdsm_trace");
    nrtdsm_trace(obj->o, static_cast<hipStream_t>(stream), mode, dRayOrgTmin, dRayDirTmax, numRays, dOut, dCounters);
    GFX_CATCH(ctx)
}
int gfx_nrtdsm_read(gfx_ctx* ctx, gfx_nrtdsm* obj, int what, uint32_t level, void* hostOut, size_t bytes) {
    GFX_TRY(ctx)
    if (!obj) throw HipError("gfx_nrtdsm_read: null object");
    displaced_read(obj->o, what, level, hostOut, bytes);
    GFX_CATCH(ctx)
}
int gfx_nrtdsm_size(gfx_ctx* ctx, gfx_nrtdsm* obj, int what, uint32_t level, size_t* bytes) {
    GFX_TRY(ctx)
    if (!obj || !bytes) throw HipError("gfx_nrtdsm_size: null object or output");
    *bytes = displaced_size(obj->o, what, level);
    GFX_CATCH(ctx)
}

int gfx_shell_create(gfx_ctx* ctx, void* stream, const void* vertices, uint32_t stride, uint32_t numVertices, const uint32_t* triangles, uint32_t numTriangles,
                     const gfx_shell_geom* geoms, uint32_t numGeoms, const gfx_tfdm_params* params, gfx_shell** out) {
    GFX_TRY(ctx)
    displaced_create(ctx, "gfx_shell_create", out, [&](ShellObject& o) {
        shell_init(o, static_cast<hipStream_t>(stream), vertices, stride, numVertices, triangles, numTriangles, geoms, numGeoms, displaced_defaults(params, true)); });
    GFX_CATCH(ctx)
}
int gfx_shell_set_params(gfx_ctx* ctx, void* stream, gfx_shell* obj, const gfx_tfdm_params* params) {
    GFX_TRY(ctx)
    displaced_guard(ctx, obj, "gfx_shell_set_params", " or parameters", params);
    shell_set_params(obj->o, static_cast<hipStream_t>(stream), *params);
    GFX_CATCH(ctx)
}
int gfx_shell_set_geometry(gfx_ctx* ctx, void* stream, gfx_shell* obj, const gfx_shell_geom* geoms, uint32_t numGeoms) {
    GFX_TRY(ctx)
    displaced_guard(ctx, obj, "gfx_shell_set_geometry");
    shell_set_geometry(obj->o, static_cast<hipStream_t>(stream), geoms, numGeoms);
    GFX_CATCH(ctx)
}
int gfx_shell_destroy(gfx_shell* obj) { return displaced_destroy(obj); }
int gfx_shell_trace(gfx_ctx* ctx, void* stream, gfx_shell* obj, int mode, const void* dRayOrgTmin, const void* dRayDirTmax, uint32_t numRays, void* dOut, void* dCounters) {
    GFX_TRY(ctx)
    displaced_guard(ctx, obj, "gfx_shell_trace");
    ScopedKernelTimer timer(ctx->c, static_cast<hipStream_t>(stream), "k_shell_trace");
    shell_trace(obj->o, static_cast<hipStream_t>(stream), mode, dRayOrgTmin, dRayDirTmax, numRays, dOut, dCounters);
    GFX_CATCH(ctx)
}
int gfx_shell_read(gfx_ctx* ctx, gfx_shell* obj, int what, void* hostOut, size_t bytes) {
    GFX_TRY(ctx)
    if (!obj) throw HipError("gfx_shell_read: null object");
    displaced_read(obj->o, what, hostOut, bytes);
    GFX_CATCH(ctx)
}
int gfx_shell_size(gfx_ctx* ctx, gfx_shell* obj, int what, size_t* bytes) {
    GFX_TRY(ctx)
    if (!obj || !bytes) throw HipError("gfx_shell_size: null object or output");
    *bytes = displaced_size(obj->o, what);
    GFX_CATCH(ctx)
}

int gfx_tfdm_set_create(gfx_ctx* ctx, gfx_tfdm_set** out) {
    GFX_TRY(ctx)
    if (!out) throw HipError("gfx_tfdm_set_create: null output handle");
    *out = new gfx_tfdm_set();
    (*out)->s.device = ctx->c.device;
    (*out)->ctx = ctx;
    GFX_CATCH(ctx)
}
int gfx_tfdm_set_add(gfx_tfdm_set* set, gfx_tfdm* obj, const float objToWorld[12], uint32_t userId, uint32_t* index) {
    if (!set) return 1;
    GFX_TRY(set->ctx)
    const uint32_t k = tfdm_set_add(set->s, obj ? &obj->o : nullptr, objToWorld, userId);
    if (index) *index = k;
    GFX_CATCH(set->ctx)
}
int gfx_tfdm_set_add_nrtdsm(gfx_tfdm_set* set, gfx_nrtdsm* obj, const float objToWorld[12], uint32_t userId, uint32_t* index) {
    if (!set) return 1;
    GFX_TRY(set->ctx)
    const uint32_t k = tfdm_set_add_nrtdsm(set->s, obj ? &obj->o : nullptr, objToWorld, userId);
    if (index) *index = k;
    GFX_CATCH(set->ctx)
}
int gfx_tfdm_set_add_shell(gfx_tfdm_set* set, gfx_shell* obj, const float objToWorld[12], uint32_t userId, uint32_t* index) {
    if (!set) return 1;
    GFX_TRY(set->ctx)
    const uint32_t k = tfdm_set_add_shell(set->s, obj ? &obj->o : nullptr, objToWorld, userId);
    if (index) *index = k;
    GFX_CATCH(set->ctx)
}
int gfx_tfdm_set_transform(gfx_tfdm_set* set, uint32_t index, const float objToWorld[12]) {
    if (!set) return 1;
    GFX_TRY(set->ctx)
    tfdm_set_transform(set->s, index, objToWorld);
    GFX_CATCH(set->ctx)
}
int gfx_tfdm_set_move(gfx_tfdm_set* set, uint32_t index, const float objToWorld[12]) {
    if (!set) return 1;
    GFX_TRY(set->ctx)
    tfdm_set_move(set->s, index, objToWorld);
    GFX_CATCH(set->ctx)
}
int gfx_tfdm_set_commit(gfx_ctx* ctx, void* stream, gfx_tfdm_set* set) {
    GFX_TRY(ctx)
    if (!set) throw HipError("gfx_tfdm_set_commit: null set");
    if (set->s.device != ctx->c.device) throw HipError("gfx_tfdm_set_commit: the set belongs to another device");
    tfdm_set_commit(set->s, static_cast<hipStream_t>(stream));
    GFX_CATCH(ctx)
}
int gfx_tfdm_set_read(gfx_ctx* ctx, gfx_tfdm_set* set, void* hostOut, size_t bytes) {
    GFX_TRY(ctx)
    if (!set) throw HipError("gfx_tfdm_set_read: null set");
    if (set->s.device != ctx->c.device) throw HipError("gfx_tfdm_set_read: the set belongs to another device");
    tfdm_set_read(set->s, hostOut, bytes);
    GFX_CATCH(ctx)
}
int gfx_tfdm_set_read_motion(gfx_ctx* ctx, gfx_tfdm_set* set, void* hostOut, size_t bytes) {
    GFX_TRY(ctx)
    if (!set) throw HipError("gfx_tfdm_set_read_motion: null set");
    if (set->s.device != ctx->c.device) throw HipError("gfx_tfdm_set_read_motion: the set belongs to another device");
    tfdm_set_read_motion(set->s, hostOut, bytes);
    GFX_CATCH(ctx)
}
int gfx_tfdm_set_bounds(gfx_tfdm_set* set, float lo[3], float hi[3]) {
    if (!set) return 1;
    GFX_TRY(set->ctx)
    tfdm_set_bounds(set->s, lo, hi);
    GFX_CATCH(set->ctx)
}
int gfx_tfdm_set_destroy(gfx_tfdm_set* set) {
    if (!set) return 1;
    int prev = -1;
    const bool switched = hipGetDevice(&prev) == hipSuccess && prev != set->s.device && hipSetDevice(set->s.device) == hipSuccess;
    (void)hipDeviceSynchronize();
    if (set->ctx && set->ctx->c.displaced.set == &set->s) displaced_bind(set->ctx->c, nullptr, nullptr, 0, 0);
    tfdm_set_release(set->s);
    if (switched) (void)hipSetDevice(prev);
    delete set;
    return 0;
}
int gfx_trace_scene_ex(gfx_ctx* ctx, void* stream, uint64_t accel, gfx_tfdm_set* set, int mode, const void* dRayOrgTmin, const void* dRayDirTmax,
                       uint32_t numRays, void* dOut, void* dCounters, void* dShellPart) {
    GFX_TRY(ctx)
    DevAccel dev;
    if (accel) dev = find_accel(ctx, accel)->dev();
    trace_scene(ctx->c, static_cast<hipStream_t>(stream), accel ? &dev : nullptr, set ? &set->s : nullptr, ctx->scenePlain, mode, dRayOrgTmin, dRayDirTmax,
                numRays, dOut, dCounters, dShellPart);
    GFX_CATCH(ctx)
}
int gfx_trace_scene(gfx_ctx* ctx, void* stream, uint64_t accel, gfx_tfdm_set* set, int mode, const void* dRayOrgTmin, const void* dRayDirTmax,
                    uint32_t numRays, void* dOut, void* dCounters) {
    return gfx_trace_scene_ex(ctx, stream, accel, set, mode, dRayOrgTmin, dRayDirTmax, numRays, dOut, dCounters, nullptr);
}

int gfx_scene_bind_displaced(gfx_ctx* ctx, gfx_tfdm_set* set, const uint32_t* geomInstSlots, uint32_t n) {
    GFX_TRY(ctx)
    displaced_bind(ctx->c, set ? &set->s : nullptr, geomInstSlots, n, GFX_DISPLACED_GBUFFER_PT);
    GFX_CATCH(ctx)
}
int gfx_scene_bind_displaced_passes(gfx_ctx* ctx, gfx_tfdm_set* set, const uint32_t* geomInstSlots, uint32_t n, uint32_t passMask) {
    GFX_TRY(ctx)
    displaced_bind(ctx->c, set ? &set->s : nullptr, geomInstSlots, n, passMask);
    GFX_CATCH(ctx)
}
int gfx_scene_bind_displaced_kinds(gfx_ctx* ctx, gfx_tfdm_set* set, const gfx_displaced_member* members, uint32_t n, uint32_t passMask) {
    GFX_TRY(ctx)
    displaced_bind_kinds(ctx->c, set ? &set->s : nullptr, members, n, passMask);
    GFX_CATCH(ctx)
}
int gfx_restir_last_rays(gfx_ctx* ctx, void* stream, void* dRayOrgTmin, void* dRayDirTmax, void* dOccluded, uint32_t capacity, uint32_t* count) {
    GFX_TRY(ctx)
    restir_last_rays(ctx->c, static_cast<hipStream_t>(stream), dRayOrgTmin, dRayDirTmax, dOccluded, capacity, count);
    GFX_CATCH(ctx)
}
int gfx_pt_last_nee_rays(gfx_ctx* ctx, void* stream, void* dRayOrgTmin, void* dRayDirTmax, void* dOccluded, void* dOwnerPixel, uint32_t capacity,
                         uint32_t* count) {
    GFX_TRY(ctx)
    pt_last_nee_rays(ctx->c, static_cast<hipStream_t>(stream), dRayOrgTmin, dRayDirTmax, dOccluded, dOwnerPixel, capacity, count);
    GFX_CATCH(ctx)
}
int gfx_restir_primary_rays(gfx_ctx* ctx, void* stream, uint32_t width, uint32_t height, void* dRayOrgTmin, void* dRayDirTmax) {
    GFX_TRY(ctx)
    restir_primary_rays(ctx->c, static_cast<hipStream_t>(stream), width, height, dRayOrgTmin, dRayDirTmax);
    GFX_CATCH(ctx)
}

int gfx_counters_enable(gfx_ctx* ctx, int enable) {
    GFX_TRY(ctx)
    ctx->c.countersEnabled = enable != 0;
    GFX_CATCH(ctx)
}

int gfx_trace_diag_read(gfx_ctx* ctx, uint64_t diag[8], int reset) {
    GFX_TRY(ctx)
    GFX_HIP(hipDeviceSynchronize());
    for (int i = 0; i < 8; ++i) diag[i] = 0;
    if (ctx->c.dTraceDiag.p) {
        GFX_HIP(hipMemcpy(diag, ctx->c.dTraceDiag.p, 64, hipMemcpyDeviceToHost));
        if (reset) GFX_HIP(hipMemset(ctx->c.dTraceDiag.p, 0, 64));
    }
    GFX_CATCH(ctx)
}

int gfx_pt_diag_read(gfx_ctx* ctx, uint64_t diag[8], int reset) {
    GFX_TRY(ctx)
    GFX_HIP(hipDeviceSynchronize());
    for (int i = 0; i < 8; ++i) diag[i] = 0;
    if (ctx->c.ptDiag.p) {
        GFX_HIP(hipMemcpy(diag, ctx->c.ptDiag.p, 64, hipMemcpyDeviceToHost));
        if (reset) GFX_HIP(hipMemset(ctx->c.ptDiag.p, 0, 64));
    }
    GFX_CATCH(ctx)
}

int gfx_counters_read(gfx_ctx* ctx, uint64_t counters[8], int reset) {
    GFX_TRY(ctx)
    GFX_HIP(hipDeviceSynchronize());
    GFX_HIP(hipMemcpy(counters, ctx->c.dTraceCounters.p, 64, hipMemcpyDeviceToHost));
    if (reset) GFX_HIP(hipMemset(ctx->c.dTraceCounters.p, 0, 64));
    GFX_CATCH(ctx)
}

} // extern "C"
