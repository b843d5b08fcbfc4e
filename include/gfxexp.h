/*
 * gfxexp.h -- C ABI of the MI355X-native path-tracing inner loop.
 *
 * This is the drop-in boundary.  Every entry point names the reference
 * interface (file:line under the GfxExp tree) whose job it takes over.  Signatures carry plain
 * pointers and sizes only; device memory is caller-owned unless stated otherwise
 * (reference ownership model: restir_di/restir_di_main.cpp:1233-1325).
 *
 * All functions return 0 on success, non-zero on failure; gfx_last_error() gives the text
 * (the reference throws std::runtime_error from CUDADRV_CHECK, utils/cuda_util.cpp:58-69).
 * Everything is asynchronous with respect to `stream` (a hipStream_t passed as void*), and a
 * gfx_ctx is not thread-safe (same as the reference: one host thread, restir_di_main.cpp:1705).
 * A context also owns ONE set of library streams and events behind the launches (the side stream the path tracers' NEE traces and the
 * block-order sorts run on, with its fork / join events, and the scratch sets of the traversal): the launches of
 * one context (gfx_pt_launch, gfx_restir_launch*) are to be issued from one host thread, and renderers that run concurrently on
 * different streams take a context each (as the band renderers of tests/ and tools/ do).  With gfx_counters_enable the
 * per-launch diagnostics are those of the calling stream's order only when "pt_overlap" is 0.
 */
#ifndef GFXEXP_H
#define GFXEXP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GFX_INVALID_SLOT 0xFFFFFFFFu

typedef struct gfx_ctx gfx_ctx;

/* ---------------------------------------------------------------- POD layouts in HBM -------- */

/* common/common_shared.h:1109-1114 (shared::Vertex, 44 B). */
typedef struct gfx_vertex {
    float position[3];
    float normal[3];
    float texCoord0Dir[3];
    float texCoord[2];
} gfx_vertex;

/* Materials.  Every value of shared::MaterialData (common/common_shared.h:1144-1177) is a texture read through
 * tex2DLod at mip level 0 (common/common_device.cuh:143-147, 778-826).  Here a value is either a texture slot
 * (gfx_texture_set; slots are 1-based, 0 = none) or, with slot 0, the constant a / b / smoothness / emittance: what
 * the reference's 1x1 "immediate" textures return (common/common_host.cpp:1045-1073, 1602-1659), i.e. the *sampled*
 * (linear) value. */
enum gfx_bsdf_type {
    GFX_BSDF_LAMBERT = 0,              /* common/common_device.cuh:335-374 */
    GFX_BSDF_DIFFUSE_AND_SPECULAR = 1, /* common/common_device.cuh:443-765 */
    GFX_BSDF_SIMPLE_PBR = 2            /* common/common_device.cuh:767-776 */
};
enum gfx_bump_type {                   /* BumpMapTextureType -> readModifiedNormal*, common/common_device.cuh:205-240 */
    GFX_BUMP_NORMAL_MAP = 0,           /* RGB normal map: n = 2 t - 1 */
    GFX_BUMP_NORMAL_MAP_2CH = 1,       /* two channels, z = sqrt(1 - x^2 - y^2) */
    GFX_BUMP_HEIGHT_MAP = 2,           /* finite differences of the four texels under the bilinear footprint */
    GFX_BUMP_LEFT_HANDED = 0x100       /* flag: flip y (TexDimInfo::isLeftHanded) */
};
typedef struct gfx_material {
    uint32_t bsdfType;
    float a[3];          /* lambert reflectance | diffuse | baseColor */
    float b[3];          /* - | specular F0 | (occlusion, roughness, metallic) */
    float smoothness;    /* diffuse+specular only */
    float emittance[3];
    uint32_t hasEmittance; /* "mat.emittance != 0" in the reference */
    uint32_t texA;          /* texture slot for a (reflectance | diffuse | baseColor_opacity), 0 = the constant */
    uint32_t texB;          /* texture slot for b (specular | occlusion_roughness_metallic), 0 = the constant */
    uint32_t texSmoothness; /* one-channel texture for smoothness, 0 = the constant */
    uint32_t texNormal;     /* normal / height map read when gfx_restir_frame_params.enableBumpMapping, 0 = flat (0.5, 0.5, 1) */
    uint32_t texEmittance;  /* 0 = the constant */
    uint32_t bumpMapType;   /* enum gfx_bump_type, optionally | GFX_BUMP_LEFT_HANDED */
    uint32_t pad[2];
} gfx_material;

/* Texel formats and the sampler each one is read through (createTextureObject, common/common_host.cpp:1462-1481):
 * all samplers are bilinear, wrap = repeat in both directions, mip level 0. */
enum gfx_tex_format {
    GFX_TEX_RGBA8_SRGB = 0,   /* 8-bit RGBA, sampler_sRGB: R, G, B decoded sRGB -> linear per texel, A / 255 */
    GFX_TEX_RGBA8_UNORM = 1,  /* 8-bit RGBA, sampler_normFloat: c / 255 */
    GFX_TEX_R8_UNORM = 2,     /* one 8-bit channel (smoothness, height maps) */
    GFX_TEX_RG8_UNORM = 3,    /* two 8-bit channels (two-channel normal maps, BC5 decoded offline) */
    GFX_TEX_RGBA32F = 4       /* float RGBA, sampler_float (HDR emittance) */
};

/* Block-compressed formats gfx_texture_set_bc takes (the BC array types of translate, common/common_host.cpp:766-886).
 * The _sRGB DXGI variants hold the same blocks: sRGB is a property of the gfx_tex_format the slot is sampled as. */
enum gfx_bc_format {
    GFX_BC1 = 0,              /* 8-byte blocks: RGB565 endpoints, 4- or 3-colour + transparent palette */
    GFX_BC2 = 1,              /* 16 bytes: 4-bit alpha + BC1 colour (always four-colour) */
    GFX_BC3 = 2,              /* 16 bytes: interpolated alpha + BC1 colour (always four-colour) */
    GFX_BC4_UNORM = 3,        /* 8 bytes: one interpolated channel, decoded as (v, v, v, 255) */
    GFX_BC4_SNORM = 4,        /*   signed endpoints, remapped from [-127, 127] to [0, 255] */
    GFX_BC5_UNORM = 5,        /* 16 bytes: two interpolated channels, decoded as (x, y, 0, 255) */
    GFX_BC5_SNORM = 6,
    GFX_BC7 = 7               /* 16 bytes: the eight modes of the format; the reserved mode decodes to (0, 0, 0, 0) */
};

/* restir_di/restir_di_shared.h:182-204 -- same element structs, row-major linear arrays. */
typedef struct gfx_gbuffer0 { uint32_t instSlot, geomInstSlot, primIndex; uint16_t qbcB, qbcC; } gfx_gbuffer0;
typedef struct gfx_gbuffer1 { float motionVector[2]; } gfx_gbuffer1;
typedef struct gfx_gbuffer2 { float positionInWorld[3]; uint32_t qGeometricNormal; } gfx_gbuffer2;
typedef struct gfx_gbuffer3 { uint32_t qShadingNormal, qShadingTangent, qTexCoord, matSlot; } gfx_gbuffer3;

/* restir_di/restir_di_shared.h:89-96,106-139.  Reservoir<LightSample> is 48 B; in HBM it is
 * stored as THREE planes of 16 B per pixel (plane k starts at k * W*H*16 bytes) so a wavefront's
 * loads are contiguous:
 *   plane0 = (emittance.r, emittance.g, emittance.b, position.x)
 *   plane1 = (position.y, position.z, normal.x, normal.y)
 *   plane2 = (normal.z, atInfinity as u32 bits, sumWeights, streamLength as u32 bits) */
typedef struct gfx_reservoir_info { float recPDFEstimate, targetDensity; } gfx_reservoir_info; /* :141-144 */

/* restir_di/restir_di_shared.h:45-60.  orientation is row-major: o[r*3+c]. */
typedef struct gfx_camera {
    float aspect;
    float fovY;
    float position[3];
    float orientation[9];
} gfx_camera;

/* closest-hit record written by gfx_trace (common/common_shared.h:1065-1078 HitObject, compacted). */
typedef struct gfx_hit {
    float dist;          /* +inf / tmax on miss */
    float bcB, bcC;
    uint32_t triIndex;   /* index into the BVH's triangle records, GFX_INVALID_SLOT on miss */
} gfx_hit;
typedef struct gfx_tri_ids { uint32_t instSlot, geomInstSlot, primIndex; } gfx_tri_ids;

/* ---------------------------------------------------------------- context ------------------- */

/* restir_di/restir_di_main.cpp:128-136 (cuInit, cuCtxCreate, optixu::Context::create). */
int gfx_ctx_create(int device, gfx_ctx** out);
void gfx_ctx_destroy(gfx_ctx* ctx);
const char* gfx_last_error(gfx_ctx* ctx);
/* Library build identification: "gfxexp_amd <version> gfx950". */
const char* gfx_version(void);

/* ---------------------------------------------------------------- scene --------------------- */

/* common/common_host.cpp:1454-1815 (create*Material): constants and / or texture slots. */
int gfx_material_set(gfx_ctx* ctx, uint32_t matSlot, const gfx_material* mat);
/* Texture upload (loadTexture + cudau::Array::write + createTextureObject, common/common_host.cpp:1163-1244,
 * 1462-1481).  texSlot >= 1; texels are tightly packed rows, row 0 first, in `format`.
 * The CUDA texture unit is replaced by a software tex2DLod with a written contract ("Textures"):
 *   x = (u - floor(u)) * W - 0.5, i = floor(x), alpha = round_to_8_fraction_bits(x - i)   (likewise y, beta)
 *   T = ((1-alpha)(1-beta)) T[i,j] + (alpha (1-beta)) T[i+1,j] + ((1-alpha) beta) T[i,j+1] + (alpha beta) T[i+1,j+1]
 * with indices wrapped modulo W / H, fp32 arithmetic in exactly this order, 8-bit texels decoded per texel
 * before filtering (c / 255, or the exact sRGB formula rounded to fp32). */
int gfx_texture_set(gfx_ctx* ctx, uint32_t texSlot, uint32_t width, uint32_t height, uint32_t format, const void* texels);
/* Inspection: tex2DLod<float4> (gather = 0) or tex2Dgather<float4> of component 0 (gather = 1) of one texture at n
 * coordinates; dUv = device float2[n], dOut = device float4[n].  Runs the functions the shading kernels call. */
int gfx_texture_sample(gfx_ctx* ctx, void* stream, uint32_t texSlot, const void* dUv, uint32_t n, void* dOut, int gather);
/* Block-compressed upload (the .dds branch of loadTexture, common/common_host.cpp:1163-1244, where the reference writes the blocks
 * into a BC array and the texture unit decodes them).  blocks = ceil(width / 4) * ceil(height / 4) blocks of `bcFormat`
 * (enum gfx_bc_format), row-major, tightly packed: level 0 of a DDS as it lies in the file.  `format` is the 8-bit gfx_tex_format
 * the slot is sampled as (GFX_TEX_RGBA32F is refused); R8 / RG8 keep the first one / two channels of the decoded RGBA8 texel.
 * The blocks are copied to the device here and expanded there at every scene upload, so the slot renders bit for bit like the
 * same texels given to gfx_texture_set; the decoded bytes are those of tools/dds_convert.py.
 * Same slot and size rules as gfx_texture_set; setting a slot again, by either call, replaces it.  A refused call leaves the
 * slot as it was. */
int gfx_texture_set_bc(gfx_ctx* ctx, uint32_t texSlot, uint32_t width, uint32_t height, uint32_t bcFormat, const void* blocks, uint32_t format);
/* Inspection: the texels of a slot as they lie in the device pool, in the slot's format (tightly packed rows); `bytes` must be
 * the slot's size exactly.  Uploads the scene first if it is dirty; works for uncompressed and block-compressed slots alike. */
int gfx_texture_read(gfx_ctx* ctx, void* stream, uint32_t texSlot, void* hostOut, size_t bytes);

/* common/common_host.cpp:1817-1905 createGeometryInstance: host vertex/triangle arrays in,
 * geomInstSlot out.  `vertexStride` >= sizeof(gfx_vertex). */
int gfx_geom_create(gfx_ctx* ctx, const void* vertices, uint32_t vertexStride, uint32_t numVertices,
                    const uint32_t* triangles, uint32_t numTriangles, uint32_t matSlot,
                    uint32_t* geomInstSlot);
/* common/common_host.cpp:2051-2078 createGeometryGroup. */
int gfx_group_create(gfx_ctx* ctx, const uint32_t* geomInstSlots, uint32_t n, uint32_t* group);
/* common/common_host.cpp:2582-2656 createInstance: xfm is 3x4 row-major (the float[12] handed to
 * optixInst.setTransform).  instSlot doubles as the OptiX instance id. */
int gfx_instance_create(gfx_ctx* ctx, uint32_t group, const float xfm[12], uint32_t* instSlot);
/* common/common_host.h:837-855 InstanceController::update, the InstanceData part: xfm becomes the instance's
 * object-to-world matrix and curToPrevTransform = (previous matrix) * invert(xfm), so the next G-buffer pass
 * writes motion vectors for the instance (optix_gbuffer_kernels.cu:132).  Like the reference's controllers, call
 * it every frame for an animated instance (a frame without a call keeps the last curToPrevTransform), then
 * gfx_accel_build again (Scene::updateASs, restir_di_main.cpp:2263-2264); the emitter distributions and
 * records are rebuilt by the next gfx_lights_build_instances.  The normal matrix is recomputed as
 * transpose(invert(upper-left 3x3)) like at creation; ..._and_normal_matrix takes the controller's own
 * matRot / curScale (row-major 3x3, common_host.h:843) for a bit-exact shim. */
int gfx_instance_set_transform(gfx_ctx* ctx, uint32_t instSlot, const float xfm[12]);
int gfx_instance_set_transform_and_normal_matrix(gfx_ctx* ctx, uint32_t instSlot, const float xfm[12], const float normalMatrix[9]);
/* Declares an instance animated before the first gfx_accel_build.  Animated instances live in their own BVH
 * subtree under a two-child root; gfx_instance_set_transform on them followed by gfx_accel_build (same handle)
 * rebuilds only that subtree -- a few small kernels for a light or two -- instead of the whole tree.  An instance
 * that was not declared becomes animated at its first gfx_instance_set_transform (one full rebuild). */
int gfx_instance_set_dynamic(gfx_ctx* ctx, uint32_t instSlot, int dynamic);

/* common/common_host.h:1027-1100 Scene::updateASs -> OptixTraversableHandle.  Builds the HIP
 * LBVH -> BVH8 over all instances (world space).  The 64-bit handle fits the reference's
 * perFramePlp.travHandle field (restir_di_main.cpp:2264). */
int gfx_accel_build(gfx_ctx* ctx, void* stream, uint64_t* handle);
/* Leaf size limit of the collapse step, 1..4 (default 4; a node's leaf triangles fit one 32-bit mask); GeometryBVHBuildConfig::maxNumPrimsPerLeaf,
 * common/bvh_builder.h:38-44. */
int gfx_accel_set_max_leaf(gfx_ctx* ctx, uint32_t maxLeafTris);
/* Build statistics of the last gfx_accel_build: {numTriangles, numNodes, numTriRecords, maxDepth}. */
int gfx_accel_stats(gfx_ctx* ctx, uint64_t handle, uint32_t stats[4]);
/* Device pointer to the gfx_tri_ids table of the BVH (indexed by gfx_hit.triIndex). */
int gfx_accel_tri_ids(gfx_ctx* ctx, uint64_t handle, const void** dTriIds, uint32_t* count);

/* common/common_host.h:1102-1266 setupLightGeomDistributions (once) and
 * :1268-1359 setupLightInstDistribution (per frame; restir_di_main.cpp:2303-2309). */
int gfx_lights_build_static(gfx_ctx* ctx, void* stream);
int gfx_lights_build_instances(gfx_ctx* ctx, void* stream, uint32_t bufferIndex);
/* Read back the three-level distribution for inspection/tests: level 0 = instances,
 * 1 = geomInsts of instance `index`, 2 = emitter triangles of geomInst `index`.
 * weights/cdf may be NULL; returns the element count in *n and the integral in *integral. */
int gfx_lights_read(gfx_ctx* ctx, uint32_t level, uint32_t index, float* weights, float* cdf,
                    uint32_t capacity, uint32_t* n, float* integral);

/* State of the emitter interval table the last gfx_lights_build_instances produced (the three searches of
 * sampleLight, restir_di_shared.h:366-415, flattened into one lookup): info = { usable (the build verified it
 * against the three searches; 0 = kernels run the searches themselves), records verified, records, guide cells,
 * distinct normal matrices among the emitter instances, interior guide cells (a lookup that lands in one is done after
 * one load), 0, 0 }. */
int gfx_lights_table_info(gfx_ctx* ctx, uint32_t info[8]);

/* Inspection / test entry of the light sampler: one light sample per (ul, u0, u1, unused) of dU (float4[n]) with the device
 * functions the passes call, no environment light.  GFX_LIGHTS_SAMPLE: sampleLight<false> as the kernels run it (the interval
 * table when the build verified it, else the three searches); GFX_LIGHTS_SAMPLE_SEARCH: the three searches whatever the
 * table's state; GFX_LIGHTS_SAMPLE_SOLID_ANGLE: sampleLight<true> from shadingPoint (may be NULL in the other modes).
 * dOut = gfx_light_sample_record[n].  Both buffers 16-byte aligned; needs gfx_lights_build_static and
 * gfx_lights_build_instances since the last change of the scene. */
enum gfx_lights_sample_mode { GFX_LIGHTS_SAMPLE = 0, GFX_LIGHTS_SAMPLE_SEARCH = 1, GFX_LIGHTS_SAMPLE_SOLID_ANGLE = 2 };
typedef struct gfx_light_sample_record {
    float emittance[3]; float areaPDensity;
    float position[3]; uint32_t atInfinity;
    float normal[3]; uint32_t record;          /* emitter record index; 0xFFFFFFFF: the pick returned early, density 0 */
    uint32_t instSlot; uint32_t tableUsed;     /* instSlot 0xFFFFFFFF with record */
    uint32_t pad[2];
} gfx_light_sample_record;
int gfx_lights_sample(gfx_ctx* ctx, void* stream, int mode, const float shadingPoint[3], const void* dU, uint32_t n, void* dOut);

/* Inspection / test entry of the deterministic math contract (csrc/gm_math.hip.h, contract version 1) and of the 16-bit
 * quantisers on top of it (csrc/shading.hip.h): function `fn` on n arguments with the device functions the passes call.
 * dA, dB = device float4[n] (dB may be NULL unless fn reads it); dOut = device uint32_t[4][n]: result word k of element i at
 * dOut[k * n + i], floats as their bits, unused words 0.  All buffers 16-byte aligned.
 *   GFX_MATH_SINCOS             A.x              -> gm_sincos s, c; gm_tan; gm_sin
 *   GFX_MATH_EXP / ACOS / ATAN  A.x              -> gm_exp / gm_acos / gm_atan
 *   GFX_MATH_ATAN2              y = A.x, x = A.y -> gm_atan2
 *   GFX_MATH_SAT                A.x              -> f2i_sat, f2u_sat, q16
 *   GFX_MATH_TO_POLAR           A.xyz            -> to_polar_yup phi, theta; encode_dir
 *   GFX_MATH_DECODE_DIR         bits of A.x      -> decode_dir x, y, z
 *   GFX_MATH_ENCODE_UV          u = A.x, v = A.y -> encode_uv
 *   GFX_MATH_DECODE_UV          bits of A.x      -> decode_uv u, v
 *   GFX_MATH_ENCODE_BC          A.x              -> encode_bc
 *   GFX_MATH_DECODE_BC          low 16 bits of A.x -> decode_bc
 *   GFX_MATH_OFFSET_RAY_ORIGIN  p = A.xyz, n = B.xyz -> offset_ray_origin x, y, z */
enum gfx_math_fn { GFX_MATH_SINCOS = 0, GFX_MATH_EXP = 1, GFX_MATH_ACOS = 2, GFX_MATH_ATAN = 3, GFX_MATH_ATAN2 = 4, GFX_MATH_SAT = 5,
                   GFX_MATH_TO_POLAR = 6, GFX_MATH_DECODE_DIR = 7, GFX_MATH_ENCODE_UV = 8, GFX_MATH_DECODE_UV = 9, GFX_MATH_ENCODE_BC = 10,
                   GFX_MATH_DECODE_BC = 11, GFX_MATH_OFFSET_RAY_ORIGIN = 12 };
int gfx_math_eval(gfx_ctx* ctx, void* stream, int fn, const void* dA, const void* dB, uint32_t n, void* dOut);

/* Inspection / test entry of the shading layer (csrc/shading.hip.h): the BSDFs, the hemisphere sampler, the shading frame with its
 * bump mapping and the unshadowed direct-lighting term, on n elements with the device functions the passes call.
 * The material is given per element as constants: dMat = device float4[2 n], element i = (bits of bsdfType, a.rgb), (b.rgb, smoothness);
 * every texture slot is 0 and Bsdf::setup runs on the device.  dA, dB = device float4[n]; dC = device float4[4 n] (four per element).
 * A list a function does not read may be NULL; one it reads must not.  dOut = device uint32_t[words][n] with
 * words = gfx_bsdf_eval_words(fn): result word k of element i at dOut[k * n + i], floats as their bits, unused words 0.  All buffers
 * 16-byte aligned; n == 0 touches nothing.
 *   GFX_BSDF_SETUP (8 words)             mat                                   -> diffuse rgb, specularF0 rgb, roughness
 *   GFX_BSDF_EVALUATE (4)                mat, vGiven = A.xyz, vSampled = B.xyz -> evaluate rgb
 *   GFX_BSDF_PDF (4)                     mat, vGiven = A.xyz, vSampled = B.xyz -> evaluate_pdf
 *   GFX_BSDF_SAMPLE (8)                  mat, vGiven = A.xyz, u0 = B.x, u1 = B.y -> sample_throughput rgb, direction xyz, density
 *                                        (the direction is 0 where sample_throughput returns before writing it)
 *   GFX_BSDF_DHR (4)                     mat, vGiven = A.xyz                   -> dh_reflectance_estimate rgb
 *   GFX_BSDF_COSINE_HEMISPHERE (8)       u0 = A.x, u1 = A.y                    -> concentric_disk dx, dy; cosine_hemisphere xyz
 *   GFX_BSDF_COORDINATE_SYSTEM (8)       n = A.xyz                             -> make_coordinate_system tangent xyz, bitangent xyz
 *   GFX_BSDF_BUMP_FRAME (16)             n = A.xyz, t = B.xyz, modNormal = C[0].xyz, probe = C[1].xyz
 *                                        -> Frame(n, t) after apply_bump_mapping: t, b, n; to_local(probe); from_local(probe)
 *   GFX_BSDF_DIRECT_LIGHTING (12)        mat, shadingPoint = A.xyz, vOutLocal = B.xyz, Frame(C[0].xyz, C[1].xyz), light sample:
 *                                        emittance = C[2].xyz, position = C[3].xyz, normal = (C[0].w, C[1].w, C[2].w), atInfinity = bits of C[3].w
 *                                        -> shadow_ray dir xyz, dist2, tmax; direct_lighting rgb; target_weight */
enum gfx_bsdf_fn { GFX_BSDF_SETUP = 0, GFX_BSDF_EVALUATE = 1, GFX_BSDF_PDF = 2, GFX_BSDF_SAMPLE = 3, GFX_BSDF_DHR = 4, GFX_BSDF_COSINE_HEMISPHERE = 5,
                   GFX_BSDF_COORDINATE_SYSTEM = 6, GFX_BSDF_BUMP_FRAME = 7, GFX_BSDF_DIRECT_LIGHTING = 8, GFX_BSDF_FN_COUNT = 9 };
int gfx_bsdf_eval(gfx_ctx* ctx, void* stream, int fn, const void* dMat, const void* dA, const void* dB, const void* dC, uint32_t n, void* dOut);
/* result words per element of gfx_bsdf_eval(fn); 0 for an unknown fn */
uint32_t gfx_bsdf_eval_words(int fn);

/* ---------------------------------------------------------------- ray queries ---------------- */

/* Replaces optixTrace (utils/optix_util.h:557-603) for wavefront ray queues and the scalar
 * bvh::traverse (common/bvh_builder.cpp:1272-1649).
 *   rayOrgTmin[i] = (org.xyz, tmin), rayDirTmax[i] = (dir.xyz, tmax); intervals are exclusive.
 *   mode CLOSEST: out = gfx_hit[numRays];  mode ANY: out = uint32_t[numRays] (1 = occluded).
 * counters (optional, device u64[4]): node fetches, triangle fetches, rays, stack spills. */
enum gfx_trace_mode { GFX_TRACE_CLOSEST = 0, GFX_TRACE_ANY = 1 };
int gfx_trace(gfx_ctx* ctx, void* stream, uint64_t accel, int mode,
              const void* dRayOrgTmin, const void* dRayDirTmax, uint32_t numRays,
              void* dOut, void* dCounters);
/* The same through the counting instantiation, additionally writing how many 64-byte items (BVH8 nodes + triangle
 * records) each ray fetched to dPerRayItems (device u32[numRays]): the work distribution a scene asks of the traversal
 * (tools/bvh_quality.py reports its histogram).  dCounters must be given. */
int gfx_trace_counted(gfx_ctx* ctx, void* stream, uint64_t accel, int mode,
                      const void* dRayOrgTmin, const void* dRayDirTmax, uint32_t numRays,
                      void* dOut, void* dCounters, void* dPerRayItems);

/* ---------------------------------------------------------------- ReSTIR DI ------------------ */

/* restir_di/restir_di_shared.h:208-239 StaticPipelineLaunchParameters with surfaces/textures
 * replaced by plain device pointers (row-major, pixel p = y*W + x). */
typedef struct gfx_restir_static_params {
    int32_t imageSizeX, imageSizeY;
    void* rngBuffer;                 /* uint64_t[W*H]  (PCG32RNG state) */
    void* gbuffer0[2];
    void* gbuffer1[2];
    void* gbuffer2[2];
    void* gbuffer3[2];
    void* reservoirBuffer[2];        /* 3 planes x W*H x 16 B */
    void* reservoirInfoBuffer[2];    /* gfx_reservoir_info[W*H] */
    void* sampleVisibilityBuffer[2]; /* uint32_t[W*H] (rearchitected only) */
    const void* spatialNeighborDeltas; /* float2[1024] */
    void* beautyAccumBuffer;         /* float4[W*H] */
    void* albedoAccumBuffer;
    void* normalAccumBuffer;
    int32_t numTilesX, numTilesY;    /* rearchitected only */
    void* lightPreSamplingRngs;      /* uint64_t[131072] */
    void* preSampledLights;          /* 48 B x 131072 */
    /* environment light (restir_di_shared.h:221-222); NULL = none */
    const void* envLightTexture;     /* float4[envW*envH], lat-long */
    int32_t envWidth, envHeight;
    const void* envRowPDF;           /* float[envH*envW]      conditional PDFs per row */
    const void* envRowCDF;           /* float[envH*(envW+1)] */
    const void* envRowIntegrals;     /* float[envH] */
    const void* envTopPDF;           /* float[envH] */
    const void* envTopCDF;           /* float[envH+1] */
    float envTopIntegral;
    /* Optional guide tables over the environment CDFs (gfxh_env_build_guides; NULL = plain binary search, same
     * results): uint16_t[envH*envW] / uint16_t[envH], entry k = largest index whose CDF value lies in cell <= k
     * of envW (envH) equal cells of [0,1). */
    const void* envRowGuide;
    const void* envTopGuide;
    /* Optional: the rows of the map with everything a light sample on it reads in one place (gfxh_env_build_row_table; NULL = the
     * separate arrays above, same results): envH x (envW + 1) records of 32 bytes {float cdf, pdf; uint32 guide; float r, g, b; 8 B
     * unused} -- record (row, i) = envRowCDF[row * (envW + 1) + i], envRowPDF[row * envW + i], envRowGuide[row * envW + i] and texel
     * (i, row) (zero where i = envW has none); the seventh word is the NEXT record's cdf.  Rows are GFX_ENV_ROW_STRIDE(envW) records apart
     * (a multiple of four: groups of four records are 128-byte lines).  A sample then touches two or three 64-byte sectors instead of six
     * or seven. */
    const void* envRowTable;
    /* Optional, with envRowTable (gfxh_env_build_row_sketch; NULL = the guide inside the records): records of GFX_ENV_SKETCH_WORDS words --
     * 33 floats = an inverse CDF (in columns) at 33 equidistant u, a 32-bit mask, the index of the record's first child record, one unused
     * word.  Record `row` (0 .. envH - 1) covers u in [0, 1) of that row: mask bit k set = for every u of cell k = [k/32, (k+1)/32) the linear
     * interpolation of knots k and k + 1 lands within one column of the column the bisection finds (verified by the builder for every
     * column of the cell, with the device's arithmetic); the sign bit of knot k repeats the verdict (set = failed), so a sample of a
     * verified cell reads the two knots and nothing else.  A cell that fails has a CHILD record (envH + first child + its rank among the
     * record's failing cells) that covers the cell's range of u the same way at 1/32 of the step; a sub-cell that fails again keeps the
     * guide.  A sample of a verified (sub-)cell reads ONE 128-byte line of the row table (the group of four records around the
     * prediction; a neighbouring line in the few cases the column sits across its edge) instead of the guide's line plus the column's;
     * the records (envH + a few hundred) stay in L2.  Same column, same sample. */
    const void* envRowSketch;
} gfx_restir_static_params;
#define GFX_ENV_ROW_STRIDE(envW) ((((uint32_t)(envW)) + 1u + 3u) & ~3u)
#define GFX_ENV_SKETCH_CELLS 32u
#define GFX_ENV_SKETCH_WORDS 36u

/* restir_di/restir_di_shared.h:241-281 PerFramePipelineLaunchParameters. */
typedef struct gfx_restir_frame_params {
    uint64_t travHandle;
    uint32_t numAccumFrames;
    uint32_t frameIndex;
    gfx_camera camera;
    gfx_camera prevCamera;
    float envLightPowerCoeff;
    float envLightRotation;
    float spatialNeighborRadius;
    float radiusThresholdForSpatialVisReuse;
    uint32_t log2NumCandidateSamples;
    uint32_t numSpatialNeighbors;
    uint32_t useLowDiscrepancyNeighbors;
    uint32_t reuseVisibility;
    uint32_t reuseVisibilityForTemporal;
    uint32_t reuseVisibilityForSpatiotemporal;
    uint32_t enableTemporalReuse;
    uint32_t enableSpatialReuse;
    uint32_t useUnbiasedEstimator;
    uint32_t bufferIndex;
    uint32_t resetFlowBuffer;
    uint32_t enableJittering;
    uint32_t enableEnvLight;
    uint32_t enableBumpMapping;
    /* path tracers: sampleLight<true> / computeSurfacePoint<.., true> -- emitter triangles sampled uniformly in the
     * solid angle they subtend from the shading point (restir_di_shared.h:417-483, path_tracing_shared.h:319-385,
     * 550-568; a compile-time `useSolidAngleSampling = false` in the reference, a run-time switch here) */
    uint32_t useSolidAngleSampling;
} gfx_restir_frame_params;

/* restir_di/restir_di_main.cpp:2350-2359: the three cuMemcpyHtoDAsync of plp/perFramePlp.
 * currentReservoirIndex is 1 bit, spatialNeighborBaseIndex wraps to 10 bits
 * (restir_di_shared.h:283-288). */
int gfx_restir_set_params(gfx_ctx* ctx, void* stream,
                          const gfx_restir_static_params* s, const gfx_restir_frame_params* f,
                          uint32_t currentReservoirIndex, uint32_t spatialNeighborBaseIndex);

/* restir_di/restir_di_main.cpp:72-95 entry-point enums; pipeline.launch(stream, plp, W, H, 1)
 * at :2366-2420. */
enum gfx_restir_pass {
    GFX_RESTIR_SETUP_GBUFFERS = 0,                 /* optix_gbuffer_kernels.cu:5-243 */
    GFX_RESTIR_INITIAL_RIS = 1,                    /* optix_restir_di_kernels.cu:289-291 */
    GFX_RESTIR_INITIAL_AND_TEMPORAL_BIASED = 2,    /* :293-295 */
    GFX_RESTIR_INITIAL_AND_TEMPORAL_UNBIASED = 3,  /* :297-299 */
    GFX_RESTIR_SPATIAL_BIASED = 4,                 /* :549-551 */
    GFX_RESTIR_SPATIAL_UNBIASED = 5,               /* :553-555 */
    GFX_RESTIR_SHADING = 6,                        /* :559-637 */
    /* Rearchitected ReSTIR (restir_di_main.cpp:2423-2487).  preSampledLights = 131072 x 48 B
     * ([emittance.rgb, position.x] [position.yz, normal.xy] [normal.z, atInfinity, areaPDensity, 0]),
     * lightPreSamplingRngs = 131072 x u64 seeded from mt19937_64(894213312210) (:1216-1219),
     * sampleVisibilityBuffer = the SampleVisibility bit union of restir_di_shared.h:146-164. */
    GFX_RESTIR_LIGHT_PRESAMPLING = 7,              /* per_pixel_ris.cu:6-40 */
    GFX_RESTIR_PER_PIXEL_RIS = 8,                  /* per_pixel_ris.cu:44-128 (8x8 tiles) */
    /* optix_restir_di_rearch_kernels.cu:227-253, in the order of RearchitectedReSTIREntryPoint
     * (restir_di_main.cpp:83-95) */
    GFX_RESTIR_TRACE_SHADOW_RAYS = 9,
    GFX_RESTIR_TRACE_SHADOW_RAYS_TEMPORAL_BIASED = 10,
    GFX_RESTIR_TRACE_SHADOW_RAYS_SPATIAL_BIASED = 11,
    GFX_RESTIR_TRACE_SHADOW_RAYS_SPATIOTEMPORAL_BIASED = 12,
    GFX_RESTIR_TRACE_SHADOW_RAYS_TEMPORAL_UNBIASED = 13,
    GFX_RESTIR_TRACE_SHADOW_RAYS_SPATIAL_UNBIASED = 14,
    GFX_RESTIR_TRACE_SHADOW_RAYS_SPATIOTEMPORAL_UNBIASED = 15,
    GFX_RESTIR_SHADE_AND_RESAMPLE = 16,            /* :649-663 */
    GFX_RESTIR_SHADE_AND_RESAMPLE_TEMPORAL = 17,
    GFX_RESTIR_SHADE_AND_RESAMPLE_SPATIAL = 18,
    GFX_RESTIR_SHADE_AND_RESAMPLE_SPATIOTEMPORAL = 19,
    /* No reference entry point of its own: GFX_RESTIR_SPATIAL_BIASED followed by GFX_RESTIR_SHADING of the reservoirs that pass wrote
     * (currentReservoirIndex is the spatial pass's; the shading reads the other buffer), as restir_di_main.cpp:2393-2420 issues them for
     * the last spatial pass of a frame.  Both on the same rows.  One kernel where the launch is small (a row band), two launches otherwise;
     * same results as the two calls. */
    GFX_RESTIR_SPATIAL_BIASED_AND_SHADING = 20,
    GFX_RESTIR_NUM_PASSES
};
int gfx_restir_launch(gfx_ctx* ctx, void* stream, int pass, uint32_t width, uint32_t height);
/* The same pass restricted to image rows [rowBegin, rowEnd): the unit of the multi-GPU row-band split
 * (no reference counterpart -- restir_di_main.cpp is single GPU, :130-133).  Buffers keep their
 * full-frame size and indexing.  rowBegin == rowEnd == 0 -> every row. */
int gfx_restir_launch_rows(gfx_ctx* ctx, void* stream, int pass, uint32_t width, uint32_t height,
                           uint32_t rowBegin, uint32_t rowEnd);
/* Rows [rowBegin, gapBegin) and [gapEnd, rowEnd) in ONE launch: the seam rows of a band (what the neighbours' next pass reads), which
 * a band renderer runs ahead of the interior [gapBegin, gapEnd) so that their exchange overlaps the interior (gfxexp_host.h, lane
 * SEAM).  GFX_RESTIR_SPATIAL_BIASED only (a per-pixel kernel: which launch computes a pixel changes nothing). */
int gfx_restir_launch_rows_gap(gfx_ctx* ctx, void* stream, int pass, uint32_t width, uint32_t height,
                               uint32_t rowBegin, uint32_t rowEnd, uint32_t gapBegin, uint32_t gapEnd);

/* Output chain (restir_di/gpu_kernels/copy_buffers.cu:6-80; host calls restir_di_main.cpp:2497-2571).
 * gfx_restir_copy_to_linear = copyToLinearBuffers: beauty / albedo / normal accumulation buffers (normal normalised
 * unless zero) and GBuffer1's motion vectors of the current gfx_restir_set_params into caller-owned linear device
 * arrays (float4 x 3, float2).  gfx_visualize = visualizeToOutputBuffer: one linear buffer -> float4 display values. */
enum gfx_buffer_to_display {                       /* BufferToDisplay, restir_di_shared.h:292-298 */
    GFX_DISPLAY_NOISY_BEAUTY = 0, GFX_DISPLAY_ALBEDO = 1, GFX_DISPLAY_NORMAL = 2, GFX_DISPLAY_FLOW = 3, GFX_DISPLAY_DENOISED_BEAUTY = 4
};
int gfx_restir_copy_to_linear(gfx_ctx* ctx, void* stream, void* dLinearColor, void* dLinearAlbedo, void* dLinearNormal, void* dLinearMotionVector);
int gfx_visualize(gfx_ctx* ctx, void* stream, const void* dLinearBuffer, int bufferTypeToDisplay, float motionVectorOffset, float motionVectorScale,
                  uint32_t width, uint32_t height, void* dOutputFloat4);
/* Camera distance |GBuffer2.positionInWorld - camera.position| of the current gfx_restir_set_params for pixels with a surface
 * (GBuffer0.instSlot != ~0u), +inf otherwise, into a caller-owned float[W*H]: the depth guide of gfx_denoise (the reference's
 * denoiser takes none; svgf/ reads the GL raster depth buffer, svgf_main.cpp). */
int gfx_restir_copy_depth_to_linear(gfx_ctx* ctx, void* stream, void* dLinearDepth);
/* 1 for pixels whose surface emits (GBuffer0.instSlot != ~0u and the material of GBuffer3.matSlot has emittance), 0 otherwise, into a
 * caller-owned uint32[W*H]: the emissive guide of gfx_denoise.  The beauty of such a pixel is emission plus reflected light, and
 * dividing it by the albedo (the reference's demodulation, svgf/gpu_kernels/optix_pathtracing_kernels.cu:354) yields values that
 * the a-trous stages would spread to the pixel's neighbours; the denoiser passes these pixels through instead. */
int gfx_restir_copy_emissive_to_linear(gfx_ctx* ctx, void* stream, void* dLinearEmissive);

/* ---------------------------------------------------------------- SVGF temporal denoiser ------ */

/* Stands in for the OptiX temporal denoiser of restir_di_main.cpp (setup :1400-1432, invoke :2504-2533): the open SVGF of
 * svgf/gpu_kernels (temporal reprojection with moments optix_pathtracing_kernels.cu:55-130 and :354-364, variance estimate
 * svgf.cu:30-130, edge-stopped a-trous stages :132-350, albedo re-modulation :378-611) restated over the linear buffers
 * gfx_restir_copy_to_linear writes plus an optional depth guide.  The order of operations is specified in
 * gfxexp_amd/csrc/denoise/denoise.hip; the CPU restatement of tests/denoise_ref.cpp follows the same text bit for bit. */
typedef struct gfx_denoiser gfx_denoiser;   /* opaque; owns its double-buffered history and scratch buffers */
enum gfx_denoise_kernel {                   /* ATrousKernelType, svgf.cu:138-218 */
    GFX_DENOISE_BOX3X3 = 0,                 /* the kernel svgf.cu launches (applyATrousFilter_box3x3) */
    GFX_DENOISE_GAUSS3X3 = 1,
    GFX_DENOISE_GAUSS5X5 = 2
};
typedef struct gfx_denoiser_settings {
    uint32_t numStages;      /* a-trous stages 0..5 with steps 1 2 4 8 16 (0 = temporal accumulation + re-modulation only); default 5 */
    uint32_t kernel;         /* gfx_denoise_kernel; default GFX_DENOISE_BOX3X3 */
    uint32_t feedbackStage;  /* 1 = the history takes stage 0's output (feedback1stFilteredResult, SVGF's default), 0 = the unfiltered
                                integrated lighting */
    float sigmaZ;            /* 1 (svgf.cu:8) */
    float sigmaN;            /* 128 (svgf.cu:15); a power of two 1..1024: pow(x, 2^k) is k squarings */
    float sigmaL;            /* 4 (svgf.cu:22) */
    float minAlpha;          /* 0.2: the 1/5 EMA floor of svgf/gpu_kernels/optix_pathtracing_kernels.cu:358-361; 0..1 */
} gfx_denoiser_settings;
typedef struct gfx_denoiser_inputs {
    uint32_t width, height;  /* of every buffer below; must equal gfx_denoiser_create's */
    const void* beauty;      /* float4[W*H], the layout gfx_restir_copy_to_linear writes; alpha is copied to the output */
    const void* albedo;      /* float4 */
    const void* normal;      /* float4, unit or zero (zero = no surface) */
    const void* flow;        /* float2: the motion vector as the G-buffer pass writes it, pixel centre minus previous position, in pixels */
    const void* depth;       /* optional float[W*H]: camera distance, +inf = background (gfx_restir_copy_depth_to_linear); NULL = no depth term */
    const void* emissive;    /* optional uint32[W*H]: nonzero = an emitting surface (gfx_restir_copy_emissive_to_linear), passed through
                                like background and never a neighbour; NULL = none */
} gfx_denoiser_inputs;
/* The history the next gfx_denoise reprojects (device pointers into the denoiser, read-only; for tests and debugging), W*H each:
 *   lighting  float4  (demodulated lighting r, g, b, 0): stage 0's output with feedbackStage, the integrated lighting otherwise
 *   moments   float2  (luminance, luminance^2) after the temporal blend
 *   length    uint32  history length 1..255, 0 = background / no history
 *   guide     float4  (normal x, y, z, depth): depth is +inf for background and emissive pixels, 0 for a surface when no depth was given */
typedef struct gfx_denoiser_history_buffers {
    const void* lighting;
    const void* moments;
    const void* length;
    const void* guide;
} gfx_denoiser_history_buffers;
/* defaults of the reference (svgf.cu:5-27, svgf_main.cpp's UI defaults: 5 stages, Box3x3, feedback of the first stage) */
int gfx_denoiser_default_settings(gfx_denoiser_settings* out);
/* optixu::Denoiser prepare / setupState / computeNormalizer (restir_di_main.cpp:1400-1432): allocates everything; settings NULL =
 * defaults.  Invalid settings or a zero size return 1 (gfx_last_error(ctx)). */
int gfx_denoiser_create(gfx_ctx* ctx, uint32_t width, uint32_t height, const gfx_denoiser_settings* settings, gfx_denoiser** out);
int gfx_denoiser_destroy(gfx_denoiser* den);
/* optixu::Denoiser::invoke (restir_di_main.cpp:2504-2533, previousDenoisedBeauty -> the denoiser's own history): enqueues at most
 * numStages + 2 kernels on `stream`; no allocation, no synchronisation, no host work between the kernels.  isFirstFrame discards the
 * history (every history length restarts at 1).  dDenoisedFloat4 = float4[W*H].  A null required input or output, or a size other
 * than create's, returns 1 and launches nothing. */
int gfx_denoise(gfx_ctx* ctx, void* stream, gfx_denoiser* den, const gfx_denoiser_inputs* in, int isFirstFrame, void* dDenoisedFloat4);
int gfx_denoiser_history(gfx_denoiser* den, gfx_denoiser_history_buffers* out);

/* ---------------------------------------------------------------- temporal anti-aliasing ------ */

/* The TAA half of svgf/'s output pass, applyAlbedoModulationAndTemporalAntiAliasing (svgf/gpu_kernels/svgf.cu:533-611, launch
 * svgf_main.cpp:2170) with reprojectPreviousAccumulation (svgf.cu:465-531): reproject the previous final image through the flow,
 * clamp it to the current frame's 3x3 neighbourhood (the mean of the box and cross extrema), blend with an exponential moving
 * average of weight 1/historyLength (the taaHistoryLength slider 2^0..2^8, default 16: svgf_main.cpp:1736, :1798-1803, :1986).
 * Independent of the denoiser, as the reference's enableSVGF and enableTemporalAA are: run it on gfx_denoise's output or on the
 * linear beauty.  One deviation: a pixel whose previous position is off screen outputs the current colour (the reference drops its
 * off-screen flag and blends black clamped to the neighbourhood).  The order of operations is specified in
 * gfxexp_amd/csrc/denoise/taa.hip; the CPU restatement of tests/taa_ref.cpp follows the same text bit for bit. */
typedef struct gfx_taa gfx_taa;              /* opaque; owns its double-buffered history */
/* The flow gfx_taa_apply should reproject through, into a caller-owned float2[W*H], from the G-buffers of the current
 * gfx_restir_set_params: per pixel the current minus the previous raster position of the point the pixel sees.  For a surface
 * that is GBuffer1.motionVector less the pixel's jitter offset ((x + 0.5) minus the hit point's current raster position); for a
 * pixel without a surface, the motion of its view direction under the camera rotation (svgf.cu:443-449; restir_di's miss program
 * projects the direction as a point, optix_gbuffer_kernels.cu:205-221); 0 under resetFlowBuffer.  The motion vector itself, fed
 * to TAA under enableJittering, resamples the history at a random sub-pixel offset every frame.  It reads only
 * the G-buffers, so it follows whatever moved the surface: a plain instance under gfx_instance_set_transform and a displaced
 * instance under gfx_tfdm_set_move alike. */
int gfx_restir_copy_taa_flow_to_linear(gfx_ctx* ctx, void* stream, void* dLinearFlow);
typedef struct gfx_taa_inputs {
    uint32_t width, height;                  /* of both buffers; must equal gfx_taa_create's */
    const void* color;                       /* float4[W*H]: the current colour; alpha is copied to the output */
    const void* flow;                        /* float2[W*H]: pixel centre minus previous position, in pixels (as gfx_denoise reads it) */
} gfx_taa_inputs;
/* Allocates the history (zeroed).  historyLength 1..256; a zero size, a side above 16384 or a historyLength out of range returns 1. */
int gfx_taa_create(gfx_ctx* ctx, uint32_t width, uint32_t height, uint32_t historyLength, gfx_taa** out);
int gfx_taa_destroy(gfx_taa* taa);
/* The reference's live slider: takes effect from the next gfx_taa_apply.  0 or above 256 returns 1 and changes nothing. */
int gfx_taa_set_history_length(gfx_taa* taa, uint32_t historyLength);
/* Enqueues exactly one kernel on `stream`; no allocation, no synchronisation.  isFirstFrame ignores the history (out = color).
 * dOutFloat4 = float4[W*H]; its image also becomes the history of the next call.  A null input or output, a size other than
 * create's, dOutFloat4 == color (the pass reads neighbours: no in-place use) or dOutFloat4 == one of the object's own history
 * buffers returns 1, launches nothing and leaves the history as it was. */
int gfx_taa_apply(gfx_ctx* ctx, void* stream, gfx_taa* taa, const gfx_taa_inputs* in, int isFirstFrame, void* dOutFloat4);
/* Device pointer of the float4[W*H] history the next gfx_taa_apply reprojects (the last output; read-only; for tests). */
int gfx_taa_history(gfx_taa* taa, const void** dHistory);

/* ---------------------------------------------------------------- path tracing ---------------- */

/* The baseline path tracer (path_tracing/path_tracing_main.cpp:2068-2093: G-buffer pipeline, then
 * the pathTraceBaseline pipeline; kernels path_tracing/gpu_kernels/optix_pathtracing_kernels.cu:74-341:
 * NEE + BSDF sampling with power-heuristic MIS, Russian roulette, implicit light hits).
 * Parameters are the ones set by gfx_restir_set_params: path_tracing_shared.h:137-173 is the subset
 * {imageSize, rngBuffer, GBuffer0/1, beauty/albedo/normal accumulation, env light} of the static block
 * and {travHandle, numAccumFrames, camera, prevCamera, envLightPowerCoeff/Rotation, bufferIndex,
 * resetFlowBuffer, enableJittering, enableEnvLight} of the per-frame block; maxPathLength
 * (path_tracing_shared.h:165, 4-bit field, UI range 2..15, default 5 at path_tracing_main.cpp:1519)
 * is passed here.  Rows [rowBegin, rowEnd) as in gfx_restir_launch_rows; rowEnd == 0 -> whole frame.  Of the NRC passes
 * GFX_PT_PATH_TRACE_NRC and GFX_PT_NRC_ACCUMULATE are per pixel and honour the rows; the others run over tiles / records. */
enum gfx_pt_pass {
    GFX_PT_SETUP_GBUFFERS = 0,        /* path_tracing/gpu_kernels/optix_gbuffer_kernels.cu */
    GFX_PT_PATH_TRACE_BASELINE = 1,   /* optix_pathtracing_kernels.cu:298-341 (pathTraceBaseline RG/CH/MS) */
    /* ReGIR (regir/regir_main.cpp:2031-2066); need gfx_regir_set_params */
    GFX_PT_REGIR_BUILD_CELL_RESERVOIRS = 2,           /* regir/gpu_kernels/build_cell_reservoirs.cu:221-223 */
    GFX_PT_REGIR_BUILD_CELL_RESERVOIRS_TEMPORAL = 3,  /* :225-227 */
    GFX_PT_PATH_TRACE_REGIR = 4,                      /* regir/gpu_kernels/optix_pathtracing_kernels.cu:425-433 */
    GFX_PT_REGIR_UPDATE_LAST_ACCESS = 5,              /* build_cell_reservoirs.cu:229-243 */
    /* Neural radiance caching (neural_radiance_caching_main.cpp:2270-2370); need gfx_nrc_set_render_params.
     * The network calls between them are gfx_nrc_infer / gfx_nrc_train. */
    GFX_PT_NRC_PREPROCESS = 6,                        /* nrc_setup_kernels.cu:6-49 */
    GFX_PT_PATH_TRACE_NRC = 7,                        /* neural_radiance_caching/gpu_kernels/optix_pathtracing_kernels.cu:693-703 */
    GFX_PT_NRC_ACCUMULATE = 8,                        /* nrc_setup_kernels.cu:51-93 */
    GFX_PT_NRC_PROPAGATE = 9,                         /* :95-137 */
    GFX_PT_NRC_SHUFFLE = 10,                          /* :139-216 */
    GFX_PT_NRC_VISUALIZE_PREDICTION = 11,             /* optix_pathtracing_kernels.cu:705-778 */
    /* numInferenceQueries = (W * H + #tiles of tileSize[bufferIndex]) rounded up to 128 -- what the reference computes on the
     * host after a stream synchronisation and a device read (neural_radiance_caching_main.cpp:2293-2303) -- written to the
     * context's device word (gfx_nrc_query_count_ptr) for gfx_nrc_infer_indirect: the frame needs no host round trip. */
    GFX_PT_NRC_COUNT_QUERIES = 12,
    /* GFX_PT_PATH_TRACE_NRC with many-light next-event estimation: every path vertex draws its light sample from the ReGIR
     * grid cell under it (sampleFromCell, regir/gpu_kernels/optix_pathtracing_kernels.cu:18-82) instead of the emitter
     * distributions (neural_radiance_caching/gpu_kernels/optix_pathtracing_kernels.cu:38-63).  The combination is an open
     * item of the reference (README.md:80-81 "Combine with many-light sampling techniques like ReSTIR/ReGIR"), so its
     * definition is this build's: the ReGIR estimate has no evaluable density, hence no MIS -- NEE carries all direct light
     * at a path vertex and emitters found by BSDF sampling (path length >= 2, incl. the environment) contribute nothing;
     * Russian roulette, cache termination and the training records are those of the NRC tracer.  Needs gfx_regir_set_params
     * (grid built by GFX_PT_REGIR_BUILD_CELL_RESERVOIRS* before, GFX_PT_REGIR_UPDATE_LAST_ACCESS after) AND
     * gfx_nrc_set_render_params. */
    GFX_PT_PATH_TRACE_NRC_REGIR = 13,
    /* GFX_PT_PATH_TRACE_NRC whose FIRST path vertex takes its next-event estimation from the pixel's ReSTIR DI reservoir -- the other
     * half of the reference's open item (README.md:80-81 "... like ReSTIR/ReGIR"; NEE site neural_radiance_caching/gpu_kernels/
     * optix_pathtracing_kernels.cu:38-63), again a composition of two things the reference has: the frame first runs the original
     * ReSTIR DI passes (GFX_RESTIR_INITIAL_* and the spatial passes, restir_di_main.cpp:2365-2421, up to but excluding SHADING) on the
     * same G-buffers and per-pixel RNGs; this pass then adds, at the first vertex, recPDFEstimate x performDirectLighting of the
     * final reservoir sample at the G-buffer's shading point with its shadow ray (the direct term of the shading pass,
     * optix_restir_di_kernels.cu:574-606) in place of the tracer's own light sample, and draws no random numbers there.  The
     * reservoir estimates all direct light of that vertex and has no density, so what the first extension ray finds emitting (path
     * length 2: surface or environment) contributes nothing; deeper vertices keep the tracer's NEE + MIS.  The reservoirs are the
     * ones of `currentReservoirIndex` (gfx_restir_set_params).  Whole-frame renderers only. */
    GFX_PT_PATH_TRACE_NRC_RESTIR = 14
};

/* The ReGIR members of regir/regir_shared.h:200-263 (grid of cells x 512 light slots).  Light-slot
 * reservoirs use the three-plane layout of the pixel reservoirs: plane k of buffer b at
 * reservoirs[b] + 16 * (k * numLightSlots + slot), numLightSlots = cells * 512.
 * lightSlotRngs are seeded row-major from mt19937_64(591842031321323413) (regir_main.cpp:1086-1092),
 * lastAccessFrameIndices start at 0xFFFFFFFF (regir_main.cpp:1096, 1112: fill(-1)).
 * The build passes read frame.frameIndex and frame.bufferIndex. */
typedef struct gfx_regir_params {
    void* reservoirs[2];
    void* reservoirInfos[2];         /* gfx_reservoir_info[numLightSlots] */
    void* lightSlotRngs;             /* uint64_t[numLightSlots] */
    void* perCellNumAccesses;        /* uint32_t[numCells] */
    void* lastAccessFrameIndices;    /* uint32_t[numCells] */
    void* numActiveCells[2];         /* uint32_t each (statistics) */
    float gridOrigin[3];
    float gridCellSize[3];
    uint32_t gridDimension[3];       /* 32 x 8 x 32 in the reference (regir_main.cpp:1112) */
    uint32_t log2NumCandidatesPerLightSlot;   /* 3 (regir_main.cpp:1733) */
    uint32_t log2NumCandidatesPerCell;        /* 2 (:1734) */
    uint32_t enableCellRandomization;         /* 1 (:1736) */
} gfx_regir_params;
int gfx_regir_set_params(gfx_ctx* ctx, const gfx_regir_params* p);
int gfx_pt_launch(gfx_ctx* ctx, void* stream, int pass, uint32_t width, uint32_t height,
                  uint32_t maxPathLength, uint32_t rowBegin, uint32_t rowEnd);

/* NRC render-side state: the NRC members of neural_radiance_caching_shared.h:229-265 (+ radianceScale of
 * the per-frame block, :277, and the three arguments of preprocessNRC, nrc_setup_kernels.cu:6-9).
 *   RadianceQuery              14 floats = one column of the network input (:118-137)
 *   TerminalInfo               float3 alpha + u32 {hasQuery:1, pathLength:8, isTrainingPixel:1, isUnbiasedTile:1}
 *   TrainingVertexInfo         float3 localThroughput + u32 {prevVertexDataIndex:23, pathLength:8}
 *   TrainingSuffixTerminalInfo u32 {prevVertexDataIndex:23, hasQuery:1, pathLength:8}
 *   dataShuffler               u32 LCG state; entry i = state after i + 1 steps from 471313181
 *                              (neural_radiance_caching_main.cpp:1186-1194)
 * numPixels = W*H; maxNumTrainingSuffixes = W*H/16 (:1150); train buffers hold 131072 records (:9). */
typedef struct gfx_nrc_params {
    float sceneAabbMin[3], sceneAabbMax[3];
    uint32_t maxNumTrainingSuffixes;
    void* numTrainingData[2];            /* uint32_t */
    void* tileSize[2];                   /* uint32_t[2], initialised to 8 x 8 */
    void* targetMinMax[2];               /* int32_t[6] ordered-int min rgb, max rgb */
    void* targetAvg[2];                  /* float[3] */
    void* offsetToSelectUnbiasedTile;    /* uint32_t */
    void* offsetToSelectTrainingPath;    /* uint32_t */
    void* inferenceRadianceQueryBuffer;  /* 56 B x (numPixels + maxNumTrainingSuffixes, rounded up to 256) */
    void* inferenceTerminalInfoBuffer;   /* 16 B x numPixels */
    void* inferredRadianceBuffer;        /* float3 x (numPixels + maxNumTrainingSuffixes, rounded up to 256) */
    void* perFrameContributionBuffer;    /* float3 x numPixels */
    void* trainRadianceQueryBuffer[2];   /* 56 B x 131072 */
    void* trainTargetBuffer[2];          /* float3 x 131072 */
    void* trainVertexInfoBuffer;         /* 16 B x 131072 */
    void* trainSuffixTerminalInfoBuffer; /* uint32_t x maxNumTrainingSuffixes */
    void* dataShufflerBuffer;            /* uint32_t x 65536 */
    float radianceScale;
    uint32_t preprocessOffsetToSelectUnbiasedTile;   /* perFrameRng() draws, :2276-2277 (mt19937(72139121)) */
    uint32_t preprocessOffsetToSelectTrainingPath;
    uint32_t isNewSequence;
} gfx_nrc_params;
int gfx_nrc_set_render_params(gfx_ctx* ctx, const gfx_nrc_params* p);

/* ---------------------------------------------------------------- neural radiance cache -------- */

/* NeuralRadianceCache (neural_radiance_caching/network_interface.h:14-28): the tiny-cuda-nn network of
 * network_interface.cu:48-132 -- Composite{HashGrid | TriangleWave (3 dims), OneBlob 4 bins (5 dims),
 * Identity (6 dims)} -> fully fused MLP, 64 neurons, numHiddenLayers (2 or 5), ReLU; loss
 * RelativeL2Luminance; optimizer EMA(0.99) o Adam(lr, 0.9, 0.99, l2_reg 1e-6).  Here: bf16 MFMA,
 * fp32 accumulation and fp32 master parameters.
 *   gfx_nrc_create    = initialize(posEnc, numHiddenLayers, learningRate)      network_interface.cu:48-132
 *   gfx_nrc_destroy   = finalize()                                            :134-139
 *   gfx_nrc_infer     = infer(stream, inputData, numData, predictionData)     :141-147
 *   gfx_nrc_train     = train(stream, inputData, targetData, numData, lossOnCPU)   :149-157
 * inputData: device fp32 [14, numData] column-major (RadianceQuery, neural_radiance_caching_shared.h:118-127),
 * predictionData / targetData: device fp32 [3, numData]; numData must be a multiple of 128 (:143, :151).
 * Parameter blob (fp32): W0 [64][64], W1.. [64][64] x (numHiddenLayers - 1), Wout [16][64] (rows >= 3
 * unused), then the hash grid (level tables back to back, 2 features per entry); W[out][in] with `in`
 * in the canonical feature order [position | one-blob 4 x 5 | identity 6 | ones].
 * get_params which: 0 training weights, 1 EMA (inference) weights, 2 Adam first moment, 3 second moment. */
enum gfx_nrc_position_encoding { GFX_NRC_TRIANGLE_WAVE = 0, GFX_NRC_HASH_GRID = 1 };   /* network_interface.h:5-8 */
int gfx_nrc_create(gfx_ctx* ctx, int positionEncoding, uint32_t numHiddenLayers, float learningRate, uint64_t* outHandle);
int gfx_nrc_destroy(gfx_ctx* ctx, uint64_t handle);
int gfx_nrc_infer(gfx_ctx* ctx, void* stream, uint64_t handle, const void* dInputData, uint32_t numData, void* dPredictionData);
int gfx_nrc_train(gfx_ctx* ctx, void* stream, uint64_t handle, const void* dInputData, const void* dTargetData,
                  uint32_t numData, float* lossOnCPU);
/* gfx_nrc_infer with the batch size read on the device: *dNumData queries (a multiple of 128, <= maxNumData) are inferred;
 * the launch is sized for maxNumData.  dNumData = gfx_nrc_query_count_ptr after GFX_PT_NRC_COUNT_QUERIES in the NRC frame. */
int gfx_nrc_infer_indirect(gfx_ctx* ctx, void* stream, uint64_t handle, const void* dInputData, const void* dNumData, uint32_t maxNumData,
                           void* dPredictionData);
int gfx_nrc_query_count_ptr(gfx_ctx* ctx, void** dNumData);
int gfx_nrc_num_params(gfx_ctx* ctx, uint64_t handle, uint32_t* outCount);
int gfx_nrc_set_params(gfx_ctx* ctx, uint64_t handle, const float* hostParams, uint32_t count);
int gfx_nrc_get_params(gfx_ctx* ctx, uint64_t handle, int which, float* hostOut, uint32_t count);
/* The device images gfx_nrc_infer reads: which = 0 the packed bf16 MLP fragments, 1 the packed bf16 hash grid (null / 0 for
 * the triangle-wave encoding).  They are brought up to date with the trained (EMA) weights when somebody asks -- this call, its _async
 * form, gfx_nrc_infer -- not after every training step (a frame trains four steps and infers once); whoever packs them first waits, on its
 * stream, for an event gfx_nrc_train records behind its optimizer, so no ordering between the caller's streams is assumed and no stream
 * handle of an earlier call is kept.  gfx_nrc_inference_image has no stream to order with: it packs on a library-owned stream and
 * returns when the images are complete (a host wait for the last training step if the images were stale).  The pointers stay valid for the
 * network's lifetime, the CONTENTS are rewritten by the next refresh after a training step -- a caller that caches the pointers must
 * order its reads before that (e.g. call one of these functions again after training).
 * gfx_nrc_inference_image_async: the same, packed on `stream`; the caller uses the images in `stream` order, no host wait.
 * A process that does not train (a band renderer other than rank 0, gfxh_nrc_set_exchange) receives these bytes from the one that does. */
int gfx_nrc_inference_image(gfx_ctx* ctx, uint64_t handle, int which, void** dPtr, uint64_t* bytes);
int gfx_nrc_inference_image_async(gfx_ctx* ctx, void* stream, uint64_t handle, int which, void** dPtr, uint64_t* bytes);
/* A 32-bit checksum of both inference images (position-weighted word sum, packed on `stream` first if stale) ADDED to the device word
 * *dOutU32: processes that each train a copy of the network on the same batches (the band-split NRC renderer) compare it to notice a
 * copy that has drifted (gfxexp_host.h gfxh_nrc_set_exchange). */
int gfx_nrc_params_checksum(gfx_ctx* ctx, void* stream, uint64_t handle, void* dOutU32);

/* Blocking device-to-host copy of library- or caller-owned device memory (TypedBuffer::read,
 * utils/cuda_util.h; used for pick info at restir_di_main.cpp:2010). */
int gfx_read_device(gfx_ctx* ctx, const void* dSrc, void* hostDst, size_t bytes);

/* Per-kernel HIP-event timing of the launches issued since the last reset
 * (cudau::Timer, utils/cuda_util.h:441-485).  names/ms arrays sized by capacity. */
int gfx_timing_enable(gfx_ctx* ctx, int enable);
int gfx_timing_collect(gfx_ctx* ctx, char names[][48], float* totalMs, uint32_t* calls,
                       uint32_t capacity, uint32_t* n);
/* Scheduling knobs of a context; none changes a result (no reference counterpart: OptiX schedules in the driver).
 *   "pixel_map" 0|1|2           which pixels share a wave / block / XCD in the per-pixel kernels: scan lines, 8 x 8 tiles
 *                               (the tiling of restir_di/gpu_kernels/per_pixel_ris.cu:44-61), tiles + XCD-aware supertiles (default)
 *   "super_x", "super_y"        log2 of the supertile size in 16 x 16-pixel blocks (mode 2; default 2, 2)
 *   "trace_blocks_per_cu", "trace_refill", "trace_batch"   persistent traversal grid, lane-refill threshold, rays per ticket
 *   "temporal_hints" 0|1        the primary ray of a pixel first tests the triangle it hit one frame ago (default 1; GFX_TEMPORAL_HINTS)
 *   "pt_overlap" 0|1            path tracers (gfx_pt_launch): the NEE any-hit trace of a bounce and the kernel that applies it run on a
 *                               library-owned second stream underneath the extension closest-hit trace of the same bounce -- the two
 *                               read and write disjoint buffers; the bounce kernel waits for both (default 1; GFX_PT_OVERLAP)
 *   "fuse_passes" 0|1|2         ray passes as ONE kernel each -- the thread that makes a ray traces it and consumes the result
 *                               (csrc/trace_local.hip.h) -- instead of producer kernel, k_trace launch, consumer kernel.  0 (default): the
 *                               G-buffer pass (GFX_RESTIR_SETUP_GBUFFERS, GFX_PT_SETUP_GBUFFERS) at every size; GFX_RESTIR_INITIAL_*, _SHADING
 *                               and _SPATIAL_BIASED_AND_SHADING for launches of up to about half a full-HD frame (a row band of a multi-GPU
 *                               frame); GFX_PT_PATH_TRACE_BASELINE / _REGIR (the whole path of a pixel in one kernel) for launches of about
 *                               one round of waves (512 x 512).  1 never, 2 always (GFX_FUSE_PASSES).  Counting launches
 *                               (gfx_counters_enable) always take the k_trace form.
 *   "block_order" 0|1           fused GFX_RESTIR_INITIAL_* / _SHADING kernels whose launch is several rounds of blocks start their blocks by
 *                               decreasing cost (traversal steps of the block's longest ray) of the same launch one frame ago instead of in
 *                               index order: the launch ends when its last tracing wave does (default 1; GFX_BLOCK_ORDER)
 *   "candidate_split" 0|1|2|4   lanes per pixel in the candidate loop of the initial-RIS passes (GFX_RESTIR_INITIAL_*): the lanes take the
 *                               pixel's candidates round robin and the reservoir is formed as the sequential loop forms it; 0 (default)
 *                               = by launch size: 4 when the launch fills the GPU's wave slots at most ~1.5 times (a row band of an
 *                               8-way split frame), else 1 (GFX_CANDIDATE_SPLIT)
 *   "candidate_prefilter" 0|1   candidate loop with one lane per pixel as a kernel of its own (a full frame): 1 (default) walks the
 *                               candidates twice -- first a conservative test on a 16-byte bound per emitter record (csrc/emitter_cull.h)
 *                               that proves about four candidates in five to have a weight of exactly zero, then the full candidate for
 *                               the rest only; 0 evaluates every candidate in lockstep.  Same reservoirs, same random streams.
 *   "nrc_staged_infer" 0|1|2    gfx_nrc_infer with the hash-grid encoding: 0 (default) a batch that gives every CU at least one pass of 3 072 queries is
 *                               encoded level by level out of LDS copies of the level tables (one persistent block per CU; same predictions bit for
 *                               bit), smaller batches gather from the tables in place; 1 never, 2 always (GFX_NRC_STAGED_INFER)
 * The same knobs are read once from the environment by gfx_ctx_create (GFX_PIXEL_MAP, GFX_SUPER_X, GFX_SUPER_Y,
 * GFX_TRACE_BLOCKS_PER_CU, GFX_TRACE_REFILL, GFX_TRACE_BATCH). */
int gfx_tunable_set(gfx_ctx* ctx, const char* name, int value);
/* Ray-traversal counters accumulated by the renderer passes: {node fetches, triangle fetches, rays (queue entries with an empty
 * interval are not counted), stack spills}
 * of the any-hit launches in [0..3] and of the closest-hit launches in [4..7]. */
int gfx_counters_enable(gfx_ctx* ctx, int enable);
int gfx_counters_read(gfx_ctx* ctx, uint64_t counters[8], int reset);
/* Scheduling diagnostics of the counting trace launches: [0] wave iterations, [1] lanes that held an
 * item summed over iterations, [2] / [3] the same after the ray queue ran dry (drain phase), [4] clock cycles summed over
 * the waves, of which [5] in the ray refill (ticket, ray loads, setup), [6] waiting for the item fetch, [7] processing
 * items (the rest: item selection, loop overhead). */
int gfx_trace_diag_read(gfx_ctx* ctx, uint64_t diag[8], int reset);
/* The one-kernel path tracers (k_pt_fused, k_pt_regen) with the tunable "pt_diag" set: [0] bounce iterations summed over the waves, [1] lanes
 * that held a ray in them, [2] traversal steps, [3] waves, [4] refills (k_pt_regen). */
int gfx_pt_diag_read(gfx_ctx* ctx, uint64_t diag[8], int reset);
/* Measurement utility ("measure peak with a streaming-copy microbenchmark on the box, don't quote the datasheet"): copies
 * `bytes` (a multiple of 16; both pointers 16-byte aligned, device memory) with 16-byte non-temporal loads and stores per lane, on
 * `stream`; dDst == NULL makes it a read-only pass over dSrc.  bench.py times both with HIP events for roofline.peak_measured /
 * peak_measured_read_only; no renderer calls it. */
int gfx_stream_copy(gfx_ctx* ctx, void* dDst, const void* dSrc, size_t bytes, void* stream);
/* Measurement utility: the expansion gfx_texture_set_bc slots go through at scene upload, on caller-owned device memory and on
 * `stream`: dBlocks (16-byte aligned) -> dTexels (16-byte aligned, width * height texels of the 8-bit `format`, rows tightly
 * packed).  tools/bench_bc_expand.py times it with HIP events; no renderer calls it. */
int gfx_bc_expand(gfx_ctx* ctx, void* stream, uint32_t bcFormat, const void* dBlocks, uint32_t width, uint32_t height, uint32_t format, void* dTexels);

/* ---------------------------------------------------------------- tessellation-free displacement mapping (TFDM) ----------
 * A height map displaces a base triangle mesh along its interpolated vertex normals; rays are intersected with the displaced
 * surface without building its micro-triangles, by descending a min-max pyramid of the map with affine-arithmetic bounds
 * (the reference's tfdm/ program).  The query stands next to gfx_trace: rays are given in the object
 * space of the base mesh, in gfx_trace's layout (origin | tmin, direction | tmax), and a ray's tmax lets the caller chain
 * the query behind gfx_trace for a scene that mixes plain and displaced geometry: trace the plain geometry first, hand its
 * hit distance in as tmax, and a displaced hit that comes back is the closer one.  gfx_trace_scene below does that chain in
 * one call, for any number of displaced instances under their own transforms; gfx_scene_bind_displaced at the end of this
 * section makes the G-buffer pass and the baseline path tracer render them. */
typedef struct gfx_tfdm gfx_tfdm;                       /* opaque; owns heights, pyramid, records, AABBs, tree */
/* How a texel of the target level is intersected (the modes of LocalIntersectionType, tfdm/tfdm_shared.h; the values are this
 * library's own): its bounding box, two flat triangles over its four corners, or -- 4 -- the displaced surface itself,
 * S(u, v) = P(u, v) + h(u, v) N(u, v) / |N(u, v)| with h bilinear over the texel's corner heights, by Newton's iteration (the
 * reference's Bilinear).  Only this last mode has a normal that is continuous inside a texel.  2 and 3
 * are refused (the reference's BSpline is not implemented there either). */
enum gfx_tfdm_local { GFX_TFDM_BOX = 0, GFX_TFDM_TWO_TRIANGLE = 1, GFX_TFDM_BILINEAR = 4 };
/* DisplacementParameters, tfdm/tfdm_shared.h, with the texture transform as the scale / rotation (degrees) / offset it is made
 * from (tfdm_main.cpp:2580-2588).  The height of a map value h is hOffset + preScale * hScale * (h - hBias) with preScale =
 * 1 / sqrt(texScale[0] * texScale[1]) (tfdm_intersection_kernels.h:54-59).  targetMipLevel: the map level whose texels are
 * intersected (0 = the finest).  A transformed texture coordinate times the map's size must stay below 2^24 in magnitude (texel
 * indices are exact as floats up to there); gfx_tfdm_create and gfx_tfdm_set_params refuse anything beyond, a texOffset of 3e5
 * for example -- reduce it modulo 1. */
typedef struct gfx_tfdm_params { float hOffset, hScale, hBias; float texScale[2], texRotation, texOffset[2];
                                 uint32_t targetMipLevel, localIntersection; } gfx_tfdm_params;
/* closest-hit record of gfx_tfdm_trace (DisplacedSurfaceAttributes + the hit kind, tfdm_intersection_kernels.h:537-561), 32 B.
 * bcB / bcC are barycentrics on the BASE triangle primIndex; normal is the unit normal of the displaced surface in object space:
 * of the box face or the flat triangle that was hit, or with GFX_TFDM_BILINEAR the normal of the smooth surface at the hit.
 * Miss: dist = the ray's tmax, primIndex = GFX_INVALID_SLOT, the rest zero. */
typedef struct gfx_tfdm_hit { float dist, bcB, bcC; uint32_t primIndex; float normal[3]; uint32_t frontFace; } gfx_tfdm_hit;
/* hOffset 0, hScale 1, hBias 0, unit texture transform, level 0, two triangles per texel. */
int gfx_tfdm_default_params(gfx_tfdm_params* out);
/* tfdm_main.cpp:2218-2255 (the height sampler and its mips), :2492-2545 (the pyramid launches and computeAABBs), :780-843 (the
 * per-triangle matrices).  vertices / triangles are host arrays as for gfx_geom_create (stride >= sizeof(gfx_vertex); position,
 * normal and texCoord are used); heightLevels are host arrays of fp32 heights in [0, 1], level k of (size >> k)^2 texels, rows
 * tightly packed.  numLevels is 1 (the library makes the coarser levels by the 2 x 2 mean ((a + b) + (c + d)) * 0.25f) or
 * log2(size) + 1.  The map is square and `size` a power of two up to 8192, as the reference demands (tfdm_main.cpp:2236-2239);
 * 1 <= numTriangles <= 2^20.  Anything else is refused with a message. */
int gfx_tfdm_create(gfx_ctx* ctx, void* stream, const void* vertices, uint32_t stride, uint32_t numVertices,
                    const uint32_t* triangles, uint32_t numTriangles,
                    const float* const* heightLevels, uint32_t numLevels, uint32_t size,
                    const gfx_tfdm_params* params, gfx_tfdm** out);
/* New parameters for an object (the GUI edits of tfdm_main.cpp:2576-2600): records, AABBs and the tree are made again, the
 * pyramid is kept.  localIntersection may change between all three modes (records, boxes and the tree do not depend on it).  A
 * refused call leaves the object as it was. */
int gfx_tfdm_set_params(gfx_ctx* ctx, void* stream, gfx_tfdm* obj, const gfx_tfdm_params* params);
/* New heights for the level-0 rectangle (x0, y0) .. (x0 + w, y0 + h) of an object's map, in place.  dSrc is
 * DEVICE memory on the object's device, 4-byte aligned: dSrc[j * srcPitch + i] is the new fp32 height of texel (x0 + i, y0 + j),
 * 0 <= i < w, 0 <= j < h.  The rectangle lies inside the map and does not wrap.  Afterwards every level of HEIGHTS and PYRAMID, AABBS
 * and RECORDS are, bit for bit, what gfx_tfdm_create with the whole new map and the same parameters makes; NODES keeps its shape
 * (node count, every first / count) with a leaf's box its primitive's new box and an inner node's box the exact union of its two
 * children's.  No micro-geometry exists to be rebuilt: only the texels above the rectangle, the per-triangle boxes and the boxes
 * of the tree are computed again, all of it on the device.  Everything runs on `stream` and the call returns after the work is
 * done (it ends with a read-back of the new root node); the order against traces of the same object on OTHER streams is the
 * caller's business.  A member of an instance set whose object was updated is stale as after gfx_tfdm_set_params: commit the set
 * again (the instance's world box comes from the new root).  A displaced pixel's motion vector stays the instance's curToPrev: a
 * change of height carries no motion.  Refused with a message, before anything of the object is written, so that the object
 * answers as before: a null or misaligned dSrc; w or h of 0; srcPitch < w; a rectangle that leaves the map; an object created
 * with its own mip levels (numLevels > 1: its coarser levels are not means, a regenerated region would mix two definitions); a
 * source value that is not finite. */
int gfx_tfdm_update_heights(gfx_ctx* ctx, void* stream, gfx_tfdm* obj, const float* dSrc, uint32_t srcPitch,
                            uint32_t x0, uint32_t y0, uint32_t w, uint32_t h);
int gfx_tfdm_destroy(gfx_tfdm* obj);
/* One ray per entry, optixTrace against the custom-primitive GAS of the reference (tfdm_intersection_kernels.h:16-35 for the
 * per-triangle boxes, :39-562 for the surface).  mode GFX_TRACE_CLOSEST: dOut = gfx_tfdm_hit[numRays]; GFX_TRACE_ANY: dOut =
 * uint32_t[numRays] (1 = occluded).  Closest-hit ties on the distance go to the lower primitive index, and a hit
 * counts only from where the ray enters its base triangle's box (less a rounding slack) on, so the answer does not depend on the tree
 * (DESIGN.md section 25).  dCounters (optional,
 * device u64[4], added to): texel AABB tests, leaf (local intersection) tests, rays, base triangles tested -- the reference's
 * TraversalStats (tfdm_shared.h) and one more.  dRayOrgTmin, dRayDirTmax and a closest-hit dOut must be 16-byte aligned (they
 * are read and written as float4), an any-hit dOut 4-byte, dCounters 8-byte; a misaligned pointer is refused. */
int gfx_tfdm_trace(gfx_ctx* ctx, void* stream, gfx_tfdm* obj, int mode, const void* dRayOrgTmin, const void* dRayDirTmax,
                   uint32_t numRays, void* dOut, void* dCounters);
/* Inspection.  PYRAMID: level `level` as (min, max) float pairs, (size >> level)^2 of them; HEIGHTS: that level of the height
 * map; AABBS: six floats (min, max) per triangle; RECORDS: the 192-byte per-triangle records; NODES: the 32-byte tree nodes
 * (csrc/tfdm/tfdm_core.hip.h).  `bytes` must be the exact size (gfx_tfdm_size). */
enum gfx_tfdm_read_what { GFX_TFDM_READ_PYRAMID = 0, GFX_TFDM_READ_AABBS = 1, GFX_TFDM_READ_RECORDS = 2, GFX_TFDM_READ_NODES = 3, GFX_TFDM_READ_HEIGHTS = 4 };
int gfx_tfdm_read(gfx_ctx* ctx, gfx_tfdm* obj, int what, uint32_t level, void* hostOut, size_t bytes);
/* Size in bytes of what gfx_tfdm_read(what, level) returns; with what = -1 the device bytes the object owns in all. */
int gfx_tfdm_size(gfx_ctx* ctx, gfx_tfdm* obj, int what, uint32_t level, size_t* bytes);

/* ---------------------------------------------------------------- crack-free displacement mapping (NRTDSM) ----------------
 * A second ray query on a displaced base mesh (the reference's nrtdsm/ program, displacement mapping only; DESIGN.md section
 * 20).  The surface is S(alpha, beta) = P + (hOffset - s hBias + s h(tc)) N with s = hScale / sqrt(texScale[0] texScale[1]),
 * P, tc and N the barycentric interpolations of the vertices, N NOT renormalised, h affine over each half texel (split along
 * the TL-BR diagonal): two base triangles that share the two vertices of an edge (position, normal and texture coordinate)
 * share the surface above it, which gfx_tfdm_* does not promise.  Parameters, hit record, counters, ray layout, alignment and
 * the items of read / size are those of gfx_tfdm_*; GFX_TFDM_READ_RECORDS gives the 144-byte records of
 * csrc/nrtdsm/nrtdsm_core.hip.h.  The hit's normal is the unit normal of the curved micro-patch at the hit, on the side of
 * growing height.  create and set_params refuse, with a message and without launching anything: targetMipLevel != 0; a
 * localIntersection other than GFX_TFDM_TWO_TRIANGLE; a map value outside [0, 1] at any level; parameters that are not finite or a
 * texScale that is not positive; a texture coordinate that reaches 2^24 texels.  After a refused set_params the object is as before.
 * A ray that is not finite or has a zero direction misses. */
typedef struct gfx_nrtdsm gfx_nrtdsm;                   /* opaque; owns heights, pyramid, records, AABBs, tree */
int gfx_nrtdsm_create(gfx_ctx* ctx, void* stream, const void* vertices, uint32_t stride, uint32_t numVertices,
                      const uint32_t* triangles, uint32_t numTriangles,
                      const float* const* heightLevels, uint32_t numLevels, uint32_t size,
                      const gfx_tfdm_params* params, gfx_nrtdsm** out);
int gfx_nrtdsm_set_params(gfx_ctx* ctx, void* stream, gfx_nrtdsm* obj, const gfx_tfdm_params* params);
/* As gfx_tfdm_update_heights, with the same stream behaviour (synchronous on `stream`; ordering against traces on other streams
 * is the caller's), the same staleness of set members and no motion; also refuses a source value outside [0, 1], as create does. */
int gfx_nrtdsm_update_heights(gfx_ctx* ctx, void* stream, gfx_nrtdsm* obj, const float* dSrc, uint32_t srcPitch,
                              uint32_t x0, uint32_t y0, uint32_t w, uint32_t h);
int gfx_nrtdsm_destroy(gfx_nrtdsm* obj);
int gfx_nrtdsm_trace(gfx_ctx* ctx, void* stream, gfx_nrtdsm* obj, int mode, const void* dRayOrgTmin, const void* dRayDirTmax,
                     uint32_t numRays, void* dOut, void* dCounters);
int gfx_nrtdsm_read(gfx_ctx* ctx, gfx_nrtdsm* obj, int what, uint32_t level, void* hostOut, size_t bytes);
int gfx_nrtdsm_size(gfx_ctx* ctx, gfx_nrtdsm* obj, int what, uint32_t level, size_t* bytes);

/* ---------------------------------------------------------------- shell mapping (the other half of NRTDSM) ----------------
 * A third ray query on a base mesh.  A small triangle mesh, the shell mesh, is authored once in the tile
 * [0, 1]^2 x [hLo, hHi] of shell space (u, v, h) and repeated over the base mesh like a texture: tile (i, j), for any integers,
 * holds a copy shifted by (i, j, 0).  A shell-space point lies at S = P + (hOffset - s hBias + s h) N with s, P and N as for
 * gfx_nrtdsm_* and (u, v) the base mesh's texture coordinates after the texture transform.  Nothing is instantiated: the object
 * owns one BVH over the shell mesh (32-byte nodes, 48-byte triangles) and 144 bytes, a box and two tree nodes per base triangle.
 * positions of a gfx_shell_geom are (u, v, h) floats `stride` bytes apart; up to 8 geometries, 2^20 triangles in all.
 * create and set_geometry refuse, with a message and leaving an existing object unchanged: no triangles or more than 2^20; more
 * than 8 geometries; a vertex that is not finite or has u or v outside [0, 1]; an index beyond numVertices.  A flat shell mesh
 * (every h equal, 0 included) is a decal and is accepted.  params: targetMipLevel and localIntersection must be 0; the other
 * refusals are gfx_nrtdsm_*'s, with 2^22 tiles in place of 2^24 texels.  params == NULL: hOffset 0, hScale 1, hBias 0, unit
 * texture transform. */
typedef struct gfx_shell gfx_shell;                     /* opaque; owns records, AABBs, the base tree, shell nodes and triangles */
typedef struct gfx_shell_geom { const float* positions; uint32_t stride, numVertices; const uint32_t* triangles; uint32_t numTriangles; } gfx_shell_geom;
/* closest-hit record of gfx_shell_trace, 48 B.  The first 32 bytes are a gfx_tfdm_hit: bcB / bcC are barycentrics on the BASE
 * triangle primIndex; normal is the unit object-space normal of the mapped shell triangle at the hit, on the side its winding
 * faces in shell space ((u, v, h) right-handed) whatever the base triangle's parametrisation; frontFace = dot(dir, normal) < 0.
 * shellTriangle indexes the concatenation of the geometries in the order given, shellGeom is its geometry, tile the copy that
 * was hit.  Miss: as gfx_tfdm_hit, the new fields zero. */
typedef struct gfx_shell_hit { float dist, bcB, bcC; uint32_t primIndex; float normal[3]; uint32_t frontFace;
                               uint32_t shellTriangle, shellGeom; int32_t tile[2]; } gfx_shell_hit;
int gfx_shell_create(gfx_ctx* ctx, void* stream, const void* vertices, uint32_t stride, uint32_t numVertices,
                     const uint32_t* triangles, uint32_t numTriangles, const gfx_shell_geom* geoms, uint32_t numGeoms,
                     const gfx_tfdm_params* params, gfx_shell** out);
int gfx_shell_set_params(gfx_ctx* ctx, void* stream, gfx_shell* obj, const gfx_tfdm_params* params);
/* Another shell mesh over the same base mesh and parameters.  A refused call leaves the object as it was. */
int gfx_shell_set_geometry(gfx_ctx* ctx, void* stream, gfx_shell* obj, const gfx_shell_geom* geoms, uint32_t numGeoms);
int gfx_shell_destroy(gfx_shell* obj);
/* As gfx_nrtdsm_trace; GFX_TRACE_CLOSEST: dOut = gfx_shell_hit[numRays], 16-byte aligned.  The counters: box tests (squares of
 * tiles and shell nodes), leaf tests (shell triangles), rays, base triangles tested. */
int gfx_shell_trace(gfx_ctx* ctx, void* stream, gfx_shell* obj, int mode, const void* dRayOrgTmin, const void* dRayDirTmax,
                    uint32_t numRays, void* dOut, void* dCounters);
/* Inspection: GFX_TFDM_READ_AABBS, _RECORDS (144 bytes each, csrc/nrtdsm/nrtdsm_core.hip.h; the root fields are tiles) and _NODES
 * (the tree over the base triangles' boxes) as for gfx_nrtdsm_read, and the shell BVH's 32-byte nodes and 48-byte triangles
 * (csrc/nrtdsm/shell_core.hip.h).  what = -1 in gfx_shell_size: the device bytes the object owns in all. */
enum gfx_shell_read_what { GFX_SHELL_READ_SHELL_NODES = 5, GFX_SHELL_READ_SHELL_TRIANGLES = 6 };
int gfx_shell_read(gfx_ctx* ctx, gfx_shell* obj, int what, void* hostOut, size_t bytes);
int gfx_shell_size(gfx_ctx* ctx, gfx_shell* obj, int what, size_t* bytes);

/* ---------------------------------------------------------------- plain and displaced instances in one query -------------
 * A set of displaced instances: gfx_tfdm objects under object-to-world transforms (row-major 3 x 4, as
 * gfx_instance_set_transform takes them), at most 1024.  One object may be added many times; objects and the context must
 * outlive the set.  gfx_tfdm_set_commit derives one 192-byte record per instance (csrc/tfdm/tfdm_instance.hip.h
 * InstanceRecord: both matrices, the padded world box, the object's device pointers and parameters, userId) and uploads the
 * table; a transform that is not finite or is singular is refused there and the committed table stays.  gfx_tfdm_set_params
 * on a member gives the object new device buffers, so the set must be committed again before the next query.  Errors of the
 * functions without a context argument are reported through the context the set was created on (gfx_last_error).
 * Motion.  Every instance has a current and a previous transform; gfx_tfdm_set_add sets both.
 *   gfx_tfdm_set_move       previous <- the instance's transform at the call, current <- objToWorld: InstanceController::update, what
 *                           gfx_instance_set_transform is for a plain instance.  Call it once per frame per moving instance: two
 *                           moves between two commits lose the first position, as for plain instances.
 *   gfx_tfdm_set_transform  the teleport: previous <- current <- objToWorld, no motion.
 * gfx_tfdm_set_commit derives a second table from the pair, one 48-byte curToPrev per instance (row-major 3 x 4): previous *
 * inverse(current), computed in double from the float entries and rounded to float once; the exact identity where the two are
 * equal bit for bit.  The G-buffer pass of a binding takes a displaced pixel's previous position through it.  Both tables are
 * swapped in together and only when every instance worked: a refused commit leaves both committed tables in force.  An instance
 * keeps its motion until the next move or teleport, as a plain instance does. */
typedef struct gfx_tfdm_set gfx_tfdm_set;
int gfx_tfdm_set_create(gfx_ctx* ctx, gfx_tfdm_set** out);
int gfx_tfdm_set_add(gfx_tfdm_set* set, gfx_tfdm* obj, const float objToWorld[12], uint32_t userId, uint32_t* index);
/* A gfx_nrtdsm object as a member of the set, next to gfx_tfdm members in any order: the same rules as
 * gfx_tfdm_set_add (a null object, an object of another device and a 1025th member are refused), and *index counts all members in
 * add order, whatever their kind.  Transform, move, commit, both reads and gfx_trace_scene treat it as any member; gfx_nrtdsm_set_params
 * on it asks for a new commit as gfx_tfdm_set_params does.  The kind of a member is the word after boxHi of its record.  Such a set is
 * rendered through gfx_scene_bind_displaced_kinds; gfx_scene_bind_displaced and gfx_scene_bind_displaced_passes
 * refuse it (by them it is traced but not rendered). */
#define GFX_INSTANCE_TFDM 0u
#define GFX_INSTANCE_NRTDSM 1u
int gfx_tfdm_set_add_nrtdsm(gfx_tfdm_set* set, gfx_nrtdsm* obj, const float objToWorld[12], uint32_t userId, uint32_t* index);
/* A gfx_shell object as a member of the set, under the rules of gfx_tfdm_set_add_nrtdsm: the same refusals,
 * *index counts all members in add order whatever their kind, and transform, move, commit, both reads, the motion table and
 * gfx_trace_scene treat it as any member.  gfx_shell_set_params and gfx_shell_set_geometry on it ask for a new commit.  In its
 * record the two height-map pointers carry the shell BVH's nodes and triangles (csrc/nrtdsm/shell_instance.hip.h).  Such a set is
 * rendered through gfx_scene_bind_displaced_kinds, one material per shell geometry; gfx_scene_bind_displaced
 * and gfx_scene_bind_displaced_passes refuse it (by them it is traced but not rendered). */
#define GFX_INSTANCE_SHELL 2u
int gfx_tfdm_set_add_shell(gfx_tfdm_set* set, gfx_shell* obj, const float objToWorld[12], uint32_t userId, uint32_t* index);
int gfx_tfdm_set_transform(gfx_tfdm_set* set, uint32_t index, const float objToWorld[12]);
int gfx_tfdm_set_move(gfx_tfdm_set* set, uint32_t index, const float objToWorld[12]);
int gfx_tfdm_set_commit(gfx_ctx* ctx, void* stream, gfx_tfdm_set* set);
/* The committed InstanceRecord table, 192 bytes per instance (`bytes` must be exactly that), for tests. */
int gfx_tfdm_set_read(gfx_ctx* ctx, gfx_tfdm_set* set, void* hostOut, size_t bytes);
/* The committed motion table, 48 bytes per instance (`bytes` must be exactly that), for tests; refuses what gfx_tfdm_set_read refuses. */
int gfx_tfdm_set_read_motion(gfx_ctx* ctx, gfx_tfdm_set* set, void* hostOut, size_t bytes);
/* The union of the committed records' world boxes (boxLo / boxHi, padded as the scene query tests them), from the committed table on
 * the host: what a ReGIR grid or a camera fit needs of members that are not in the BVH8.  An empty set gives the empty box lo = +inf,
 * hi = -inf; a set with an uncommitted change is refused. */
int gfx_tfdm_set_bounds(gfx_tfdm_set* set, float lo[3], float hi[3]);
int gfx_tfdm_set_destroy(gfx_tfdm_set* set);

/* closest-hit record of gfx_trace_scene, 32 B (what a renderer needs from a displaced hit: tfdm/tfdm_shared.h:570-577).
 *   miss                       dist = the ray's tmax, where = index = GFX_INVALID_SLOT, the rest zero
 *   plain hit                  where = GFX_SCENE_PLAIN, dist / bcB / bcC / index as gfx_hit (index = triIndex), normal zero
 *   displaced hit, instance k  where = k << 1 | frontFace, index = the base primIndex, bcB / bcC on the base triangle, normal =
 *                              the unit WORLD-space normal (the object-space normal through the instance's normal matrix; for
 *                              an instance of GFX_TFDM_BILINEAR that of the smooth surface at the hit) */
typedef struct gfx_scene_hit { float dist, bcB, bcC; uint32_t index; float normal[3]; uint32_t where; } gfx_scene_hit;
#define GFX_SCENE_PLAIN 0x80000000u
/* One optixTrace on an instance AS that mixes triangle GASes and custom-primitive GASes (tfdm/tfdm_main.cpp:2620-2640): world
 * rays in gfx_trace's layout against the BVH8 `accel` (0: none) and the displaced instances of `set` (NULL: none).  The closest
 * hit wins; on equal distance a plain hit beats a displaced one and a lower instance index a higher one.  mode
 * GFX_TRACE_CLOSEST: dOut = gfx_scene_hit[numRays]; GFX_TRACE_ANY: dOut = uint32_t[numRays] (1 = occluded).  Distances are the
 * world ray's parameter (object-space directions are not renormalised).  dCounters (optional, device u64[8], added to): [0..3]
 * as gfx_tfdm_trace, [4] world-box tests, [5] object-space traversals started.  Alignment as gfx_tfdm_trace.  A set with an
 * uncommitted add or transform, or with a member whose gfx_tfdm_set_params (gfx_nrtdsm_set_params) ran after the commit, is refused
 * with a message.  Members of all kinds are walked in one index order, so the rule above holds across kinds; [0..3] sum over them.
 * A shell member's hit is a displaced hit as above (index = the base primIndex, bcB / bcC on the base triangle, normal = the unit world
 * normal, where = k << 1 | frontFace); a stale shell member's message names gfx_shell_set_params or gfx_shell_set_geometry. */
int gfx_trace_scene(gfx_ctx* ctx, void* stream, uint64_t accel, gfx_tfdm_set* set, int mode, const void* dRayOrgTmin, const void* dRayDirTmax,
                    uint32_t numRays, void* dOut, void* dCounters);
/* What only a shell member's hit has, the last 16 bytes of a gfx_shell_hit: all zeros for a miss, a plain hit and a hit on a member
 * of another kind. */
typedef struct gfx_scene_shell_part { uint32_t shellTriangle, shellGeom; int32_t tile[2]; } gfx_scene_shell_part;
/* gfx_trace_scene with that side output.  GFX_TRACE_CLOSEST: dShellPart is NULL or a 16-byte aligned gfx_scene_shell_part[numRays],
 * written for every ray (a misaligned one is refused with a message); GFX_TRACE_ANY ignores it.  gfx_trace_scene is this call with
 * NULL, and gives the same gfx_scene_hit bytes. */
int gfx_trace_scene_ex(gfx_ctx* ctx, void* stream, uint64_t accel, gfx_tfdm_set* set, int mode, const void* dRayOrgTmin, const void* dRayDirTmax,
                       uint32_t numRays, void* dOut, void* dCounters, void* dShellPart);

/* Displaced instances in the renderer (DESIGN.md sections 16 and 17).  While a set is bound, GFX_RESTIR_SETUP_GBUFFERS /
 * GFX_PT_SETUP_GBUFFERS and GFX_PT_PATH_TRACE_BASELINE trace plain and displaced geometry together (the scene query above, in their
 * wavefront form whatever "fuse_passes" says).  A binding made with GFX_DISPLACED_RESTIR in its pass mask (gfx_scene_bind_displaced_passes)
 * also runs the ReSTIR passes and the rearchitected set over it: their shadow rays become the scene's any-hit query, and they too run in
 * their three-kernel form whatever "fuse_passes" says.  A binding made with GFX_DISPLACED_REGIR runs the ReGIR passes of gfx_pt_launch
 * (DESIGN.md section 26): the two cell-reservoir builds and GFX_PT_REGIR_UPDATE_LAST_ACCESS as they always ran (the grid never looks at
 * geometry), GFX_PT_PATH_TRACE_REGIR in its wavefront form whatever "fuse_passes" says, its shadow and extension rays through the scene
 * query.  The grid is the caller's (gfx_regir_set_params): the displaced members are not in the BVH8, so size it from the scene's bounds
 * joined with gfx_tfdm_set_bounds (a vertex outside the grid clamps to a border cell).  The two bits may be set together.  Every pass
 * the binding does not carry (ReSTIR and ReGIR without their bit; NRC, GFX_PT_PATH_TRACE_NRC_REGIR included, with any binding) is refused
 * with a message.  Without a binding every pass does what it always did.
 *   geomInstSlots[k]  the geometry instance k of the set is shaded with: a gfx_geom_create of the vertex and triangle arrays the
 *                     instance's gfx_tfdm was created from, put in NO group (so it is not in the BVH8).  Material, texture
 *                     coordinates and texCoord0Dir come from it, transform and normal matrix from the instance's record.
 * Refused: n other than the set's instance count, an unknown slot, a slot whose triangle count differs from the object's, a slot
 * whose material emits (the light distributions do not know displaced emitters).  A set with an uncommitted change is refused at
 * launch, as gfx_trace_scene refuses it.  set == NULL unbinds; gfx_tfdm_set_destroy of the bound set unbinds too.
 * A displaced pixel in the G-buffers:
 *   gbuffer0   instSlot = GFX_GBUFFER_DISPLACED | k (k: the set index; 0xFFFFFFFF stays "no surface"), geomInstSlot = the bound
 *              geometry, primIndex = the base triangle, qbcB / qbcC = the base barycentrics
 *   gbuffer1   the motion vector of prevPositionInWorld = curToPrev * positionInWorld under the previous camera, curToPrev being the
 *              instance's entry of the set's motion table: an instance moved with gfx_tfdm_set_move carries its own motion, one that
 *              was not moved (or was teleported with gfx_tfdm_set_transform) only the camera's
 *   gbuffer2   positionInWorld = origin + distance * direction of the world ray; qGeometricNormal = the hit's world normal
 *   gbuffer3   qShadingNormal = the same normal (no bump mapping on a displaced surface, as in the reference), qShadingTangent =
 *              texCoord0Dir of the base triangle in world space, orthogonal to it; qTexCoord, matSlot from the base triangle
 * BSDF textures are read at level 0 (this library's textures have no mip chain; the reference passes targetMipLevel).
 * G-buffers that hold displaced pixels are for the passes above, the ReSTIR passes of a binding that carries GFX_DISPLACED_RESTIR
 * (no ReSTIR kernel looks an instance, a geometry or a triangle up by a G-buffer id: DESIGN.md section 17) and the output-chain
 * copies; run the G-buffer pass again after unbinding before any other pass reads them. */
#define GFX_GBUFFER_DISPLACED 0x80000000u
int gfx_scene_bind_displaced(gfx_ctx* ctx, gfx_tfdm_set* set, const uint32_t* geomInstSlots, uint32_t n);   /* set == NULL: unbind */
/* The same binding with the passes it serves: gfx_scene_bind_displaced is this call with GFX_DISPLACED_GBUFFER_PT, which every
 * binding carries.  Checks and refusals are those above; an unknown bit in passMask is refused.  Displaced emitters stay refused. */
#define GFX_DISPLACED_GBUFFER_PT 1u   /* the G-buffer passes and the baseline path tracer */
#define GFX_DISPLACED_RESTIR 2u       /* ... and the ReSTIR passes, the rearchitected set included */
/* (bit 4 is not assigned: a mask that carries it is refused as an unknown bit, which callers may rely on) */
#define GFX_DISPLACED_REGIR 8u        /* ... and the ReGIR passes: both cell builds, GFX_PT_PATH_TRACE_REGIR, the last-access update */
int gfx_scene_bind_displaced_passes(gfx_ctx* ctx, gfx_tfdm_set* set, const uint32_t* geomInstSlots, uint32_t n, uint32_t passMask);
/* The binding for a set with members of any kind: the two calls above refuse a set that has an NRTDSM or a
 * shell member, this one renders it.  members[k] describes member k of the set; passMask as above; set == NULL unbinds.  An NRTDSM
 * member is shaded as a TFDM member is (its hit has the same fields).  A shell member has one material per shell geometry, as the
 * reference's materialSlots[shellBvhGeomIndex]: a hit on shell geometry g is shaded with shellMatSlots[g]; texture coordinate and
 * tangent stay the base triangle's.  In the G-buffers of a set that has a shell member, gbuffer0.geomInstSlot of a displaced pixel
 * is geomInstSlot | shellGeom << 28 (shellGeom 0 for a member of another kind) and gbuffer3.matSlot the material chosen.
 * Refused, besides what gfx_scene_bind_displaced_passes refuses, with the member's index in the message: a shell member whose
 * numShellMaterials is not the object's number of shell geometries, another member with a count other than 0, an unknown material
 * slot among the first numShellMaterials, one that emits, a shell member's geomInstSlot >= 2^28.  The counts and the materials are
 * checked again at every launch (gfx_shell_set_geometry and gfx_material_set may have run since). */
typedef struct gfx_displaced_member {
    uint32_t geomInstSlot;        /* as geomInstSlots[k] of gfx_scene_bind_displaced */
    uint32_t numShellMaterials;   /* 0 for a TFDM / NRTDSM member; for a shell member the object's number of shell geometries (1..8) */
    uint32_t shellMatSlots[8];    /* material of shell geometry g; entries >= numShellMaterials are ignored */
} gfx_displaced_member;           /* 40 bytes */
int gfx_scene_bind_displaced_kinds(gfx_ctx* ctx, gfx_tfdm_set* set, const gfx_displaced_member* members, uint32_t n, uint32_t passMask);
/* The primary rays the G-buffer pass of the current parameters (gfx_restir_set_params) generates, by the device function the pass
 * runs: row-major, one ray per pixel, gfx_trace's layout.  With jittering on it reads rngBuffer and does not write it back. */
int gfx_restir_primary_rays(gfx_ctx* ctx, void* stream, uint32_t width, uint32_t height, void* dRayOrgTmin, void* dRayDirTmax);
/* The ray queue (gfx_trace's layout) and the occlusion words (uint32, 1 = occluded) of the most recent ray pass gfx_restir_launch*
 * ran in its three-kernel form, copied into buffers of `capacity` entries, with or without a binding; *count = the queue entries that
 * pass traced: its launch slots, slots without a ray included (tmax = -1, word 0), for a pass with one entry per slot, the device
 * count for a pass that compacts its rays (the unbiased spatial pass, the rearchitected set; this waits for `stream`).  Refused with
 * a message: no ray pass yet, the last one ran fused (no queue exists), capacity < *count (which is still set), rays not 16-byte or
 * words not 4-byte aligned.  `stream` is a hipStream_t passed as void*, as everywhere in this header. */
int gfx_restir_last_rays(gfx_ctx* ctx, void* stream, void* dRayOrgTmin, void* dRayDirTmax, void* dOccluded, uint32_t capacity, uint32_t* count);
/* The same for gfx_pt_launch: the compacted NEE (shadow ray) queue of the most recent any-hit pass a path tracer traced in its
 * wavefront form (the last one of that launch: the baseline's terminal vertex emits none, ReGIR ends on one), its occlusion words and,
 * if dOwnerPixel is not NULL, the pixel that owns each entry (uint32, row-major index); *count = the device count of that pass (this
 * waits for `stream`).  With or without a binding; under one the words are the scene query's.  The buffers are the context's ray
 * scratch: call before the next launch that traces rays.  Refused with a message: no such pass yet, the last path-tracing launch ran
 * fused (one kernel, no queue), the queue reallocated for a larger launch since, capacity < *count (which is still set), rays not
 * 16-byte or words / owners not 4-byte aligned. */
int gfx_pt_last_nee_rays(gfx_ctx* ctx, void* stream, void* dRayOrgTmin, void* dRayDirTmax, void* dOccluded, void* dOwnerPixel, uint32_t capacity,
                         uint32_t* count);

#ifdef __cplusplus
}
#endif
#endif /* GFXEXP_H */
