// scene_builder.cpp -- the gfxh_scene container of the host layer (include/gfxexp_host.h), and the loaders that take a file path.
//
// Mirrors the asset path of the reference host program without assimp:
//   immediate material values createImmTexture + sRGB sampler, common_host.cpp:1045-1073, 1602-1659
//   rectangle light           createRectangleLight, common_host.cpp:2431-2476
//   instances                 createInstance, common_host.cpp:2582-2656
//   textures by path          loadTexture, common_host.cpp:1163-1244
// The readers behind the paths are image_formats.cpp and image_codecs.cpp; OBJ + MTL, the procedural street, the environment-map
// tables and the image writers are translation units of their own (host_scene.h lists them).
#include <new>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <random>
#include "host_scene.h"
#include "tex_format.h"
#include "image_codecs.h"
#include "image_formats.h"
#include "../bc/bc_decode.hip.h"

using namespace gfx_host;
using gfx_img::Image;

namespace {

thread_local std::string g_hostError;

void mat3_mul(const double a[9], const double b[9], double o[9]) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) o[r * 3 + c] = a[r * 3 + 0] * b[0 * 3 + c] + a[r * 3 + 1] * b[1 * 3 + c] + a[r * 3 + 2] * b[2 * 3 + c];
}
// qFromEulerAngles = Rz(roll) * Ry(yaw) * Rx(pitch), common/basic_types.h:5120-5123
void euler_matrix(double roll, double pitch, double yaw, double o[9]) {
    const double cz = std::cos(roll), sz = std::sin(roll), cy = std::cos(yaw), sy = std::sin(yaw), cx = std::cos(pitch), sx = std::sin(pitch);
    const double Rz[9] = { cz, -sz, 0, sz, cz, 0, 0, 0, 1 };
    const double Ry[9] = { cy, 0, sy, 0, 1, 0, -sy, 0, cy };
    const double Rx[9] = { 1, 0, 0, 0, cx, -sx, 0, sx, cx };
    double t[9];
    mat3_mul(Rz, Ry, t);
    mat3_mul(t, Rx, o);
}

bool read_file(const std::string& path, std::vector<uint8_t>& out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    return true;
}
// the file at `path` through gfx_img::decode_any; false with the host error set, which names the file
bool decode_image(const std::string& path, Image& img) {
    std::vector<uint8_t> d;
    if (!read_file(path, d)) { g_hostError = "cannot read " + path; return false; }
    if (gfx_img::decode_any(d.data(), d.size(), img, g_hostError)) return true;
    g_hostError += ": " + path;
    return false;
}
template <uint32_t F>
void bc_first_channel(const uint8_t* blocks, uint32_t w, uint32_t h, std::vector<uint8_t>& out) {
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) out[static_cast<size_t>(y) * w + x] = static_cast<uint8_t>(gfx::bc::image_texel<F>(blocks, w, x, y) & 0xFFu);
}

} // namespace

std::string& gfx_host::host_error() { return g_hostError; }

bool gfx_host::read_dds(const std::string& path, std::vector<uint8_t>& file, gfxh_dds_info& info) {
    if (!read_file(path, file)) { g_hostError = "cannot open " + path; return false; }
    if (gfxh_dds_parse(file.data(), file.size(), &info)) { g_hostError += ": " + path; return false; }
    return true;
}

extern "C" {

const char* gfxh_last_error(void) { return g_hostError.c_str(); }
gfxh_scene* gfxh_scene_create(void) { return new gfxh_scene(); }
void gfxh_scene_destroy(gfxh_scene* s) { delete s; }

uint32_t gfxh_scene_add_material(gfxh_scene* s, const gfx_material* m) {
    s->materials.push_back(*m);
    return static_cast<uint32_t>(s->materials.size() - 1);
}

uint32_t gfxh_scene_add_material_traditional(gfxh_scene* s, const float diffuse[3], const float specular[3],
                                             float smoothness, const float emittance[3]) {
    gfx_material m;
    std::memset(&m, 0, sizeof(m));
    m.bsdfType = GFX_BSDF_DIFFUSE_AND_SPECULAR;
    for (int i = 0; i < 3; ++i) {
        m.a[i] = srgb_degamma(quantize8(diffuse[i]));
        m.b[i] = srgb_degamma(quantize8(specular[i]));
        m.emittance[i] = emittance ? emittance[i] : 0.0f;
    }
    m.smoothness = quantize8(smoothness);
    m.hasEmittance = (m.emittance[0] != 0.0f || m.emittance[1] != 0.0f || m.emittance[2] != 0.0f) ? 1u : 0u;
    return gfxh_scene_add_material(s, &m);
}

// ---------------------------------------------------------------- textures
uint32_t gfxh_scene_add_texture(gfxh_scene* s, uint32_t width, uint32_t height, uint32_t format, const void* texels) {
    const size_t bpp = gfx::tex_bytes_per_texel(format);
    if (!bpp || !width || !height || !texels) { g_hostError = "gfxh_scene_add_texture: bad arguments"; return 0; }
    if (width > gfx_img::kMaxDim || height > gfx_img::kMaxDim) { g_hostError = "gfxh_scene_add_texture: texture larger than 16384 x 16384"; return 0; }
    try {   // nothing may unwind through the C boundary (a bad_alloc from the copy)
        Tex t;
        t.width = width; t.height = height; t.format = format;
        t.texels.assign(static_cast<const uint8_t*>(texels), static_cast<const uint8_t*>(texels) + bpp * width * height);
        s->textures.push_back(std::move(t));
    }
    catch (const std::exception& e) { g_hostError = std::string("gfxh_scene_add_texture: ") + e.what(); return 0; }
    return static_cast<uint32_t>(s->textures.size());   // 1-based slot
}
uint32_t gfxh_scene_num_textures(gfxh_scene* s) { return static_cast<uint32_t>(s->textures.size()); }
int gfxh_scene_get_texture(gfxh_scene* s, uint32_t slot, uint32_t* width, uint32_t* height, uint32_t* format, const void** texels) {
    if (slot == 0 || slot > s->textures.size()) { g_hostError = "gfxh_scene_get_texture: bad slot"; return 1; }
    const Tex& t = s->textures[slot - 1];
    *width = t.width; *height = t.height; *format = t.format; *texels = t.isBc ? nullptr : t.texels.data();
    return 0;
}
uint32_t gfxh_scene_add_texture_bc(gfxh_scene* s, uint32_t width, uint32_t height, uint32_t bcFormat, const void* blocks, uint32_t format) {
    const size_t blockBytes = gfx::bc::block_bytes(bcFormat), bpp = gfx::tex_bytes_per_texel(format);
    if (!blockBytes || !bpp || format == GFX_TEX_RGBA32F || !width || !height || !blocks) { g_hostError = "gfxh_scene_add_texture_bc: bad arguments"; return 0; }
    if (width > gfx_img::kMaxDim || height > gfx_img::kMaxDim) { g_hostError = "gfxh_scene_add_texture_bc: texture larger than 16384 x 16384"; return 0; }
    try {
        Tex t;
        t.width = width; t.height = height; t.format = format; t.isBc = true; t.bcFormat = bcFormat;
        const size_t bytes = static_cast<size_t>((width + 3) / 4) * ((height + 3) / 4) * blockBytes;
        t.blocks.assign(static_cast<const uint8_t*>(blocks), static_cast<const uint8_t*>(blocks) + bytes);
        s->textures.push_back(std::move(t));
    }
    catch (const std::exception& e) { g_hostError = std::string("gfxh_scene_add_texture_bc: ") + e.what(); return 0; }
    return static_cast<uint32_t>(s->textures.size());
}
int gfxh_scene_get_texture_bc(gfxh_scene* s, uint32_t slot, uint32_t* bcFormat, const void** blocks, size_t* bytes) {
    if (slot == 0 || slot > s->textures.size()) { g_hostError = "gfxh_scene_get_texture_bc: bad slot"; return 1; }
    const Tex& t = s->textures[slot - 1];
    if (!t.isBc) { *blocks = nullptr; *bytes = 0; return 0; }
    *bcFormat = t.bcFormat; *blocks = t.blocks.data(); *bytes = t.blocks.size();
    return 0;
}

int gfxh_dds_parse(const void* data, size_t bytes, gfxh_dds_info* info) {
    std::string err;
    if (!data || !info) { g_hostError = "gfxh_dds_parse: null argument"; return 1; }
    if (!gfx_img::dds_parse(static_cast<const uint8_t*>(data), bytes, *info, err)) { g_hostError = "gfxh_dds_parse: " + err; return 1; }
    return 0;
}

int gfxh_image_info(const void* data, size_t bytes, gfxh_image_desc* info) {
    gfx_img::Info i; std::string err;
    if (!data || !info || !gfx_img::info(static_cast<const uint8_t*>(data), bytes, i, err)) { g_hostError = "gfxh_image_info: " + (err.empty() ? std::string("null argument") : err); return 1; }
    info->width = i.width; info->height = i.height; info->channels = i.channels; info->kind = i.kind;
    return 0;
}
int gfxh_image_decode_rgba8(const void* data, size_t bytes, void* out, size_t capacityBytes) {
    gfx_img::Info i; std::string err;
    if (!data || !out) { g_hostError = "gfxh_image_decode_rgba8: null argument"; return 1; }
    // the header first, so that a buffer that is too small is reported before anything is decoded
    if (!gfx_img::info(static_cast<const uint8_t*>(data), bytes, i, err)) { g_hostError = "gfxh_image_decode_rgba8: " + err; return 1; }
    if (capacityBytes < 4ull * i.width * i.height) { g_hostError = "gfxh_image_decode_rgba8: the output buffer holds fewer than 4 * width * height bytes"; return 1; }
    std::vector<uint8_t> rgba;
    if (!gfx_img::decode(static_cast<const uint8_t*>(data), bytes, i, rgba, err)) { g_hostError = "gfxh_image_decode_rgba8: " + err; return 1; }
    if (rgba.size() > capacityBytes) { g_hostError = "gfxh_image_decode_rgba8: the decoded image does not have the size of its header"; return 1; }
    std::memcpy(out, rgba.data(), rgba.size());
    return 0;
}

// loadTexture (common_host.cpp:1163-1244): cached per path; 8-bit images become RGBA8 read through `format8`
// (GFX_TEX_RGBA8_SRGB for colour maps = needsDegamma, GFX_TEX_RGBA8_UNORM for normal maps, GFX_TEX_R8_UNORM takes
// the red channel); float images become GFX_TEX_RGBA32F (isHDR).  Returns the texture slot, 0 on failure.
uint32_t gfxh_scene_load_texture(gfxh_scene* s, const char* path, uint32_t format8) {
    const std::string key = std::string(path) + "#" + std::to_string(format8);
    auto it = s->textureCache.find(key);
    if (it != s->textureCache.end()) return it->second;
    Image img;
    try {
        if (gfx_img::is_dds_path(path)) {
            // the .dds branch of loadTexture (common_host.cpp:1185-1209): level 0 as it lies in the file; blocks stay blocks
            std::vector<uint8_t> file;
            gfxh_dds_info info;
            if (!read_dds(path, file, info)) return 0;
            if (info.isBlockCompressed) {
                const uint32_t fmt = (format8 == GFX_TEX_RGBA8_UNORM || format8 == GFX_TEX_R8_UNORM || format8 == GFX_TEX_RG8_UNORM) ? format8 : GFX_TEX_RGBA8_SRGB;
                const uint32_t slot = gfxh_scene_add_texture_bc(s, info.width, info.height, info.bcFormat, file.data() + info.dataOffset, fmt);
                if (slot) s->textureCache[key] = slot;
                return slot;
            }
            img.w = info.width; img.h = info.height;
            img.rgba8.assign(file.begin() + static_cast<std::ptrdiff_t>(info.dataOffset), file.begin() + static_cast<std::ptrdiff_t>(info.dataOffset + info.dataBytes));
            if (info.isBGRA) for (size_t i = 0; i < img.rgba8.size(); i += 4) std::swap(img.rgba8[i], img.rgba8[i + 2]);
        }
        else if (!decode_image(path, img)) return 0;
    }
    catch (const std::exception& e) { g_hostError = std::string("gfxh_scene_load_texture: ") + e.what(); return 0; }   // a bad_alloc from the decode buffers
    uint32_t slot = 0;
    if (img.isFloat) slot = gfxh_scene_add_texture(s, img.w, img.h, GFX_TEX_RGBA32F, img.rgba32f.data());
    else if (format8 == GFX_TEX_R8_UNORM || format8 == GFX_TEX_RG8_UNORM) {
        const uint32_t ch = format8 == GFX_TEX_R8_UNORM ? 1 : 2;
        std::vector<uint8_t> packed;
        try { packed.resize(static_cast<size_t>(img.w) * img.h * ch); }
        catch (const std::exception& e) { g_hostError = std::string("gfxh_scene_load_texture: ") + e.what(); return 0; }
        for (size_t i = 0; i < static_cast<size_t>(img.w) * img.h; ++i) for (uint32_t c = 0; c < ch; ++c) packed[i * ch + c] = img.rgba8[4 * i + c];
        slot = gfxh_scene_add_texture(s, img.w, img.h, format8, packed.data());
    }
    else slot = gfxh_scene_add_texture(s, img.w, img.h, format8 == GFX_TEX_RGBA8_UNORM ? GFX_TEX_RGBA8_UNORM : GFX_TEX_RGBA8_SRGB, img.rgba8.data());
    if (slot) s->textureCache[key] = slot;
    return slot;
}

// The height texture of tfdm_main.cpp:2218-2255 as gfx_tfdm_create takes it: first channel, c / 255.
int gfxh_tfdm_load_height(const char* path, uint32_t* size, float** heights) {
    if (!path || !size || !heights) { g_hostError = "gfxh_tfdm_load_height: null argument"; return 1; }
    *size = 0; *heights = nullptr;
    uint32_t w = 0, h = 0;
    std::vector<uint8_t> first;
    try {
        if (gfx_img::is_dds_path(path)) {
            std::vector<uint8_t> file;
            gfxh_dds_info info;
            if (!read_dds(path, file, info)) return 1;
            w = info.width; h = info.height;
            first.resize(static_cast<size_t>(w) * h);
            const uint8_t* data = file.data() + info.dataOffset;
            if (!info.isBlockCompressed) for (size_t i = 0; i < first.size(); ++i) first[i] = data[4 * i + (info.isBGRA ? 2 : 0)];
            else switch (info.bcFormat) {
                case GFX_BC1: bc_first_channel<gfx::bc::kBC1>(data, w, h, first); break;
                case GFX_BC2: bc_first_channel<gfx::bc::kBC2>(data, w, h, first); break;
                case GFX_BC3: bc_first_channel<gfx::bc::kBC3>(data, w, h, first); break;
                case GFX_BC4_UNORM: bc_first_channel<gfx::bc::kBC4U>(data, w, h, first); break;
                case GFX_BC4_SNORM: bc_first_channel<gfx::bc::kBC4S>(data, w, h, first); break;
                case GFX_BC5_UNORM: bc_first_channel<gfx::bc::kBC5U>(data, w, h, first); break;
                case GFX_BC5_SNORM: bc_first_channel<gfx::bc::kBC5S>(data, w, h, first); break;
                case GFX_BC7: bc_first_channel<gfx::bc::kBC7>(data, w, h, first); break;
                default: g_hostError = std::string("gfxh_tfdm_load_height: unknown block format in ") + path; return 1;
            }
        }
        else {
            Image img;
            if (!decode_image(path, img)) return 1;
            if (img.isFloat) { g_hostError = std::string("gfxh_tfdm_load_height: a float image is no 8-bit height map: ") + path; return 1; }
            w = img.w; h = img.h;
            first.resize(static_cast<size_t>(w) * h);
            for (size_t i = 0; i < first.size(); ++i) first[i] = img.rgba8[4 * i];
        }
    }
    catch (const std::exception& e) { g_hostError = std::string("gfxh_tfdm_load_height: ") + e.what(); return 1; }
    // tfdm_main.cpp:2236-2239
    if (w != h) { g_hostError = std::string("gfxh_tfdm_load_height: the height map is not square: ") + path; return 1; }
    if (w == 0 || (w & (w - 1u)) != 0u) { g_hostError = std::string("gfxh_tfdm_load_height: the height map's size is no power of two: ") + path; return 1; }
    float* out = static_cast<float*>(std::malloc(sizeof(float) * first.size()));
    if (!out) { g_hostError = "gfxh_tfdm_load_height: out of memory"; return 1; }
    for (size_t i = 0; i < first.size(); ++i) out[i] = static_cast<float>(first[i]) / 255.0f;
    *size = w; *heights = out;
    return 0;
}
void gfxh_tfdm_free_height(float* heights) { std::free(heights); }

uint32_t gfxh_scene_add_geom(gfxh_scene* s, const gfx_vertex* v, uint32_t nv, const uint32_t* tris, uint32_t nt, uint32_t matSlot) {
    Geom g;
    g.v.assign(v, v + nv);
    g.t.assign(tris, tris + 3ull * nt);
    g.mat = matSlot;
    s->geoms.push_back(std::move(g));
    return static_cast<uint32_t>(s->geoms.size() - 1);
}
uint32_t gfxh_scene_add_group(gfxh_scene* s, const uint32_t* geomSlots, uint32_t n) {
    s->groups.emplace_back(geomSlots, geomSlots + n);
    return static_cast<uint32_t>(s->groups.size() - 1);
}
uint32_t gfxh_scene_add_instance(gfxh_scene* s, uint32_t group, const float xfm[12]) {
    Inst i;
    i.group = group;
    std::memcpy(i.xfm, xfm, sizeof(float) * 12);
    s->insts.push_back(i);
    return static_cast<uint32_t>(s->insts.size() - 1);
}

uint32_t gfxh_scene_add_rectangle(gfxh_scene* s, float width, float depth, const float emittance[3]) {
    const float refl[3] = { 0.01f, 0.01f, 0.01f }, spec[3] = { 0, 0, 0 };
    const uint32_t mat = gfxh_scene_add_material_traditional(s, refl, spec, 0.3f, emittance);
    const V3 n = { 0, -1, 0 }, t = { 1, 0, 0 };
    const gfx_vertex v[4] = {
        make_vertex({ -0.5f * width, 0.0f, -0.5f * depth }, n, t, 0.0f, 1.0f),
        make_vertex({ 0.5f * width, 0.0f, -0.5f * depth }, n, t, 1.0f, 1.0f),
        make_vertex({ 0.5f * width, 0.0f, 0.5f * depth }, n, t, 1.0f, 0.0f),
        make_vertex({ -0.5f * width, 0.0f, 0.5f * depth }, n, t, 0.0f, 0.0f) };
    const uint32_t tris[6] = { 0, 1, 2, 0, 2, 3 };
    const uint32_t g = gfxh_scene_add_geom(s, v, 4, tris, 2, mat);
    return gfxh_scene_add_group(s, &g, 1);
}

uint32_t gfxh_scene_add_rectangle_textured(gfxh_scene* s, float width, float depth, const float emittance[3], const char* emitterTexturePath) {
    const uint32_t group = gfxh_scene_add_rectangle(s, width, depth, emittance);
    if (group == 0xFFFFFFFFu || !emitterTexturePath || !emitterTexturePath[0]) return group;
    // createEmittanceTexture (common_host.cpp:1524-1531): an 8-bit image goes behind the sRGB sampler, a float image behind the
    // float sampler; a file that cannot be read leaves the immediate emittance in place
    const uint32_t tex = gfxh_scene_load_texture(s, emitterTexturePath, GFX_TEX_RGBA8_SRGB);
    if (tex) { gfx_material& m = s->materials.back(); m.texEmittance = tex; m.hasEmittance = 1u; }
    return group;
}

void gfxh_make_transform(float scale, float rollDeg, float pitchDeg, float yawDeg, const float pos[3], float out[12]) {
    const double d2r = 3.14159265358979323846 / 180.0;
    double R[9];
    euler_matrix(rollDeg * d2r, pitchDeg * d2r, yawDeg * d2r, R);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) out[r * 4 + c] = static_cast<float>(R[r * 3 + c] * scale);
        out[r * 4 + 3] = pos[r];
    }
}
void gfxh_make_orientation(float rollDeg, float pitchDeg, float yawDeg, float out[9]) {
    const double d2r = 3.14159265358979323846 / 180.0;
    double R[9];
    euler_matrix(rollDeg * d2r, pitchDeg * d2r, yawDeg * d2r, R);
    for (int i = 0; i < 9; ++i) out[i] = static_cast<float>(R[i]);
}

void gfxh_seed_rng_states(uint64_t* states, uint64_t count, uint64_t seed) {
    std::mt19937_64 gen(seed);
    for (uint64_t i = 0; i < count; ++i) states[i] = gen();
}

int gfxh_scene_counts(gfxh_scene* s, uint32_t counts[5]) {
    counts[0] = static_cast<uint32_t>(s->materials.size());
    counts[1] = static_cast<uint32_t>(s->geoms.size());
    counts[2] = static_cast<uint32_t>(s->groups.size());
    counts[3] = static_cast<uint32_t>(s->insts.size());
    uint64_t tris = 0;
    for (const Inst& i : s->insts) for (uint32_t g : s->groups[i.group]) tris += s->geoms[g].t.size() / 3;
    counts[4] = static_cast<uint32_t>(tris);
    return 0;
}
int gfxh_scene_get_material(gfxh_scene* s, uint32_t i, gfx_material* out) { if (i >= s->materials.size()) return 1; *out = s->materials[i]; return 0; }
int gfxh_scene_get_geom(gfxh_scene* s, uint32_t i, const gfx_vertex** v, uint32_t* nv, const uint32_t** tris, uint32_t* nt, uint32_t* matSlot) {
    if (i >= s->geoms.size()) return 1;
    const Geom& g = s->geoms[i];
    *v = g.v.data(); *nv = static_cast<uint32_t>(g.v.size()); *tris = g.t.data(); *nt = static_cast<uint32_t>(g.t.size() / 3); *matSlot = g.mat;
    return 0;
}
int gfxh_scene_get_group(gfxh_scene* s, uint32_t i, const uint32_t** geomSlots, uint32_t* n) {
    if (i >= s->groups.size()) return 1;
    *geomSlots = s->groups[i].data(); *n = static_cast<uint32_t>(s->groups[i].size());
    return 0;
}
int gfxh_scene_get_instance(gfxh_scene* s, uint32_t i, uint32_t* group, float xfm[12]) {
    if (i >= s->insts.size()) return 1;
    *group = s->insts[i].group; std::memcpy(xfm, s->insts[i].xfm, sizeof(float) * 12);
    return 0;
}
int gfxh_scene_bounds(gfxh_scene* s, float bounds[6]) {
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (const Inst& i : s->insts)
        for (uint32_t g : s->groups[i.group])
            for (const gfx_vertex& v : s->geoms[g].v) {
                float w[3];
                xfm_point(i.xfm, v.position, w);
                for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], w[k]); hi[k] = std::max(hi[k], w[k]); }
            }
    for (int k = 0; k < 3; ++k) { bounds[k] = lo[k]; bounds[3 + k] = hi[k]; }
    return 0;
}

int gfxh_scene_upload(gfxh_scene* s, gfx_ctx* ctx) {
    for (uint32_t t = 0; t < s->textures.size(); ++t) {
        const Tex& tx = s->textures[t];
        if (tx.isBc ? gfx_texture_set_bc(ctx, t + 1, tx.width, tx.height, tx.bcFormat, tx.blocks.data(), tx.format)
                    : gfx_texture_set(ctx, t + 1, tx.width, tx.height, tx.format, tx.texels.data())) { g_hostError = gfx_last_error(ctx); return 1; }
    }
    for (uint32_t i = 0; i < s->materials.size(); ++i)
        if (gfx_material_set(ctx, i, &s->materials[i])) { g_hostError = gfx_last_error(ctx); return 1; }
    for (const Geom& g : s->geoms) {
        uint32_t slot;
        if (gfx_geom_create(ctx, g.v.data(), sizeof(gfx_vertex), static_cast<uint32_t>(g.v.size()), g.t.data(),
                            static_cast<uint32_t>(g.t.size() / 3), g.mat, &slot)) { g_hostError = gfx_last_error(ctx); return 1; }
    }
    for (const auto& grp : s->groups) {
        uint32_t slot;
        if (gfx_group_create(ctx, grp.data(), static_cast<uint32_t>(grp.size()), &slot)) { g_hostError = gfx_last_error(ctx); return 1; }
    }
    for (const Inst& i : s->insts) {
        uint32_t slot;
        if (gfx_instance_create(ctx, i.group, i.xfm, &slot)) { g_hostError = gfx_last_error(ctx); return 1; }
    }
    return 0;
}

} // extern "C"
