// host_scene.h -- what the translation units of the host scene layer share (internal; the C ABI is include/gfxexp_host.h):
// the gfxh_scene container, the per-thread error string behind gfxh_last_error, and the few helpers more than one of them needs.
//   scene_builder.cpp   the container, materials, rectangles, transforms, the loaders by path
//   obj_loader.cpp      OBJ + MTL          street_scene.cpp   the procedural street
//   env_tables.cpp      environment-map tables, the Halton disk          image_output.cpp   tone mapper and image writers
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <string>
#include <vector>
#include "../../../include/gfxexp_host.h"

namespace gfx_host {

struct Geom { std::vector<gfx_vertex> v; std::vector<uint32_t> t; uint32_t mat; };
struct Inst { uint32_t group; float xfm[12]; };
// an uncompressed texture holds texels; a block-compressed one holds blocks (isBc) and is sampled as the 8-bit `format`
struct Tex { uint32_t width = 0, height = 0, format = 0; std::vector<uint8_t> texels; bool isBc = false; uint32_t bcFormat = 0; std::vector<uint8_t> blocks; };

} // namespace gfx_host

struct gfxh_scene {
    std::vector<gfx_material> materials;
    std::vector<gfx_host::Geom> geoms;
    std::vector<std::vector<uint32_t>> groups;
    std::vector<gfx_host::Inst> insts;
    std::vector<gfx_host::Tex> textures;             // textures[k] is texture slot k + 1
    std::map<std::string, uint32_t> textureCache;    // file path + format -> slot (TextureCacheKey, common_host.cpp:1163-1182)
};

namespace gfx_host {

// the string gfxh_last_error returns, one per thread (defined in scene_builder.cpp)
std::string& host_error();

// A .dds file and its parsed header; false with the host error set ("cannot open <path>", or the parser's reason followed by the
// path).  The read may throw bad_alloc: callers sit inside the try block of their C entry point.  (scene_builder.cpp)
bool read_dds(const std::string& path, std::vector<uint8_t>& file, gfxh_dds_info& info);

struct V3 { float x, y, z; };
inline V3 operator+(V3 a, V3 b) { return { a.x + b.x, a.y + b.y, a.z + b.z }; }
inline V3 operator-(V3 a, V3 b) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }
inline V3 operator*(V3 a, float s) { return { a.x * s, a.y * s, a.z * s }; }
inline V3 cross(V3 a, V3 b) { return { a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
inline float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline V3 normalize(V3 a) { const float l = std::sqrt(dot(a, a)); const float r = 1 / l; return { a.x * r, a.y * r, a.z * r }; }

// makeCoordinateSystem, common/common_host.cpp:2349-2356
inline V3 tangent_from_normal(V3 n) {
    const float sign = n.z >= 0 ? 1.0f : -1.0f;
    const float a = -1 / (sign + n.z);
    const float b = n.x * n.y * a;
    return { 1 + sign * n.x * n.x * a, sign * b, -sign * n.x };
}

inline gfx_vertex make_vertex(V3 p, V3 n, V3 t, float u, float v) {
    gfx_vertex o;
    o.position[0] = p.x; o.position[1] = p.y; o.position[2] = p.z;
    o.normal[0] = n.x; o.normal[1] = n.y; o.normal[2] = n.z;
    o.texCoord0Dir[0] = t.x; o.texCoord0Dir[1] = t.y; o.texCoord0Dir[2] = t.z;
    o.texCoord[0] = u; o.texCoord[1] = v;
    return o;
}

// 8-bit immediate texture value (common_host.cpp:1045-1073) ...
// The reference converts the float straight to uint32_t -- undefined for a negative or non-finite material constant (an .mtl file is
// untrusted input); what its x86-64 build does is cvttss2si to 64 bits and keep the low word, which is spelled out here.
inline uint32_t float_to_u32_like_x86_64(float f) {
    if (!(f > -9.2e18f && f < 9.2e18f)) return 0u;                 // NaN / outside int64: the "integer indefinite" 0x8000...0, low word 0
    return static_cast<uint32_t>(static_cast<uint64_t>(static_cast<int64_t>(f)));
}
inline float quantize8(float v) { const uint32_t q = std::min(float_to_u32_like_x86_64(255 * v), 255u); return q / 255.0f; }
// ... read through an sRGB-decoding sampler (basic_types.h:5396-5402 states the formula)
inline float srgb_degamma(float v) {
    if (v <= 0.04045f) return v / 12.92f;
    return std::pow((v + 0.055f) / 1.055f, 2.4f);
}

inline void xfm_point(const float m[12], const float p[3], float o[3]) {
    for (int r = 0; r < 3; ++r) o[r] = m[r * 4 + 0] * p[0] + m[r * 4 + 1] * p[1] + m[r * 4 + 2] * p[2] + m[r * 4 + 3];
}

} // namespace gfx_host
