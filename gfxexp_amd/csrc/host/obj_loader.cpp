// obj_loader.cpp -- the OBJ + MTL reader of the host layer: gfxh_scene_load_obj, gfxh_scene_load_obj_conv.
//
// Mirrors the asset path of the reference host program without assimp:
//   OBJ + MTL reader          createTriangleMeshes, common/common_host.cpp:2178-2429
//   texture maps              createDiffuseAndSpecularMaterial / createSimplePBRMaterial, common_host.cpp:1560-1760
#include <cmath>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <tuple>
#include "host_scene.h"
#include "image_formats.h"

using namespace gfx_host;

// Header of a .dds map named by a material; false when the path is no .dds or the file cannot be parsed (the load then fails the
// usual way and leaves the immediate value in place).
static bool dds_map_info(const std::string& path, gfxh_dds_info& info) {
    if (!gfx_img::is_dds_path(path.c_str())) return false;
    std::vector<uint8_t> file;
    try { return read_dds(path, file, info); }
    catch (const std::exception&) { return false; }
}

extern "C" {

static uint32_t load_obj_impl(gfxh_scene* s, const char* path, int simplePbr);
uint32_t gfxh_scene_load_obj(gfxh_scene* s, const char* path) { return gfxh_scene_load_obj_conv(s, path, GFXH_MATCONV_TRADITIONAL); }
uint32_t gfxh_scene_load_obj_conv(gfxh_scene* s, const char* path, int materialConvention) {
    try { return load_obj_impl(s, path, materialConvention == GFXH_MATCONV_SIMPLE_PBR ? 1 : 0); }   // nothing may unwind through the C boundary
    catch (const std::exception& e) { host_error() = std::string("gfxh_scene_load_obj: ") + e.what(); return 0xFFFFFFFFu; }
}
static uint32_t load_obj_impl(gfxh_scene* s, const char* path, int simplePbr) {
    std::ifstream in(path);
    if (!in) { host_error() = std::string("cannot open ") + path; return 0xFFFFFFFFu; }
    const std::string dir = std::string(path).substr(0, std::string(path).find_last_of("/\\") + 1);
    std::vector<V3> pos, nrm;
    std::vector<std::pair<float, float>> uv;
    struct MtlDesc {
        float kd[3] = { 0, 0, 0 }, ks[3] = { 0, 0, 0 }, ke[3] = { 0, 0, 0 }; float ns = 0;
        std::string mapKd, mapKs, mapKe, mapBump, mapNormal;   // AI_MATKEY_TEXTURE_DIFFUSE / SPECULAR / EMISSIVE / HEIGHT / NORMALS
    };
    std::map<std::string, MtlDesc> mtl;
    std::vector<std::string> matOrder;
    struct Corner { int v, t, n; };
    std::map<std::string, std::vector<Corner>> facesByMat;   // triangulated corner list per material
    std::string curMat = "";
    std::string line;
    auto parse_mtl = [&](const std::string& file) {
        std::ifstream m(dir + file);
        std::string l, cur;
        while (std::getline(m, l)) {
            std::istringstream ss(l);
            std::string k; ss >> k;
            if (k == "newmtl") { ss >> cur; mtl[cur] = MtlDesc(); }
            else if (k == "Kd") ss >> mtl[cur].kd[0] >> mtl[cur].kd[1] >> mtl[cur].kd[2];
            else if (k == "Ks") ss >> mtl[cur].ks[0] >> mtl[cur].ks[1] >> mtl[cur].ks[2];
            else if (k == "Ke") ss >> mtl[cur].ke[0] >> mtl[cur].ke[1] >> mtl[cur].ke[2];
            else if (k == "Ns") ss >> mtl[cur].ns;
            else if (k == "map_Kd" || k == "map_Ks" || k == "map_Ke" || k == "map_bump" || k == "map_Bump" || k == "bump" || k == "norm" || k == "map_Kn") {
                // last token = file name (options such as "-bm 1.0" come before it)
                std::string tok, file;
                while (ss >> tok) file = tok;
                for (char& ch : file) if (ch == '\\') ch = '/';
                MtlDesc& d = mtl[cur];
                if (k == "map_Kd") d.mapKd = file;
                else if (k == "map_Ks") d.mapKs = file;
                else if (k == "map_Ke") d.mapKe = file;
                else if (k == "norm" || k == "map_Kn") d.mapNormal = file;
                else d.mapBump = file;
            }
        }
    };
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string k; ss >> k;
        if (k == "v") { V3 p; ss >> p.x >> p.y >> p.z; pos.push_back(p); }
        else if (k == "vn") { V3 p; ss >> p.x >> p.y >> p.z; nrm.push_back(p); }
        else if (k == "vt") { float a = 0, b = 0; ss >> a >> b; uv.push_back({ a, b }); }
        else if (k == "mtllib") { std::string f; while (ss >> f) parse_mtl(f); }      // "mtllib a.mtl b.mtl": every library named
        else if (k == "usemtl") { ss >> curMat; }
        else if (k == "f") {
            std::vector<Corner> cs;
            std::string tok;
            while (ss >> tok) {
                Corner c = { 0, 0, 0 };
                int idx[3] = { 0, 0, 0 };
                int which = 0; std::string num;
                for (size_t i = 0; i <= tok.size(); ++i) {
                    if (i == tok.size() || tok[i] == '/') {
                        if (!num.empty()) {
                            char* end = nullptr;
                            const long val = std::strtol(num.c_str(), &end, 10);
                            if (*end != 0 || val < -2147483647L || val > 2147483647L) { host_error() = std::string("bad face index '") + tok + "' in " + path; return 0xFFFFFFFFu; }
                            idx[which] = static_cast<int>(val);
                        }
                        num.clear(); ++which; if (which > 2) break;
                    }
                    else num.push_back(tok[i]);
                }
                c.v = idx[0] < 0 ? static_cast<int>(pos.size()) + idx[0] : idx[0] - 1;
                c.t = idx[1] == 0 ? -1 : (idx[1] < 0 ? static_cast<int>(uv.size()) + idx[1] : idx[1] - 1);
                c.n = idx[2] == 0 ? -1 : (idx[2] < 0 ? static_cast<int>(nrm.size()) + idx[2] : idx[2] - 1);
                if (c.v < 0 || c.v >= static_cast<int>(pos.size()) || c.t >= static_cast<int>(uv.size()) || c.n >= static_cast<int>(nrm.size()) ||
                    (idx[1] != 0 && c.t < 0) || (idx[2] != 0 && c.n < 0)) {
                    host_error() = std::string("face index out of range '") + tok + "' in " + path; return 0xFFFFFFFFu;
                }
                cs.push_back(c);
            }
            if (!facesByMat.count(curMat)) matOrder.push_back(curMat);
            std::vector<Corner>& dst = facesByMat[curMat];
            for (size_t i = 1; i + 1 < cs.size(); ++i) { dst.push_back(cs[0]); dst.push_back(cs[i]); dst.push_back(cs[i + 1]); }
        }
    }
    std::vector<uint32_t> geomSlots;
    for (const std::string& name : matOrder) {
        const MtlDesc d = mtl.count(name) ? mtl[name] : MtlDesc();
        // smoothness = sqrt(Ns) / 11 (common_host.cpp:2271-2274); four Bistro pavement materials are pinned to 0.2 (:2286-2297)
        float smoothness = std::sqrt(d.ns) / 11.0f;
        if (name == "Pavement_Cobblestone_Big_BLENDSHADER" || name == "Pavement_Cobblestone_Small_BLENDSHADER" ||
            name == "Pavement_Brick_BLENDSHADER" || name == "Pavement_Cobblestone_Wet_BLENDSHADER") smoothness = 0.2f;
        const uint32_t matSlot = gfxh_scene_add_material_traditional(s, d.kd, d.ks, smoothness, d.ke);
        {   // texture maps (createDiffuseAndSpecularMaterial, common_host.cpp:1560-1700): a map that cannot be read
            // leaves the immediate value in place
            gfx_material& m = s->materials[matSlot];
            // needsDegamma of a colour map: true for every file stb_image reads (common_host.cpp:1223), but for a .dds it is what
            // translate derives from the file's format -- only the _SRGB DXGI formats (:766-886, :1194); the sampler follows it (:1597-1606)
            gfxh_dds_info dds;
            auto colour_format = [&](const std::string& file) {
                return dds_map_info(dir + file, dds) && !dds.isSRGB ? GFX_TEX_RGBA8_UNORM : GFX_TEX_RGBA8_SRGB;
            };
            if (!d.mapKd.empty()) m.texA = gfxh_scene_load_texture(s, (dir + d.mapKd).c_str(), colour_format(d.mapKd));
            if (!d.mapKs.empty()) m.texB = gfxh_scene_load_texture(s, (dir + d.mapKs).c_str(), simplePbr ? GFX_TEX_RGBA8_UNORM : colour_format(d.mapKs));
            if (simplePbr) {
                // MaterialConvention::SimplePBR (common_host.cpp:2323-2334, createSimplePBRMaterial :1689-1760): the diffuse slot
                // holds base colour (+ opacity) behind the sRGB sampler, the specular slot (occlusion, roughness, metallic) behind
                // the normalised-float sampler -- no degamma; no smoothness
                m.bsdfType = GFX_BSDF_SIMPLE_PBR;
                for (int i = 0; i < 3; ++i) m.b[i] = quantize8(d.ks[i]);
                m.smoothness = 0.0f;
            }
            const std::string& nmap = !d.mapBump.empty() ? d.mapBump : d.mapNormal;   // TEXTURE_HEIGHT first, then TEXTURE_NORMALS (:2278-2282)
            if (!nmap.empty()) {
                // getBumpMapType (common_host.cpp:890-904) picks the bump reader from the block format of a .dds map: BC1 / BC2 / BC3 /
                // BC7 -> normal map, BC4 -> height map, BC5 -> two-channel normal map; every other file is a three-channel normal map
                uint32_t format8 = GFX_TEX_RGBA8_UNORM, bumpType = GFX_BUMP_NORMAL_MAP;
                if (dds_map_info(dir + nmap, dds) && dds.isBlockCompressed) {
                    if (dds.bcFormat == GFX_BC4_UNORM || dds.bcFormat == GFX_BC4_SNORM) { format8 = GFX_TEX_R8_UNORM; bumpType = GFX_BUMP_HEIGHT_MAP; }
                    else if (dds.bcFormat == GFX_BC5_UNORM || dds.bcFormat == GFX_BC5_SNORM) { format8 = GFX_TEX_RG8_UNORM; bumpType = GFX_BUMP_NORMAL_MAP_2CH; }
                }
                m.texNormal = gfxh_scene_load_texture(s, (dir + nmap).c_str(), format8);
                m.bumpMapType = bumpType;
            }
            if (!d.mapKe.empty()) {
                m.texEmittance = gfxh_scene_load_texture(s, (dir + d.mapKe).c_str(), colour_format(d.mapKe));
                if (m.texEmittance) m.hasEmittance = 1u;
            }
        }
        const std::vector<Corner>& cs = facesByMat[name];
        Geom g; g.mat = matSlot;
        std::map<std::tuple<int, int, int>, uint32_t> dedup;   // aiProcess_JoinIdenticalVertices
        for (size_t f = 0; f + 2 < cs.size(); f += 3) {
            V3 fn = { 0, 0, 1 };
            bool needFaceNormal = cs[f].n < 0 || cs[f + 1].n < 0 || cs[f + 2].n < 0;
            if (needFaceNormal) fn = normalize(cross(pos[cs[f + 1].v] - pos[cs[f].v], pos[cs[f + 2].v] - pos[cs[f].v]));
            for (int k = 0; k < 3; ++k) {
                const Corner c = cs[f + k];
                const auto key = std::make_tuple(c.v, c.t, needFaceNormal ? -2 - static_cast<int>(f) : c.n);
                auto it = dedup.find(key);
                uint32_t vi;
                if (it != dedup.end()) vi = it->second;
                else {
                    const V3 n = normalize(needFaceNormal ? fn : nrm[c.n]);
                    const V3 tg = normalize(tangent_from_normal(n));
                    const float u = c.t >= 0 ? uv[c.t].first : 0.0f;
                    const float v = c.t >= 0 ? 1.0f - uv[c.t].second : 0.0f;   // aiProcess_FlipUVs
                    g.v.push_back(make_vertex(pos[c.v], n, tg, u, v));
                    vi = static_cast<uint32_t>(g.v.size() - 1);
                    dedup[key] = vi;
                }
                g.t.push_back(vi);
            }
        }
        // aiProcess_CalcTangentSpace (common_host.cpp:2163, 2346-2368: texCoord0Dir = aiMesh->mTangents when the mesh has texture
        // coordinates, the frame built from the normal otherwise): the tangent of a vertex is the direction in which u grows, dP/du of
        // its triangles -- (e1 dv2 - e2 dv1) / (du1 dv2 - du2 dv1), unchanged by the v flip above --, summed over the triangles that
        // share the vertex, made orthogonal to the normal.  Triangles without texture coordinates or with a degenerate mapping
        // contribute nothing; a vertex nothing contributed to keeps the frame built from its normal.
        {
            std::vector<V3> sum(g.v.size(), V3{ 0, 0, 0 });
            for (size_t f = 0; f + 2 < cs.size(); f += 3) {
                if (cs[f].t < 0 || cs[f + 1].t < 0 || cs[f + 2].t < 0) continue;
                const uint32_t i0 = g.t[f], i1 = g.t[f + 1], i2 = g.t[f + 2];
                const V3 e1 = pos[cs[f + 1].v] - pos[cs[f].v], e2 = pos[cs[f + 2].v] - pos[cs[f].v];
                const double du1 = static_cast<double>(uv[cs[f + 1].t].first) - uv[cs[f].t].first, du2 = static_cast<double>(uv[cs[f + 2].t].first) - uv[cs[f].t].first;
                const double dv1 = -(static_cast<double>(uv[cs[f + 1].t].second) - uv[cs[f].t].second), dv2 = -(static_cast<double>(uv[cs[f + 2].t].second) - uv[cs[f].t].second);
                const double det = du1 * dv2 - du2 * dv1;
                if (!(std::fabs(det) > 1e-20)) continue;
                V3 t = { static_cast<float>((e1.x * dv2 - e2.x * dv1) / det), static_cast<float>((e1.y * dv2 - e2.y * dv1) / det), static_cast<float>((e1.z * dv2 - e2.z * dv1) / det) };
                const float len = std::sqrt(t.x * t.x + t.y * t.y + t.z * t.z);
                if (!(len > 0.0f) || !std::isfinite(len)) continue;
                t = { t.x / len, t.y / len, t.z / len };
                for (uint32_t i : { i0, i1, i2 }) sum[i] = sum[i] + t;
            }
            for (size_t i = 0; i < g.v.size(); ++i) {
                const V3 n = { g.v[i].normal[0], g.v[i].normal[1], g.v[i].normal[2] };
                const float d = sum[i].x * n.x + sum[i].y * n.y + sum[i].z * n.z;
                const V3 t = { sum[i].x - n.x * d, sum[i].y - n.y * d, sum[i].z - n.z * d };
                const float len = std::sqrt(t.x * t.x + t.y * t.y + t.z * t.z);
                if (!(len > 1e-6f) || !std::isfinite(len)) continue;
                g.v[i].texCoord0Dir[0] = t.x / len; g.v[i].texCoord0Dir[1] = t.y / len; g.v[i].texCoord0Dir[2] = t.z / len;
            }
        }
        s->geoms.push_back(std::move(g));
        geomSlots.push_back(static_cast<uint32_t>(s->geoms.size() - 1));
    }
    if (geomSlots.empty()) { host_error() = std::string("no faces in ") + path; return 0xFFFFFFFFu; }
    return gfxh_scene_add_group(s, geomSlots.data(), static_cast<uint32_t>(geomSlots.size()));
}

} // extern "C"
