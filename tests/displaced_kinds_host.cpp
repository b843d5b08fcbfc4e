// displaced_kinds_host.cpp -- the host compilation of gfxexp_amd/csrc/nrtdsm/displaced_kinds.hip.h behind a C interface
// (tests/displaced_kinds_host.py compiles it into a directory the test provides), next to tests/displaced_host.cpp.  The same text
// hipcc compiles for the shell-aware renderer kernels, so the GPU tests compare with it bit for bit.
#include <cstdint>
#include "nrtdsm/displaced_kinds.hip.h"

using namespace gfx::tfdm;

extern "C" {

uint32_t displaced_kinds_host_sizeof(int what) {
    return what == 0 ? sizeof(InstanceRecord) : what == 1 ? sizeof(gfx_scene_hit) : what == 2 ? sizeof(gfx_camera) : what == 3 ? sizeof(gfx_scene_shell_part)
                                                                                                                               : sizeof(gfx_displaced_member);
}
uint32_t displaced_kinds_host_constant(int what) { return what == 0 ? kShellMatsPerMember : what == 1 ? kGeomSlotBits : what == 2 ? kGeomSlotMask : kRecordKindShell; }

// n independent choices: kind, member, shellGeom, the bound geometry's material
void displaced_kinds_host_material(const uint32_t* kind, const uint32_t* member, const uint32_t* shellGeom, const uint32_t* geomMat, const uint32_t* shellMats, uint32_t n,
                                   uint32_t* out) {
    for (uint32_t i = 0; i < n; ++i) out[i] = displaced_material(kind[i], member[i], shellGeom[i], shellMats, geomMat[i]);
}

void displaced_kinds_host_word(const uint32_t* slot, const uint32_t* shellGeom, uint32_t n, uint32_t* word, uint32_t* slotBack, uint32_t* geomBack) {
    for (uint32_t i = 0; i < n; ++i) {
        word[i] = displaced_geom_word(slot[i], shellGeom[i]);
        slotBack[i] = geom_word_slot(word[i]);
        geomBack[i] = geom_word_shell_geom(word[i]);
    }
}

// displaced_host_resolve (tests/displaced_host.cpp) for a set of all kinds: the material is chosen here from the record's kind word,
// the shell part and the two tables of the binding (geomSlots[k], geomMats[k] = the bound geometry's material, shellMats[8 k + g]);
// curToPrev: 12 floats per member, or null.  mats: the material chosen per hit.
void displaced_kinds_host_resolve(const InstanceRecord* table, const gfx_scene_hit* hits, const gfx_scene_shell_part* parts, const float* orgTmin, const float* dirTmax,
                                  const float* baseVerts, const uint32_t* geomSlots, const uint32_t* geomMats, const uint32_t* shellMats, const float* curToPrev,
                                  const int32_t* xy, uint32_t n, const gfx_camera* prevCamera, float imageSizeX, float imageSizeY, int resetFlow, float* points,
                                  uint32_t* g0, float* g1, uint32_t* g2, uint32_t* g3, uint32_t* mats, int plainForm) {
    for (uint32_t i = 0; i < n; ++i) {
        SceneHit h;
        h.dist = hits[i].dist; h.bcB = hits[i].bcB; h.bcC = hits[i].bcC; h.index = hits[i].index;
        h.normal = v3(hits[i].normal[0], hits[i].normal[1], hits[i].normal[2]); h.where = hits[i].where;
        const uint32_t k = h.where >> 1;
        BaseVertex v[3];
        for (int c = 0; c < 3; ++c) {
            const float* f = baseVerts + 15 * i + 5 * c;
            v[c].texCoord0Dir = v3(f[0], f[1], f[2]); v[c].u = f[3]; v[c].v = f[4];
        }
        const DisplacedPoint p = displaced_point(table[k], h, v3(orgTmin[4 * i], orgTmin[4 * i + 1], orgTmin[4 * i + 2]),
                                                 v3(dirTmax[4 * i], dirTmax[4 * i + 1], dirTmax[4 * i + 2]), v[0], v[1], v[2]);
        float* o = points + 11 * i;
        o[0] = p.position.x; o[1] = p.position.y; o[2] = p.position.z; o[3] = p.normal.x; o[4] = p.normal.y; o[5] = p.normal.z;
        o[6] = p.tangent.x; o[7] = p.tangent.y; o[8] = p.tangent.z; o[9] = p.u; o[10] = p.v;
        const uint32_t mat = displaced_material(table[k].pad0, k, parts[i].shellGeom, shellMats, geomMats[k]);
        mats[i] = mat;
        const float* m = curToPrev ? curToPrev + 12 * k : nullptr;
        // plainForm: displaced_gbuffer itself with the same arguments, for the byte comparison of the words the two share
        const DisplacedGBuffer g = plainForm ? displaced_gbuffer(p, h, geomSlots[k], mat, *prevCamera, xy[2 * i], xy[2 * i + 1], imageSizeX, imageSizeY, resetFlow != 0, m)
                                             : displaced_gbuffer_kinds(p, h, geomSlots[k], parts[i].shellGeom, mat, *prevCamera, xy[2 * i], xy[2 * i + 1], imageSizeX,
                                                                       imageSizeY, resetFlow != 0, m);
        for (int c = 0; c < 4; ++c) { g0[4 * i + c] = g.g0[c]; g3[4 * i + c] = g.g3[c]; }
        g1[2 * i] = g.mv[0]; g1[2 * i + 1] = g.mv[1];
        for (int c = 0; c < 3; ++c) g2[4 * i + c] = f2b(g.position[c]);
        g2[4 * i + 3] = g.qGeometricNormal;
    }
}

} // extern "C"
