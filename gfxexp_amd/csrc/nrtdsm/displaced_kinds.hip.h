// displaced_kinds.hip.h -- what a renderer adds to tfdm/displaced_surface.hip.h for a set with members of all three kinds
// (gfx_scene_bind_displaced_kinds).  A hit of an NRTDSM or a shell member has the fields of a TFDM member's
// (the reference's computeSurfacePoint treats every displaced kind alike, nrtdsm/nrtdsm_shared.h:653-695), so position, normal,
// tangent, texture coordinate and every G-buffer word but two are displaced_surface.hip.h's.  The two:
//   * the material.  A shell member has one per shell geometry, GeometryInstanceDataForNRTDSM::materialSlots[shellBvhGeomIndex]
//     (nrtdsm/gpu_kernels/optix_pathtracing_kernels.cu:134-139): shellMatSlots[8 k + shellGeom] of the binding's table for member k;
//     a member of another kind keeps the material of its bound geometry;
//   * gbuffer0.geomInstSlot = geomInstSlot | shellGeom << 28, the reference's 28 + 4 split of that word (nrtdsm/nrtdsm_shared.h:
//     132-140; its meshType is the kind word of the member's record here, reached through gbuffer0.instSlot).  shellGeom is the
//     shell part's (gfx_scene_shell_part), zero unless a shell member won, so the word of another member is its geometry slot.
// Shared by k_gbuffer_resolve_scene_shell (restir.hip), k_pt_first_scene_shell / k_pt_bounce_scene_shell (pathtrace.hip) and the
// tests (tests/displaced_kinds_host.cpp).  Plain C++17 under the math contract of tfdm_core.hip.h.
#pragma once
#include "../tfdm/displaced_surface.hip.h"

namespace gfx {
namespace tfdm {

constexpr uint32_t kShellMatsPerMember = 8;              // shell::kMaxGeoms: gfx_displaced_member::shellMatSlots
constexpr uint32_t kGeomSlotBits = 28;
constexpr uint32_t kGeomSlotMask = (1u << kGeomSlotBits) - 1u;
constexpr uint32_t kRecordKindShell = GFX_INSTANCE_SHELL;  // the kind word of a shell member's record (shell_instance.hip.h kKindShell)

// The material of a displaced hit on member k of `kind` (the kind word of its record): shellMats = the binding's table.  shellGeom
// is below 8 for every hit a shell BVH can give (shell_build.h refuses a ninth geometry); the mask keeps a word that is not inside
// the member's row.
GFX_TFDM_FN uint32_t displaced_material(uint32_t kind, uint32_t k, uint32_t shellGeom, const uint32_t* shellMats, uint32_t geomMaterialSlot) {
    if (kind != kRecordKindShell) return geomMaterialSlot;
    return shellMats[kShellMatsPerMember * k + (shellGeom & (kShellMatsPerMember - 1u))];
}

GFX_TFDM_FN uint32_t displaced_geom_word(uint32_t geomInstSlot, uint32_t shellGeom) { return geomInstSlot | (shellGeom << kGeomSlotBits); }
GFX_TFDM_FN uint32_t geom_word_slot(uint32_t word) { return word & kGeomSlotMask; }
GFX_TFDM_FN uint32_t geom_word_shell_geom(uint32_t word) { return word >> kGeomSlotBits; }

// displaced_gbuffer for a pixel of such a set: the same words, with the two above in their places
GFX_TFDM_FN DisplacedGBuffer displaced_gbuffer_kinds(const DisplacedPoint& p, const SceneHit& h, uint32_t geomInstSlot, uint32_t shellGeom, uint32_t matSlot,
                                                     const gfx_camera& prevCamera, int x, int y, float imageSizeX, float imageSizeY, bool resetFlow,
                                                     const float* curToPrev = nullptr) {
    DisplacedGBuffer g = displaced_gbuffer(p, h, geomInstSlot, matSlot, prevCamera, x, y, imageSizeX, imageSizeY, resetFlow, curToPrev);
    g.g0[1] = displaced_geom_word(geomInstSlot, shellGeom);
    return g;
}

} // namespace tfdm
} // namespace gfx
