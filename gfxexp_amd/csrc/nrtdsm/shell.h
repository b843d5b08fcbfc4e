// shell.h -- host-side state of a shell-mapped object (shell.hip) behind gfx_shell_*.
#pragma once
#include "../tfdm/displaced_object.h"
#include "shell_core.hip.h"

namespace gfx {

struct ShellObject : DisplacedObject {
    uint32_t numShellNodes = 0, numShellTriangles = 0;
    uint32_t numGeoms = 0;              // shell geometries of the current shell BVH: a renderer binds one material to each (tfdm/tfdm_set.hip)
    DevBuf shellNodes, shellTris;       // Node[numShellNodes], ShellTri[numShellTriangles]
    tfdm::Node root;                    // nodes[0] on the host and the generation of the buffers, as NrtdsmObject keeps them: what a
    uint64_t generation = 0;            // member of an instance set needs (tfdm/tfdm_set.hip)
    const char* lastChange = "gfx_shell_create";    // the call that made the buffers of this generation: a stale member's message names it
    ShellObject() : DisplacedObject("gfx_shell", sizeof(nrtdsm::PrismRecord)) {}
};

inline void displaced_release(ShellObject& o) {
    o.shellNodes.release(); o.shellTris.release();
    displaced_release(static_cast<DisplacedObject&>(o));
}

// the common items and the shell BVH on top
inline size_t displaced_size(const ShellObject& o, int what) {
    const DisplacedObject& base = o;
    switch (what) {
    case -1: return o.shellNodes.bytes + o.shellTris.bytes + displaced_size(base, -1);
    case GFX_SHELL_READ_SHELL_NODES: return sizeof(tfdm::Node) * o.numShellNodes;
    case GFX_SHELL_READ_SHELL_TRIANGLES: return sizeof(shell::ShellTri) * o.numShellTriangles;
    default: return displaced_size(base, what);
    }
}

inline void displaced_read(const ShellObject& o, int what, void* hostOut, size_t bytes) {
    if (what < 0) throw HipError("gfx_shell_read: unknown item");
    const size_t need = displaced_size(o, what);
    const void* src = what == GFX_SHELL_READ_SHELL_NODES ? o.shellNodes.p : what == GFX_SHELL_READ_SHELL_TRIANGLES ? o.shellTris.p : displaced_item(o, what);
    read_item(o, need, src, hostOut, bytes);
}

void shell_init(ShellObject& o, hipStream_t stream, const void* vertices, uint32_t stride, uint32_t numVertices, const uint32_t* triangles, uint32_t numTriangles,
                const gfx_shell_geom* geoms, uint32_t numGeoms, const gfx_tfdm_params& params);
void shell_set_params(ShellObject& o, hipStream_t stream, const gfx_tfdm_params& params);
void shell_set_geometry(ShellObject& o, hipStream_t stream, const gfx_shell_geom* geoms, uint32_t numGeoms);
void shell_trace(ShellObject& o, hipStream_t stream, int mode, const void* dRayOrgTmin, const void* dRayDirTmax, uint32_t numRays, void* dOut, void* dCounters);

} // namespace gfx
