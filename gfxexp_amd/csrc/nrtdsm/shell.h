// shell.h -- host-side state of a shell-mapped object (shell.hip) behind gfx_shell_*.
#pragma once
#include "../internal.h"
#include "shell_core.hip.h"

namespace gfx {

struct ShellObject {
    int device = 0;
    uint32_t numTriangles = 0, numNodes = 0, numShellNodes = 0, numShellTriangles = 0;
    gfx_tfdm_params pub;                // as the caller gave them
    tfdm::Params params;                // derived (shell_build.h make_shell_params)
    // host mirror of the base mesh: the records are made again when the parameters or the shell mesh change
    std::vector<float> positions, normals, texCoords;   // 9 / 9 / 6 floats per triangle, vertex order A B C
    DevBuf shellNodes, shellTris;       // Node[numShellNodes], ShellTri[numShellTriangles]
    DevBuf records, aabbs, nodes;       // PrismRecord[numTriangles], Box[numTriangles], Node[numNodes]
};

void shell_init(ShellObject& o, hipStream_t stream, const void* vertices, uint32_t stride, uint32_t numVertices, const uint32_t* triangles, uint32_t numTriangles,
                const gfx_shell_geom* geoms, uint32_t numGeoms, const gfx_tfdm_params& params);
void shell_set_params(ShellObject& o, hipStream_t stream, const gfx_tfdm_params& params);
void shell_set_geometry(ShellObject& o, hipStream_t stream, const gfx_shell_geom* geoms, uint32_t numGeoms);
void shell_release(ShellObject& o);
void shell_trace(ShellObject& o, hipStream_t stream, int mode, const void* dRayOrgTmin, const void* dRayDirTmax, uint32_t numRays, void* dOut, void* dCounters);
size_t shell_size(const ShellObject& o, int what);
void shell_read(ShellObject& o, int what, void* hostOut, size_t bytes);

} // namespace gfx
