// tex_format.h -- bytes per texel of a gfx_tex_format value, 0 for an unknown one: the one definition that the scene container
// (scene_builder.cpp) and the context's texture slots (capi.cpp) share.
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../../include/gfxexp.h"

namespace gfx {
inline size_t tex_bytes_per_texel(uint32_t format) {
    switch (format) {
    case GFX_TEX_RGBA8_SRGB: case GFX_TEX_RGBA8_UNORM: return 4;
    case GFX_TEX_R8_UNORM: return 1;
    case GFX_TEX_RG8_UNORM: return 2;
    case GFX_TEX_RGBA32F: return 16;
    default: return 0;
    }
}
} // namespace gfx
