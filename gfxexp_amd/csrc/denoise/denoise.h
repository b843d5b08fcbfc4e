// denoise.h -- host-side state of the SVGF denoiser (denoise.hip) behind gfx_denoiser_* and gfx_restir_copy_depth_to_linear.
#pragma once
#include "../internal.h"

namespace gfx {

// ---- restir output chain: the depth and emissive guides
void restir_copy_depth_to_linear(Context& ctx, hipStream_t stream, void* depth);
void restir_copy_emissive_to_linear(Context& ctx, hipStream_t stream, void* emissive);
// ---- denoise.hip
struct Denoiser {
    int device = 0;
    uint32_t width = 0, height = 0;
    gfx_denoiser_settings st;
    // history: [k] for k = cur is what the next call reprojects, the other one what it writes
    DevBuf lighting[2], moments[2], length[2], guide[2];
    DevBuf lv[2];            // (lighting.rgb, variance) between the a-trous stages
    uint32_t cur = 0;
};
void denoiser_default_settings(gfx_denoiser_settings* out);
void denoiser_check_settings(const gfx_denoiser_settings& st);     // throws on invalid settings
void denoiser_init(Denoiser& d, uint32_t width, uint32_t height, const gfx_denoiser_settings& st);
void denoiser_release(Denoiser& d);
void denoise(Denoiser& d, hipStream_t stream, const gfx_denoiser_inputs& in, bool isFirstFrame, void* out);

} // namespace gfx
