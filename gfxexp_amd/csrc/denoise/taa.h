// taa.h -- host-side state of the temporal anti-aliasing pass (taa.hip) behind gfx_taa_*.
#pragma once
#include "../internal.h"

namespace gfx {

struct TemporalAA {
    int device = 0;
    uint32_t width = 0, height = 0;
    uint32_t historyLength = 16;
    // history: [cur] is what the next call reprojects, the other one what it writes
    DevBuf history[2];
    uint32_t cur = 0;
};
constexpr uint32_t kTaaMaxHistoryLength = 256;       // the reference's slider, 2^0..2^8 (svgf_main.cpp:1798-1803)
void taa_init(TemporalAA& t, uint32_t width, uint32_t height, uint32_t historyLength);
void taa_release(TemporalAA& t);
void restir_copy_taa_flow_to_linear(Context& ctx, hipStream_t stream, void* flow);
void taa_apply(TemporalAA& t, hipStream_t stream, const void* color, const void* flow, bool isFirstFrame, void* out);

} // namespace gfx
