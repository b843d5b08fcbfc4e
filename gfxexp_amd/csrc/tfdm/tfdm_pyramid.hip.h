// tfdm_pyramid.hip.h -- the min-max pyramid kernels of a height map, shared by tfdm.hip and nrtdsm/nrtdsm.hip (each translation
// unit gets its own copy with internal linkage).  Included inside namespace gfx { namespace { ... } } after `using namespace tfdm`.
//
//   k_tfdm_minmax_first / k_tfdm_minmax_level   generateFirstMinMaxMipMap / generateMinMaxMipMap (tfdm_preprocess_kernels.cu:46-131),
//                                               launched level after level as tfdm_main.cpp:2492-2545 does
__global__ void __launch_bounds__(256) k_tfdm_minmax_first(const float* __restrict__ heights, F2* __restrict__ pyramid, int maxDepth) {
    const int w = 1 << maxDepth;
    const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= w || y >= w) return;
    pyramid[y * w + x] = texel_min_max(heights, maxDepth, 0, x, y);
}

__global__ void __launch_bounds__(256) k_tfdm_minmax_level(const float* __restrict__ heights, F2* pyramid, int maxDepth, int level) {
    const int w = 1 << (maxDepth - level);
    const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= w || y >= w) return;
    pyramid[level_offset(maxDepth, level) + static_cast<uint32_t>(y * w + x)] = pyramid_reduce(heights, pyramid, maxDepth, level, x, y);
}
