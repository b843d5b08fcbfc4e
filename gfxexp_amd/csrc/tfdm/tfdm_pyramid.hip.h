// tfdm_pyramid.hip.h -- the min-max pyramid kernels of a height map, shared by tfdm.hip and nrtdsm/nrtdsm.hip (each translation
// unit gets its own copy with internal linkage).  Included inside namespace gfx { namespace { ... } } after `using namespace tfdm`
// and displaced_object.h (HeightMapObject).
//
//   k_tfdm_minmax_first / k_tfdm_minmax_level   generateFirstMinMaxMipMap / generateMinMaxMipMap (tfdm_preprocess_kernels.cu:46-131),
//                                               launched level after level as tfdm_main.cpp:2492-2545 does
//   upload_height_map                           the host side of both: all levels (tfdm_build.h make_levels) to the device and
//                                               the pyramid over them
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

void upload_height_map(HeightMapObject& o, hipStream_t stream, const std::vector<float>& levels) {
    const int maxDepth = floor_log2(o.size);
    o.heights.reserve(sizeof(float) * levels.size());
    o.pyramid.reserve(sizeof(F2) * levels.size());
    GFX_HIP(hipMemcpyAsync(o.heights.p, levels.data(), sizeof(float) * levels.size(), hipMemcpyHostToDevice, stream));
    const uint32_t b0 = (o.size + 15u) / 16u;
    k_tfdm_minmax_first<<<dim3(b0, b0), 256, 0, stream>>>(o.heights.as<float>(), o.pyramid.as<F2>(), maxDepth);
    GFX_HIP(hipGetLastError());
    for (int l = 1; l <= maxDepth; ++l) {
        const uint32_t b = ((o.size >> l) + 15u) / 16u;
        k_tfdm_minmax_level<<<dim3(b, b), 256, 0, stream>>>(o.heights.as<float>(), o.pyramid.as<F2>(), maxDepth, l);
        GFX_HIP(hipGetLastError());
    }
    GFX_HIP(hipStreamSynchronize(stream));           // the caller's `levels` may go out of scope
}
