// tfdm_update.hip.h -- a height map changed in place: the kernels and the host side of gfx_tfdm_update_heights and
// gfx_nrtdsm_update_heights, shared by tfdm.hip and nrtdsm/nrtdsm.hip as tfdm_pyramid.hip.h is (each translation unit gets its own
// copy with internal linkage).  Included inside namespace gfx { namespace { ... } } after `using namespace tfdm`,
// displaced_object.h, tfdm_lds_stack.hip.h (wave_sum) and tfdm_pyramid.hip.h.  DESIGN.md section 25.
//
//   k_tfdm_update_check      the source rectangle's values: one lane per value, the refusals OR-ed over the wave, one atomic per wave
//   k_tfdm_update_copy       the rectangle into level 0 of the height map
//   k_tfdm_update_mean       a rectangle of level l >= 1 from level l - 1, make_levels' ((a + b) + (c + d)) * 0.25f
//   k_tfdm_update_minmax     a wrapped rectangle of pyramid level l: texel_min_max / pyramid_reduce, as k_tfdm_minmax_* over a level
//   k_tfdm_count_boxes       how many per-triangle boxes are not empty
//   k_tfdm_refit_depth       one depth of the tree, one node per lane (tfdm_update.h refit_node)
//   k_tfdm_refit_top         the depths that fit one block, deepest first, by one block with a barrier between two depths
//
// The regions are tfdm_update.h's (dirty_levels).  Every kernel is plain C++: no lane of them reads what another block of the
// same launch writes, and the order between launches is the stream's.
constexpr uint32_t kUpdateNonFinite = 1u, kUpdateOutOfRange = 2u;      // flag word 0 (k_tfdm_update_check)
constexpr int kFlagValues = 0, kFlagNonEmpty = 1, kFlagEmptyLeaf = 2, kNumUpdateFlags = 8;
constexpr uint32_t kRefitBlock = 256;

__global__ void __launch_bounds__(256) k_tfdm_update_check(const float* __restrict__ src, uint32_t pitch, uint32_t w, uint32_t h, uint32_t unitRange, uint32_t* flags) {
    const uint32_t i = blockIdx.x * 16u + (threadIdx.x & 15u), j = blockIdx.y * 16u + (threadIdx.x >> 4);
    uint32_t bad = 0u;
    if (i < w && j < h) {
        const float v = src[static_cast<size_t>(j) * pitch + i];
        if (!(fabsf(v) < inf())) bad = kUpdateNonFinite;
        else if (unitRange != 0u && !(v >= 0.0f && v <= 1.0f)) bad = kUpdateOutOfRange;
    }
    for (int off = 32; off > 0; off >>= 1) bad |= __shfl_down(bad, off, 64);       // every lane of the wave is here
    if ((threadIdx.x & 63u) == 0u && bad != 0u) atomicOr(flags + kFlagValues, bad);
}

__global__ void __launch_bounds__(256) k_tfdm_update_copy(const float* __restrict__ src, uint32_t pitch, float* __restrict__ heights, uint32_t size, uint32_t x0, uint32_t y0,
                                                          uint32_t w, uint32_t h) {
    const uint32_t i = blockIdx.x * 16u + (threadIdx.x & 15u), j = blockIdx.y * 16u + (threadIdx.x >> 4);
    if (i >= w || j >= h) return;
    heights[static_cast<size_t>(y0 + j) * size + (x0 + i)] = src[static_cast<size_t>(j) * pitch + i];
}

__global__ void __launch_bounds__(256) k_tfdm_update_mean(float* heights, int maxDepth, int level, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h) {
    const uint32_t i = blockIdx.x * 16u + (threadIdx.x & 15u), j = blockIdx.y * 16u + (threadIdx.x >> 4);
    if (i >= w || j >= h) return;
    const uint32_t lw = 1u << (maxDepth - level), x = x0 + i, y = y0 + j;
    const float* s = heights + level_offset(maxDepth, level - 1);
    const float a = s[(2u * y) * 2u * lw + 2u * x], b = s[(2u * y) * 2u * lw + 2u * x + 1u];
    const float c = s[(2u * y + 1u) * 2u * lw + 2u * x], d = s[(2u * y + 1u) * 2u * lw + 2u * x + 1u];
    heights[level_offset(maxDepth, level) + y * lw + x] = ((a + b) + (c + d)) * 0.25f;
}

__global__ void __launch_bounds__(256) k_tfdm_update_minmax(const float* __restrict__ heights, F2* pyramid, int maxDepth, int level, uint32_t x0, uint32_t y0, uint32_t w,
                                                            uint32_t h) {
    const uint32_t i = blockIdx.x * 16u + (threadIdx.x & 15u), j = blockIdx.y * 16u + (threadIdx.x >> 4);
    if (i >= w || j >= h) return;
    const uint32_t lw = 1u << (maxDepth - level);
    const int x = static_cast<int>((x0 + i) & (lw - 1u)), y = static_cast<int>((y0 + j) & (lw - 1u));
    const F2 r = level == 0 ? texel_min_max(heights, maxDepth, 0, x, y) : pyramid_reduce(heights, pyramid, maxDepth, level, x, y);
    pyramid[level_offset(maxDepth, level) + static_cast<uint32_t>(y) * lw + static_cast<uint32_t>(x)] = r;
}

__global__ void __launch_bounds__(256) k_tfdm_count_boxes(const float* __restrict__ aabbs, uint32_t numTriangles, uint32_t* flags) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t n = wave_sum(i < numTriangles && !box_is_empty(aabbs + 6u * static_cast<size_t>(i)) ? 1u : 0u);
    if ((threadIdx.x & 63u) == 0u && n != 0u) atomicAdd(flags + kFlagNonEmpty, n);
}

__global__ void __launch_bounds__(kRefitBlock) k_tfdm_refit_depth(Node* nodes, const float* __restrict__ aabbs, const uint32_t* __restrict__ order, uint32_t count,
                                                                  uint32_t* flags) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i >= count) return;
    if (!refit_node(nodes, order[i], aabbs)) flags[kFlagEmptyLeaf] = 1u;
}

struct RefitTop { uint32_t offset[kMaxTreeLevels + 1]; int deepest; };      // depths deepest .. 0, each of at most kRefitBlock nodes

__global__ void __launch_bounds__(kRefitBlock) k_tfdm_refit_top(Node* nodes, const float* __restrict__ aabbs, const uint32_t* __restrict__ order, RefitTop top, uint32_t* flags) {
    for (int d = top.deepest; d >= 0; --d) {
        const uint32_t i = top.offset[d] + threadIdx.x;
        if (i < top.offset[d + 1] && !refit_node(nodes, order[i], aabbs)) flags[kFlagEmptyLeaf] = 1u;
        __syncthreads();            // the next depth reads these nodes: same block, so the barrier orders them
    }
}

inline dim3 tiles16(uint32_t w, uint32_t h) { return dim3((w + 15u) / 16u, (h + 15u) / 16u); }

// The scratch of an update and the level table of the current tree.  Allocates at the first update and reads the tree back once
// per generation; nothing of the object has changed when this throws.
void prepare_update(HeightMapObject& o, hipStream_t stream) {
    o.updateFlags.reserve(sizeof(uint32_t) * kNumUpdateFlags);
    if (!o.updateHost) GFX_HIP(hipHostMalloc(&o.updateHost, sizeof(uint32_t) * kNumUpdateFlags + sizeof(Node)));
    if (o.levelTableValid) return;
    std::vector<Node> tree(o.numNodes);
    GFX_HIP(hipMemcpyAsync(tree.data(), o.nodes.p, sizeof(Node) * o.numNodes, hipMemcpyDeviceToHost, stream));
    GFX_HIP(hipMemsetAsync(o.updateFlags.p, 0, sizeof(uint32_t) * kNumUpdateFlags, stream));
    k_tfdm_count_boxes<<<(o.numTriangles + 255u) / 256u, 256, 0, stream>>>(o.aabbs.as<float>(), o.numTriangles, o.updateFlags.as<uint32_t>());
    GFX_HIP(hipGetLastError());
    GFX_HIP(hipMemcpyAsync(o.updateHost, o.updateFlags.p, sizeof(uint32_t) * kNumUpdateFlags, hipMemcpyDeviceToHost, stream));
    GFX_HIP(hipStreamSynchronize(stream));
    if (!make_level_table(tree.data(), o.numNodes, o.levelTable)) throw HipError(std::string(o.name) + "_update_heights: the object's tree is deeper than a refit supports");
    o.levelOrder.reserve(sizeof(uint32_t) * o.numNodes);
    GFX_HIP(hipMemcpy(o.levelOrder.p, o.levelTable.order.data(), sizeof(uint32_t) * o.numNodes, hipMemcpyHostToDevice));
    o.numNonEmpty = static_cast<const uint32_t*>(o.updateHost)[kFlagNonEmpty];
    o.levelTableValid = true;
}

// `launchPrim()` runs the query's per-triangle kernel over all triangles on the object's own records and boxes.  Returns true
// with `root` the refitted root; false when a primitive's box became empty or stopped being empty, so that the tree's shape is not
// a fresh build's any more: heights, pyramid, records and boxes are the new ones then, and the caller makes the tree again
// (rebuild).  `canRefit` false: the caller knows that already (it will rebuild whatever comes out), so only heights and pyramid
// are made.  `timing`: the context whose timing (gfx_timing_enable) gets the four phases of the call.
template <typename LaunchPrim>
bool update_heights(Context& timing, HeightMapObject& o, hipStream_t stream, const float* dSrc, uint32_t srcPitch, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                    bool unitRange, bool canRefit, LaunchPrim launchPrim, Node& root) {
    const std::string who = std::string(o.name) + "_update_heights: ";
    if (!dSrc || (reinterpret_cast<uintptr_t>(dSrc) & 3u)) throw HipError(who + "the source is null or not 4-byte aligned");
    if (w == 0u || h == 0u) throw HipError(who + "the rectangle is empty");
    if (srcPitch < w) throw HipError(who + "srcPitch is smaller than the rectangle's width");
    if (static_cast<uint64_t>(x0) + w > o.size || static_cast<uint64_t>(y0) + h > o.size) throw HipError(who + "the rectangle leaves the map (it does not wrap)");
    if (o.ownMips)
        throw HipError(who + "the object was created with its own mip levels; their coarser levels are not means of the finer ones, so a region of them cannot be made again");
    prepare_update(o, stream);
    uint32_t* dFlags = o.updateFlags.as<uint32_t>();
    uint32_t* hFlags = static_cast<uint32_t*>(o.updateHost);
    {
        ScopedKernelTimer timer(timing, stream, "tfdm_update_check");
        GFX_HIP(hipMemsetAsync(dFlags, 0, sizeof(uint32_t) * kNumUpdateFlags, stream));
        k_tfdm_update_check<<<tiles16(w, h), 256, 0, stream>>>(dSrc, srcPitch, w, h, unitRange ? 1u : 0u, dFlags);
        GFX_HIP(hipGetLastError());
        GFX_HIP(hipMemcpyAsync(hFlags, dFlags, sizeof(uint32_t) * kNumUpdateFlags, hipMemcpyDeviceToHost, stream));
    }
    GFX_HIP(hipStreamSynchronize(stream));
    if (hFlags[kFlagValues] & kUpdateNonFinite) throw HipError(who + "a source value is not finite");
    if (hFlags[kFlagValues] & kUpdateOutOfRange) throw HipError(who + "a source value lies outside [0, 1] (the descent clips the map value to that range)");

    // ---- from here on the object changes
    const int maxDepth = o.params.maxDepth;
    float* heights = o.heights.as<float>();
    F2* pyramid = o.pyramid.as<F2>();
    {
        ScopedKernelTimer timer(timing, stream, "tfdm_update_pyramid");
        const std::vector<DirtyLevel> dirty = dirty_levels(maxDepth, x0, y0, w, h);
        k_tfdm_update_copy<<<tiles16(w, h), 256, 0, stream>>>(dSrc, srcPitch, heights, o.size, x0, y0, w, h);
        GFX_HIP(hipGetLastError());
        for (int l = 1; l <= maxDepth; ++l) {
            const DirtyLevel& d = dirty[l];
            k_tfdm_update_mean<<<tiles16(d.hx.len, d.hy.len), 256, 0, stream>>>(heights, maxDepth, l, d.hx.start, d.hy.start, d.hx.len, d.hy.len);
            GFX_HIP(hipGetLastError());
        }
        for (int l = 0; l <= maxDepth; ++l) {
            const DirtyLevel& d = dirty[l];
            k_tfdm_update_minmax<<<tiles16(d.px.len, d.py.len), 256, 0, stream>>>(heights, pyramid, maxDepth, l, d.px.start, d.py.start, d.px.len, d.py.len);
            GFX_HIP(hipGetLastError());
        }
    }
    if (!canRefit) return false;
    {
        ScopedKernelTimer timer(timing, stream, "tfdm_update_prim");
        launchPrim();
        GFX_HIP(hipGetLastError());
        k_tfdm_count_boxes<<<(o.numTriangles + 255u) / 256u, 256, 0, stream>>>(o.aabbs.as<float>(), o.numTriangles, dFlags);
        GFX_HIP(hipGetLastError());
    }
    {
        ScopedKernelTimer timer(timing, stream, "tfdm_update_refit");
        const LevelTable& t = o.levelTable;
        const uint32_t* order = o.levelOrder.as<uint32_t>();
        int top = 0;                   // the depths 0 .. top have at most kRefitBlock nodes each
        while (top + 1 < t.numLevels && t.offset[top + 2] - t.offset[top + 1] <= kRefitBlock) ++top;
        for (int d = t.numLevels - 1; d > top; --d) {
            const uint32_t count = t.offset[d + 1] - t.offset[d];
            k_tfdm_refit_depth<<<(count + kRefitBlock - 1u) / kRefitBlock, kRefitBlock, 0, stream>>>(o.nodes.as<Node>(), o.aabbs.as<float>(), order + t.offset[d], count, dFlags);
            GFX_HIP(hipGetLastError());
        }
        RefitTop rt;
        for (int d = 0; d <= kMaxTreeLevels; ++d) rt.offset[d] = t.offset[d];
        rt.deepest = top;
        k_tfdm_refit_top<<<1, kRefitBlock, 0, stream>>>(o.nodes.as<Node>(), o.aabbs.as<float>(), order, rt, dFlags);
        GFX_HIP(hipGetLastError());
        GFX_HIP(hipMemcpyAsync(hFlags, dFlags, sizeof(uint32_t) * kNumUpdateFlags, hipMemcpyDeviceToHost, stream));
        GFX_HIP(hipMemcpyAsync(hFlags + kNumUpdateFlags, o.nodes.p, sizeof(Node), hipMemcpyDeviceToHost, stream));
    }
    GFX_HIP(hipStreamSynchronize(stream));
    // the one-node tree over only-empty boxes has one leaf, which keeps its box
    const bool nothingTree = o.numNodes == 1u && o.numNonEmpty == 0u;
    const bool sameShape = hFlags[kFlagNonEmpty] == o.numNonEmpty && (nothingTree || hFlags[kFlagEmptyLeaf] == 0u);
    if (!sameShape) return false;
    std::memcpy(&root, hFlags + kNumUpdateFlags, sizeof(Node));
    return true;
}
