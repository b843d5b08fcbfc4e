// bc_textures.h -- host-side state of block-compressed texture slots (gfx_texture_set_bc) and the expansion at scene upload.
//
// A block-compressed slot is a HostTexture with extent and the 8-bit format it is sampled as, and no texels: its blocks go to the
// device once, when the slot is set, and stay there.  Every rebuild of the texel pool (scene_upload) reserves the slot's region
// and expands the resident blocks into it on the upload's stream: no decoded texel crosses the bus, nothing is decoded on the CPU.
// The table of those block buffers is kept here, keyed by context.
#pragma once
#include <cstddef>
#include <cstdint>
#include <hip/hip_runtime.h>

namespace gfx {

struct Context;

// Copies the blocks of slot `texSlot` to the device (synchronous, set-up time) and remembers them; replaces earlier blocks of the slot.
// Throws and leaves the table as it was when the allocation or the copy fails.
void bc_texture_store(Context& ctx, uint32_t texSlot, uint32_t bcFormat, const void* blocks, size_t bytes);
// The slot holds uncompressed texels again (gfx_texture_set): drops its blocks, if any.
void bc_texture_forget(Context& ctx, uint32_t texSlot);
bool bc_texture_is(const Context& ctx, uint32_t texSlot);
// gfx_ctx_destroy: frees every block buffer of the context.
void bc_textures_drop(Context& ctx);
// Enqueues the expansion of slot `texSlot` into dTexels (the slot's region of the texel pool, 16-byte aligned, rows tightly packed
// in `format`, one of the four 8-bit gfx_tex_format values).
void bc_texture_expand(Context& ctx, hipStream_t stream, uint32_t texSlot, uint32_t width, uint32_t height, uint32_t format, void* dTexels);
// The same launch on caller-owned device memory (tools/bench_bc_expand.py measures it; dBlocks 16-byte aligned).
void bc_expand_launch(hipStream_t stream, uint32_t bcFormat, const void* dBlocks, uint32_t width, uint32_t height, uint32_t format, void* dTexels);

} // namespace gfx
