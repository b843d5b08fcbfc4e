"""Rate of the block-compressed texture expansion (gfx_texture_set_bc's upload-time kernels, csrc/bc/bc_expand.hip): for each BC
format a 4096 x 4096 texture of random blocks expanded into RGBA8 (and BC4 -> R8, BC5 -> RG8), HIP events around `--iters`
expansions after a warm-up.  One JSON line: microseconds per expansion, GB/s of blocks read plus texels written, and that rate as
a fraction of the box's streaming-copy rate (gfx_stream_copy on 1 GiB, read + write bytes), taken in the same process.

    python tools/bench_bc_expand.py [--size 4096] [--iters 20]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gfxexp_amd import api  # noqa: E402

CASES = [("BC1", api.BC1, api.TEX_RGBA8_UNORM), ("BC2", api.BC2, api.TEX_RGBA8_UNORM), ("BC3", api.BC3, api.TEX_RGBA8_UNORM),
         ("BC4_UNORM", api.BC4_UNORM, api.TEX_RGBA8_UNORM), ("BC4_SNORM", api.BC4_SNORM, api.TEX_RGBA8_UNORM),
         ("BC5_UNORM", api.BC5_UNORM, api.TEX_RGBA8_UNORM), ("BC5_SNORM", api.BC5_SNORM, api.TEX_RGBA8_UNORM), ("BC7", api.BC7, api.TEX_RGBA8_UNORM),
         ("BC4_UNORM->R8", api.BC4_UNORM, api.TEX_R8_UNORM), ("BC4_SNORM->R8", api.BC4_SNORM, api.TEX_R8_UNORM),
         ("BC5_UNORM->RG8", api.BC5_UNORM, api.TEX_RG8_UNORM), ("BC5_SNORM->RG8", api.BC5_SNORM, api.TEX_RG8_UNORM)]


def timed(fn, iters, warmup=3):
    """Seconds per call: HIP events around `iters` calls on the current stream."""
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def main(argv):
    size = int(argv[argv.index("--size") + 1]) if "--size" in argv else 4096
    iters = int(argv[argv.index("--iters") + 1]) if "--iters" in argv else 20
    ctx = api.Context(0)
    stream = torch.cuda.current_stream().cuda_stream
    n = 1 << 30
    src = torch.empty(n, dtype=torch.uint8, device="cuda")
    dst = torch.empty(n, dtype=torch.uint8, device="cuda")
    src.fill_(1)
    copy_rate = 2 * n / timed(lambda: ctx.stream_copy(dst.data_ptr(), src.data_ptr(), n, stream), 10)
    del src, dst
    torch.cuda.empty_cache()
    out = {"metric": "bc_expand", "size": size, "iters": iters, "stream_copy_GBps": round(copy_rate / 1e9, 1), "formats": {}}
    rng = np.random.default_rng(1)
    num_blocks = (size // 4) ** 2
    for name, bc, fmt in CASES:
        block_bytes, texel_bytes = num_blocks * api.BC_BLOCK_BYTES[bc], size * size * api.TEX_BYTES_PER_TEXEL[fmt]
        blocks = torch.from_numpy(rng.integers(0, 256, block_bytes, dtype=np.uint8)).cuda()
        texels = torch.empty(texel_bytes, dtype=torch.uint8, device="cuda")
        secs = timed(lambda: ctx.bc_expand(bc, blocks.data_ptr(), size, size, fmt, texels.data_ptr(), stream), iters)
        rate = (block_bytes + texel_bytes) / secs
        out["formats"][name] = {"us": round(secs * 1e6, 1), "GBps": round(rate / 1e9, 1), "of_stream_copy": round(rate / copy_rate, 3)}
        del blocks, texels
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
