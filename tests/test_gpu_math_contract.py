"""-m gpu: the device copy of the deterministic math contract (gfxexp_amd/csrc/gm_math.hip.h) and of the 16-bit quantisers
(shading.hip.h), run by the inspection entry gfx_math_eval, against the CPU oracle, bit for bit, on the lists of
tests/math_cases.py.  tests/test_math_contract_cpu.py holds the oracle against float64, so equality here puts the kernels' own
functions under those bounds too.

One rule differs from util.assert_same_bits: a float word passes when both sides are NaN (sign and payload of a NaN are not part of
the contract: x86 produces -nan where the GPU produces +nan), and the number of NaN words must be the one the CPU test recorded
for the list (math_cases.NAN_WORDS), so a device that turns numbers into NaNs still fails.  Inputs the host code has no defined
result for (gm_exp outside its domain, gm_sincos at |x| >= 2^31 pi/2) are not in the lists; see tests/math_cases.py."""
import functools

import numpy as np
import pytest

from gfxexp_amd import api
from oracle import oracle as O
from tests import math_cases as MC

pytestmark = pytest.mark.gpu
F, U = np.float32, np.uint32
CASES = [(fn, name) for fn, lists in MC.GPU_LISTS.items() for name in lists]


@functools.lru_cache(maxsize=None)
def context():
    return api.Context(0)


@pytest.fixture(scope="module", autouse=True)
def leave_the_gpu_as_found():
    """The lists are large: when the module is done, its context goes and the memory goes back to the driver, so the tests that
    follow meet the device as they would without this module."""
    yield
    import gc
    import torch
    if context.cache_info().currsize:
        context().close()
        context.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def fn_id(fn):
    return getattr(api, "MATH_" + fn)


def gpu_eval(fn, A, B=None, stream=None):
    """gfx_math_eval once on (A, B): uint32 [4, n]."""
    import torch
    n = len(A)
    s = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(s):
        d_a = torch.from_numpy(A).cuda()
        d_b = torch.from_numpy(B).cuda() if B is not None else None
        d_out = torch.full((4 * n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        context().math_eval(fn_id(fn), d_a.data_ptr(), n, d_out.data_ptr(), d_b.data_ptr() if B is not None else 0, stream=s.cuda_stream)
        s.synchronize()
        return d_out.cpu().numpy().view(U).reshape(4, n)


def assert_parity(what, fn, got, want, A):
    for k in range(4):
        if k >= len(want):
            assert not np.any(got[k]), f"{what}: unused result word {k} is not 0"
            continue
        bad = got[k] != want[k]
        if k < MC.FLOAT_WORDS[fn]:
            bad &= ~(np.isnan(got[k].view(F)) & np.isnan(want[k].view(F)))
        if np.any(bad):
            i = int(np.flatnonzero(bad)[0])
            raise AssertionError(f"{what}: word {k} differs on {np.count_nonzero(bad)} of {len(bad)} elements, first at {i}: argument "
                                 f"{A[i]!r} (bits {[hex(b) for b in A[i].view(U)]}), device {int(got[k][i]):#010x}, oracle {int(want[k][i]):#010x}")


@pytest.mark.parametrize("fn,name", CASES, ids=[f"{fn}-{name}" for fn, name in CASES])
def test_device_equals_oracle(built_lib, fn, name):
    A, B = MC.GPU_LISTS[fn][name]()
    assert 0 < len(A) <= 1 << 24
    got = gpu_eval(fn, A, B)
    want = MC.oracle_words(fn, A, B)
    assert_parity(f"{fn} on {name}", fn, got, want, A)
    assert MC.nan_words(fn, list(got)) == MC.NAN_WORDS[(fn, name)]


@pytest.mark.parametrize("n", [1, 255, 257, 1000 + 37])
def test_lengths_off_the_block_size(built_lib, n):
    """A list that is no multiple of the 256-thread block, and a single element: every element is written, nothing past the end."""
    import torch
    A = MC.a4(MC.unary_edges()[5000:5000 + n])
    d_a = torch.from_numpy(A).cuda()
    d_out = torch.full((4 * n + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    context().math_eval(api.MATH_SINCOS, d_a.data_ptr(), n, d_out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(U)
    assert np.all(out[4 * n:] == 0x5A5A5A5A)
    assert_parity(f"SINCOS n = {n}", "SINCOS", out[:4 * n].reshape(4, n), MC.oracle_words("SINCOS", A), A)


def test_a_second_stream_reproduces_the_first(built_lib):
    import torch
    p = MC.atan2_pairs()[:100003]
    A = MC.a4(p[:, 0], p[:, 1])
    first = gpu_eval("ATAN2", A)
    second = gpu_eval("ATAN2", A, stream=torch.cuda.Stream())
    assert np.array_equal(first, second)
    assert_parity("ATAN2 on a second stream", "ATAN2", second, MC.oracle_words("ATAN2", A), A)


def test_refusals_launch_nothing(built_lib):
    import torch
    ctx = context()
    n = 64
    d_a = torch.zeros(4 * n + 4, dtype=torch.float32, device="cuda")
    d_out = torch.full((4 * n + 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    a, o = d_a.data_ptr(), d_out.data_ptr()
    with pytest.raises(api.GfxError, match="unknown fn"):
        ctx.math_eval(13, a, n, o)
    with pytest.raises(api.GfxError, match="unknown fn"):
        ctx.math_eval(-1, a, n, o)
    with pytest.raises(api.GfxError, match="must not be null"):
        ctx.math_eval(api.MATH_EXP, 0, n, o)
    with pytest.raises(api.GfxError, match="must not be null"):
        ctx.math_eval(api.MATH_EXP, a, n, 0)
    with pytest.raises(api.GfxError, match="second argument buffer"):
        ctx.math_eval(api.MATH_OFFSET_RAY_ORIGIN, a, n, o)
    with pytest.raises(api.GfxError, match="16-byte aligned"):
        ctx.math_eval(api.MATH_EXP, a + 4, n, o)
    with pytest.raises(api.GfxError, match="16-byte aligned"):
        ctx.math_eval(api.MATH_EXP, a, n, o + 8)
    with pytest.raises(api.GfxError, match="16-byte aligned"):
        ctx.math_eval(api.MATH_OFFSET_RAY_ORIGIN, a, n, o, d_b=a + 4)
    ctx.math_eval(api.MATH_EXP, 0, 0, 0)                                  # n == 0: nothing to do, nothing touched
    torch.cuda.synchronize()
    assert torch.all(d_out == 0x5A5A5A5A)
    ctx.math_eval(api.MATH_EXP, a, n, o)                                  # and the accepted call does write: exp(0) = 1
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(U)
    assert np.all(out[:n] == 0x3F800000) and np.all(out[n:4 * n] == 0) and np.all(out[4 * n:] == 0x5A5A5A5A)


def test_decode_to_polar_encode_chain_on_the_device(built_lib):
    """decode_dir -> to_polar_yup / encode_dir with the device's own intermediate values never leaving it: the codes that come
    back are those of the same chain on the oracle."""
    import torch
    q = MC.dir_codes_edges()
    n = len(q)
    ctx, s = context(), torch.cuda.current_stream().cuda_stream
    d_a = torch.from_numpy(MC.codes_a4(q)).cuda()
    d_dir = torch.zeros(4 * n, dtype=torch.int32, device="cuda")
    ctx.math_eval(api.MATH_DECODE_DIR, d_a.data_ptr(), n, d_dir.data_ptr(), stream=s)
    d_v = d_dir.view(4, n).t().contiguous()                              # (x, y, z, 0) per element, as bits
    d_out = torch.zeros(4 * n, dtype=torch.int32, device="cuda")
    ctx.math_eval(api.MATH_TO_POLAR, d_v.data_ptr(), n, d_out.data_ptr(), stream=s)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(U).reshape(4, n)
    v = O.decode_normal(q)
    phi, theta = O.to_polar(v)
    assert_parity("decode -> to_polar -> encode", "TO_POLAR", got, [phi.view(U), theta.view(U), O.encode_normal(v)], MC.codes_a4(q))


def test_host_table_uses_the_same_sincos(built_lib):
    """gfxh_spatial_neighbor_deltas (host/env_tables.cpp, the third copy of the sincos) equals r (cos, sin) with the device's gm_sincos."""
    r, theta = MC.neighbor_delta_polar()
    got = gpu_eval("SINCOS", MC.a4(theta))
    s, c = got[0].view(F), got[1].view(F)
    want = api.spatial_neighbor_deltas()
    mine = np.stack([r * c, r * s], axis=1)
    mine[r == 0] = 0
    assert np.array_equal(mine.view(U), want.view(U)), f"{np.count_nonzero(mine.view(U) != want.view(U))} words differ"
