"""-m gpu: the device copy of the shading layer (gfxexp_amd/csrc/shading.hip.h: Bsdf, the GGX helpers, concentric_disk,
cosine_hemisphere, make_coordinate_system, Frame, apply_bump_mapping, shadow_ray, direct_lighting, target_weight), run by the
inspection entry gfx_bsdf_eval, against the CPU oracle, bit for bit, on the lists of tests/bsdf_cases.py.
tests/test_bsdf_cpu.py holds the oracle against a float64 statement of the definitions, so equality here puts the kernels' own
functions under those bounds too.

As in test_gpu_math_contract.py a float word passes when both sides are NaN (sign and payload of a NaN are not part of the contract),
and the number of NaN words must be the one the CPU test recorded for the list (bsdf_cases.NAN_WORDS)."""
import functools

import numpy as np
import pytest

from gfxexp_amd import api
from tests import bsdf_cases as BC

pytestmark = pytest.mark.gpu
F, U = np.float32, np.uint32
GUARD = 0x5A5A5A5A
CASES = [(fn, name) for fn, lists in BC.LISTS.items() for name in lists]


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
    return getattr(api, "BSDF_" + fn)


def gpu_eval(fn, c, stream=None, tail=0):
    """gfx_bsdf_eval once on list c: uint32 [words, n] (and the `tail` guard words behind the output)."""
    import torch
    n = max(len(x) for x in c.values() if x is not None)
    words = api.BSDF_EVAL_WORDS[fn_id(fn)]
    s = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(s):
        d = {k: (torch.from_numpy(np.array(v)).cuda() if v is not None else None) for k, v in c.items()}
        ptr = {k: (v.data_ptr() if v is not None else 0) for k, v in d.items()}
        d_out = torch.full((words * n + tail,), GUARD, dtype=torch.int32, device="cuda")
        context().bsdf_eval(fn_id(fn), n, d_out.data_ptr(), d_mat=ptr["mat"], d_a=ptr["A"], d_b=ptr["B"], d_c=ptr["C"], stream=s.cuda_stream)
        s.synchronize()
        out = d_out.cpu().numpy().view(U)
    return (out[:words * n].reshape(words, n), out[words * n:]) if tail else out.reshape(words, n)


def describe(c, i):
    return ", ".join(f"{k} = {v[i].tolist()} (bits {[hex(b) for b in v[i].view(U)]})" for k, v in c.items() if v is not None)


def assert_parity(what, fn, got, want, c):
    assert got.shape[0] == api.BSDF_EVAL_WORDS[fn_id(fn)] and want.shape[0] == BC.WORDS[fn]
    for k in range(got.shape[0]):
        if k >= len(want):
            assert not np.any(got[k]), f"{what}: unused result word {k} is not 0"
            continue
        bad = (got[k] != want[k]) & ~(np.isnan(got[k].view(F)) & np.isnan(want[k].view(F)))
        if np.any(bad):
            i = int(np.flatnonzero(bad)[0])
            raise AssertionError(f"{what}: word {k} differs on {np.count_nonzero(bad)} of {len(bad)} elements, first at {i}: {describe(c, i)}; "
                                 f"device {int(got[k][i]):#010x} ({got[k][i:i + 1].view(F)[0]!r}), oracle {int(want[k][i]):#010x} ({want[k][i:i + 1].view(F)[0]!r})")


def part(c, sl):
    return {k: (None if v is None else v[sl]) for k, v in c.items()}


@pytest.mark.parametrize("fn,name", CASES, ids=[f"{fn}-{name}" for fn, name in CASES])
def test_device_equals_oracle(built_lib, fn, name):
    c = BC.LISTS[fn][name]()
    got = gpu_eval(fn, c)
    assert_parity(f"{fn} on {name}", fn, got, BC.oracle_words(fn, c), c)
    assert BC.nan_words(got) == BC.NAN_WORDS[(fn, name)]


def test_unit_views_above_the_surface_sample_without_nan(built_lib):
    """The largest random numbers (u0 = 1 - 2^-23, 1 - 2^-24) with unit view directions of z > 0: no NaN in throughput, direction or
    density (the radicand of the visible-normal sampler is clamped at 0)."""
    for name in ("u-edge", "u0-top"):
        got = gpu_eval("SAMPLE", BC.LISTS["SAMPLE"][name]())
        assert BC.nan_words(got) == 0, f"SAMPLE on {name}: {BC.nan_words(got)} NaN words"


@pytest.mark.parametrize("n", [1, 255, 257, 1000 + 37])
def test_lengths_off_the_block_size(built_lib, n):
    """A list that is no multiple of the 256-thread block, and a single element: every element is written, nothing past the end.
    BUMP_FRAME has the widest output and reads every kind of list but the material's; DIRECT_LIGHTING reads that too."""
    for fn, name in (("BUMP_FRAME", "interior"), ("DIRECT_LIGHTING", "edge")):
        c = part(BC.LISTS[fn][name](), slice(5000, 5000 + n))
        got, tail = gpu_eval(fn, c, tail=64)
        assert np.all(tail == GUARD)
        assert_parity(f"{fn} n = {n}", fn, got, BC.oracle_words(fn, c), c)


def test_a_second_stream_reproduces_the_first(built_lib):
    import torch
    c = part(BC.sample_interior(), slice(0, 100003))
    first = gpu_eval("SAMPLE", c)
    second = gpu_eval("SAMPLE", c, stream=torch.cuda.Stream())
    assert np.array_equal(first, second)
    assert_parity("SAMPLE on a second stream", "SAMPLE", second, BC.oracle_words("SAMPLE", c), c)


def test_refusals_launch_nothing(built_lib):
    import torch
    ctx = context()
    n = 64
    d_in = torch.zeros(16 * n + 4, dtype=torch.float32, device="cuda")
    d_out = torch.full((16 * n + 4,), GUARD, dtype=torch.int32, device="cuda")
    a, o = d_in.data_ptr(), d_out.data_ptr()
    full = dict(d_mat=a, d_a=a, d_b=a, d_c=a)
    for fn in (9, -1):
        with pytest.raises(api.GfxError, match="unknown fn"):
            ctx.bsdf_eval(fn, n, o, **full)
    with pytest.raises(api.GfxError, match="output buffer must not be null"):
        ctx.bsdf_eval(api.BSDF_EVALUATE, n, 0, **full)
    needs = {api.BSDF_SETUP: ("d_mat",), api.BSDF_EVALUATE: ("d_mat", "d_a", "d_b"), api.BSDF_PDF: ("d_mat", "d_a", "d_b"),
             api.BSDF_SAMPLE: ("d_mat", "d_a", "d_b"), api.BSDF_DHR: ("d_mat", "d_a"), api.BSDF_COSINE_HEMISPHERE: ("d_a",),
             api.BSDF_COORDINATE_SYSTEM: ("d_a",), api.BSDF_BUMP_FRAME: ("d_a", "d_b", "d_c"),
             api.BSDF_DIRECT_LIGHTING: ("d_mat", "d_a", "d_b", "d_c")}
    which = {"d_mat": "material list", "d_a": "first argument list", "d_b": "second argument list", "d_c": "extra argument list"}
    for fn, lists in needs.items():
        for missing in lists:                               # a list the function reads is null
            with pytest.raises(api.GfxError, match=which[missing] + ", which is null"):
                ctx.bsdf_eval(fn, n, o, **{k: (0 if k == missing else a) for k in lists})
        for off in lists:                                   # ... or misaligned
            with pytest.raises(api.GfxError, match="16-byte aligned"):
                ctx.bsdf_eval(fn, n, o, **{k: (a + 4 if k == off else a) for k in lists})
        with pytest.raises(api.GfxError, match="16-byte aligned"):
            ctx.bsdf_eval(fn, n, o + 8, **{k: a for k in lists})
    ctx.bsdf_eval(api.BSDF_EVALUATE, 0, 0)                                # n == 0: nothing to do, nothing touched
    torch.cuda.synchronize()
    assert torch.all(d_out == GUARD)
    ctx.bsdf_eval(api.BSDF_COSINE_HEMISPHERE, n, o, d_a=a)                # and the accepted call does write: (0, 0) -> (-1, ~0, 0)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(U)
    want = BC.oracle_words("COSINE_HEMISPHERE", dict(A=np.zeros((n, 4), F)))
    assert np.array_equal(out[:5 * n].reshape(5, n), want) and np.all(out[5 * n:8 * n] == 0) and np.all(out[8 * n:] == GUARD)
    for fn in range(9):                                                   # the width the library reports is the one the wrapper documents
        assert built_lib.gfx_bsdf_eval_words(fn) == api.BSDF_EVAL_WORDS[fn]
    assert built_lib.gfx_bsdf_eval_words(9) == 0 and built_lib.gfx_bsdf_eval_words(-1) == 0


def test_sample_evaluate_pdf_chain_on_the_device(built_lib):
    """SAMPLE -> (directions transposed on the device) -> EVALUATE and PDF, the device's own intermediate values never leaving it:
    what comes back is the same chain on the oracle."""
    import torch
    parts = [part(BC.sample_interior(), slice(0, 1 << 16)), part(BC.sample_u_edge(), slice(0, None, 37)), BC.sample_direction_edge()]
    c = {k: np.concatenate([p[k] for p in parts]) for k in ("mat", "A", "B")}
    n = len(c["A"])
    ctx, s = context(), torch.cuda.current_stream().cuda_stream
    d_mat, d_a, d_u = (torch.from_numpy(c[k]).cuda() for k in ("mat", "A", "B"))
    d_smp = torch.zeros(8 * n, dtype=torch.int32, device="cuda")
    ctx.bsdf_eval(api.BSDF_SAMPLE, n, d_smp.data_ptr(), d_mat=d_mat.data_ptr(), d_a=d_a.data_ptr(), d_b=d_u.data_ptr(), stream=s)
    d_dir = d_smp.view(8, n)[[3, 4, 5, 7]].t().contiguous()               # (x, y, z, 0) per element, as bits
    d_f = torch.zeros(4 * n, dtype=torch.int32, device="cuda")
    d_p = torch.zeros(4 * n, dtype=torch.int32, device="cuda")
    ctx.bsdf_eval(api.BSDF_EVALUATE, n, d_f.data_ptr(), d_mat=d_mat.data_ptr(), d_a=d_a.data_ptr(), d_b=d_dir.data_ptr(), stream=s)
    ctx.bsdf_eval(api.BSDF_PDF, n, d_p.data_ptr(), d_mat=d_mat.data_ptr(), d_a=d_a.data_ptr(), d_b=d_dir.data_ptr(), stream=s)
    torch.cuda.synchronize()
    smp = BC.oracle_out("SAMPLE", c)
    chained = dict(mat=c["mat"], A=c["A"], B=BC.a4(smp[:, 3:6]))
    assert_parity("SAMPLE -> EVALUATE", "EVALUATE", d_f.cpu().numpy().view(U).reshape(4, n), BC.oracle_words("EVALUATE", chained), chained)
    assert_parity("SAMPLE -> PDF", "PDF", d_p.cpu().numpy().view(U).reshape(4, n), BC.oracle_words("PDF", chained), chained)
