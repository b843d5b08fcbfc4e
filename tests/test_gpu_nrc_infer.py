"""-m gpu: NRC INFERENCE (gfx_nrc_infer / gfx_nrc_infer_indirect: k_nrc_infer, k_nrc_infer_staged, k_nrc_infer_piped, k_nrc_pack) pinned without a
statistical tolerance.  The checks live in tests/nrc_infer_checks.py (the derivations of the deltas are in its docstring);
tests/test_nrc_infer_checks_cpu.py shows without a GPU that they hold oracle/nrc_net.py at half of each delta and reject nine wrong encoders and
two wrong layer layouts.  tests/test_gpu_nrc_net.py keeps the random-weight comparisons within their stated tolerances.

  features    22 selector parameter sets make the network return its own encoding, bf16(feature f), three features a set; on edge_inputs
      (cell boundaries of every level and an ulp either side, positions outside [0, 1) up to 3 000, one-blob inputs on and beside the bin
      edges and in [-3, 3] with both one-blob forms inside one wave, signed / large / zero identity inputs) every output must lie in
      [bf16(F - delta), bf16(F + delta)] of the float64 reference F.  1, 2 and 5 hidden layers, both encodings, batches of 128 and 128 * 25.
  layers      eight variants of an exactly summable network (sparse dyadic weights, every matrix position non-zero in one of them): the
      outputs equal the exact reference in every bit.  1, 2, 3 and 5 hidden layers.
  isolation   every third query NaN / +-Inf / +-1e30 in all 14 inputs: the other queries' outputs are the bits of a run with 0.5 there.
  count       gfx_nrc_infer_indirect at live counts 0, 1, 63, 64, 65, n - 1, n, n + 128: the first `live` outputs are the direct call's bits,
      the rest keeps its sentinel.
  Hash grid: "nrc_staged_infer" 1 (k_nrc_infer), 2 (k_nrc_infer_staged) and 3 (k_nrc_infer_piped; with more than two hidden layers mode 3 runs
  k_nrc_infer_staged -- the ids say so) and the three agree bit for bit; the triangle wave has k_nrc_infer only.

Measured on an MI355X: all 36 cases pass and no kernel needed a change.  Per feature block, over the 22 sets: the share of outputs equal
to bf16(F), the share that took another acceptable value, and the largest distance from F to the reals that round to the device's value r, in
units of delta (0 where r = bf16(F), accepted means <= 1; |r - F| itself is the bf16 step, 2^11 delta and more, and says nothing).  The
figures are the same for 1, 2 and 5 hidden layers and for the three hash-grid modes -- they have to be, the kernels agree bit for bit:

  block                     batch   = bf16(F)   other accepted   largest distance / delta
  hash grid (32 features)     128   1.0         0                0
  hash grid                 3 200   0.99998     1.95e-5 (2)      0.014
  triangle wave (36)          128   1.0         0                0
  triangle wave             3 200   1.0         0                0
  one-blob (20)               128   0.9844      0.0156           0.070
  one-blob                  3 200   0.9875      0.0125           0.088
  identity (6), pad (6 / 2)  both   1.0         0                0
  The one-blob outputs that are not bf16(F) have F within 0.09 delta of a bf16 rounding tie (small features far out on the kernel's tail
  for the most part, and some whose F is exactly 0 where the CDF sums leave a residue of one fp32 step); the numpy restatement of the kernel's
  two forms (nrc_infer_checks.fp32_oneblob, five-integral inside [0, 1]) gives the same three figures on the same inputs.
  layers: 0 of 3 x 128 and 3 x 3 200 outputs differ from the exact reference in all 8 variants x 4 depths x 4 kernels-and-encodings.
  isolation and count: no clean query changed; no output past the live count was written, live count 0 and the clamped n + 128 included.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from gfxexp_amd import api
from oracle import nrc_net as N
from tests import nrc_infer_checks as K
from tests.test_gpu_nrc_net import _inputs, _random_params

BATCHES = (128, 128 * 25)          # one tile pair; two staged passes of 25 tiles (ragged: 12 waves x 4 slots hold 48)
SENTINEL = -7.0
ENC_NAME = {N.POS_HASHGRID: "hashgrid", N.POS_TRIANGLEWAVE: "trianglewave"}


def _cases(hiddens):
    """(pos_enc, hidden, mode) with ids that name the kernel a mode really runs."""
    out = []
    for hidden in hiddens:
        for mode, name in ((1, "mode1-in-place"), (2, "mode2-staged"), (3, "mode3-piped" if hidden <= 2 else "mode3-runs-staged")):
            out.append(pytest.param(N.POS_HASHGRID, hidden, mode, id=f"hashgrid-hidden{hidden}-{name}"))
        out.append(pytest.param(N.POS_TRIANGLEWAVE, hidden, 1, id=f"trianglewave-hidden{hidden}-in-place"))
    return out


class _Device:
    """A network in a context of its own with "nrc_staged_infer" = mode."""

    def __init__(self, pos_enc, hidden, mode):
        self.ctx = api.Context(0)
        self.ctx.tunable_set("nrc_staged_infer", mode)
        self.net = api.NeuralRadianceCache(self.ctx, pos_enc, hidden)

    def infer(self, x, live=None):
        """Outputs [n, 3] of a sentinel-filled buffer; live: through gfx_nrc_infer_indirect with that device-side count."""
        import torch
        n = x.shape[0]
        dx = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
        dy = torch.full((n, 3), SENTINEL, dtype=torch.float32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        if live is None:
            self.net.infer(dx.data_ptr(), n, dy.data_ptr(), stream)
        else:
            cnt = torch.tensor([live], dtype=torch.int32, device="cuda")
            self.ctx._check(api.lib().gfx_nrc_infer_indirect(self.ctx.h, C.c_void_p(stream), C.c_uint64(self.net.h), C.c_void_p(dx.data_ptr()),
                                                             C.c_void_p(cnt.data_ptr()), C.c_uint32(n), C.c_void_p(dy.data_ptr())))
        torch.cuda.synchronize()
        return dy.cpu().numpy()

    def close(self):
        self.net.close()
        self.ctx.close()


@functools.lru_cache(maxsize=None)
def _edge(n):
    x, grid = K.edge_inputs(n), K.feature_grid()
    return x, grid, {enc: K.ref_features(enc, x, grid) for enc in ENC_NAME}


@functools.lru_cache(maxsize=None)
def _selector_outputs(pos_enc, hidden, mode):
    """{n: [N_SETS, n, 3]}: every selector set on edge_inputs(n); computed once per (encoding, depth, mode) and left unchanged."""
    dev = _Device(pos_enc, hidden, mode)
    try:
        out = {n: np.zeros((K.N_SETS, n, 3), np.float32) for n in BATCHES}
        for s in range(K.N_SETS):
            dev.net.set_params(K.selector_params(pos_enc, hidden, s, _edge(BATCHES[0])[1]))
            for n in BATCHES:
                out[n][s] = dev.infer(_edge(n)[0])
    finally:
        dev.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("pos_enc,hidden,mode", _cases((1, 2, 5)))
def test_every_feature_lies_in_its_rounding_interval(built_lib, pos_enc, hidden, mode):
    outs = _selector_outputs(pos_enc, hidden, mode)
    for n in BATCHES:
        _, _, refs = _edge(n)
        F, D = refs[pos_enc]
        got = np.zeros((n, 64))
        for s in range(K.N_SETS):
            got[:, K.selector_features(s)] = outs[n][s]                  # (features 0 and 1 are read twice: set 21 wraps; compared below per set)
        fig = {b: K.figures(got[:, sl], F[:, sl], D[:, sl]) for b, sl in K.blocks(pos_enc).items()}
        print("NRC-INFER-FIGURES", {"case": f"{ENC_NAME[pos_enc]} hidden {hidden} mode {mode} batch {n}",
                                    **{b: {k: float(f"{v:.4g}") for k, v in f.items()} for b, f in fig.items()}})
        for s in range(K.N_SETS):
            f = K.selector_features(s)
            r = outs[n][s]
            assert np.isfinite(r).all() and (r != SENTINEL).any(), (s, "non-finite or unwritten outputs")
            assert K.is_bf16(r).all(), (s, "an output is not a bf16 number: more than one term reached a sum")
            bad = ~K.accept(r, F[:, f], D[:, f])
            if bad.any():
                q, o = np.argwhere(bad)[0]
                raise AssertionError(f"batch {n} set {s}: {int(bad.sum())} outputs outside their interval; first: query {q} feature {f[o]} "
                                     f"got {r[q, o]!r} reference {F[q, f[o]]!r} delta {D[q, f[o]]!r} inputs {_edge(n)[0][q]!r}")
    if mode != 1:                                                     # the contract of test_gpu_nrc_net.py: the kernels agree bit for bit
        base = _selector_outputs(pos_enc, hidden, 1)
        for n in BATCHES:
            diff = outs[n].view(np.uint32) != base[n].view(np.uint32)
            assert not diff.any(), f"batch {n}: {int(diff.sum())} outputs differ from the in-place kernel's (first (set, query, output) {np.argwhere(diff)[0]})"


@pytest.mark.gpu
@pytest.mark.parametrize("pos_enc,hidden,mode", _cases((1, 2, 3, 5)))
def test_layers_bit_for_bit_on_exactly_summable_networks(built_lib, pos_enc, hidden, mode):
    K.exact_network_coverage(pos_enc, hidden)
    dev = _Device(pos_enc, hidden, mode)
    try:
        for variant in range(K.N_VARIANTS):
            for n in BATCHES:
                net = K.exact_network(pos_enc, hidden, variant, n)        # (not kept: a hash-grid parameter blob is 4 MB)
                dev.net.set_params(net["params"])
                y = dev.infer(net["x"])
                diff = K.canon_bits(y) != K.canon_bits(net["ref"])
                if diff.any():
                    q, o = np.argwhere(diff)[0]
                    raise AssertionError(f"variant {variant} batch {n}: {int(diff.sum())} of {diff.size} outputs differ from the exact reference; "
                                         f"first: query {q} output {o} got {y[q, o]!r} exact {net['ref'][q, o]!r}")
    finally:
        dev.close()


def _poisoned(x):
    """(poisoned copy, clean copy, mask of the untouched queries): every third query holds NaN, +-Inf or +-1e30 in all of its inputs
    (the kind changes from input to input and from query to query) / 0.5 in the clean copy."""
    bad = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32)
    rows = np.arange(0, x.shape[0], 3)
    dirty, clean = x.copy(), x.copy()
    dirty[rows] = bad[(rows[:, None] // 3 + np.arange(14)[None, :]) % bad.size]
    clean[rows] = 0.5
    keep = np.ones(x.shape[0], bool)
    keep[rows] = False
    return dirty, clean, keep


@pytest.mark.gpu
@pytest.mark.parametrize("pos_enc,hidden,mode", _cases((2,)))
def test_non_finite_queries_do_not_reach_their_neighbours(built_lib, pos_enc, hidden, mode):
    """The LDS input staging, the v_permlane32_swap hand-over and the pass scratch move values between lanes: none may move between queries."""
    rng = np.random.default_rng(41)
    dev = _Device(pos_enc, hidden, mode)
    try:
        dev.net.set_params(_random_params(rng, pos_enc, hidden))
        for n in BATCHES:
            dirty, clean, keep = _poisoned(_edge(n)[0])
            y_dirty, y_clean = dev.infer(dirty), dev.infer(clean)
            assert np.isfinite(y_clean).all() and (y_clean != SENTINEL).any()
            diff = (y_dirty.view(np.uint32) != y_clean.view(np.uint32))[keep]
            assert not diff.any(), f"batch {n}: {int(diff.any(axis=1).sum())} clean queries changed beside poisoned ones (first clean index {np.argwhere(diff)[0][0]})"
    finally:
        dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pos_enc,hidden,mode", _cases((2,)))
def test_device_side_count_at_its_edges(built_lib, pos_enc, hidden, mode):
    rng = np.random.default_rng(43)
    dev = _Device(pos_enc, hidden, mode)
    try:
        dev.net.set_params(_random_params(rng, pos_enc, hidden))
        for n in BATCHES:
            x = _inputs(rng, n)
            direct = dev.infer(x)
            assert np.isfinite(direct).all() and (direct != SENTINEL).all()
            for count in (0, 1, 63, 64, 65, n - 1, n, n + 128):
                live = min(count, n)                                  # a count past the batch is clamped to it
                z = dev.infer(x, live=count)
                assert np.array_equal(z[:live].view(np.uint32), direct[:live].view(np.uint32)), f"batch {n} count {count}: the live outputs differ from the direct call"
                assert (z[live:] == SENTINEL).all(), f"batch {n} count {count}: queries past the device-side count were written"
    finally:
        dev.close()
