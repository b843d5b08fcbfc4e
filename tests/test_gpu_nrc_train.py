"""-m gpu: the NRC TRAINING step (gfx_nrc_train: k_nrc_train<1> / <2>, k_nrc_grid_scatter, k_nrc_reduce_partials, k_nrc_optimizer)
through the C ABI, at the shapes and in the modes that tests/test_gpu_nrc_net.py does not reach.  The checks live in
tests/nrc_train_checks.py; tests/test_nrc_optimizer_cpu.py shows without a GPU that they reject a wrong optimizer.

  one step against oracle/nrc_net.py   the bounds of test_gpu_nrc_net.py::test_one_training_step_matches_oracle (loss 2e-3 relative, MLP
      part of Adam's first moment 1e-2 relative L2, the same hash-grid entries touched for > 99.9 %) at batches of 128 (one short
      chunk, 4 dW partials), 128*37 (ragged last chunk, 148 partials), 128*130 (chunks longer than one staging batch of
      k_nrc_grid_scatter) and 64*4*numCUs + 128 (128 past the first batch that launches k_nrc_train<2>, chunks of four staging batches and a
      ragged one: the test asserts the kernel's own threshold on the device's CU count).  The hash-grid gradient m[grid_off:] / 0.1 is held against the oracle's fp32-sum gradient
      within max(1e-2, 2 x the oracle's own fp16-sum-to-fp32-sum distance on the same batch): the bound comes from the reference alone,
      the factor 2 is the device's undefined summing order.
  GFX_NRC_GRID_GRAD = f32 / f16atomic  the same step against the oracle summing in fp32 / in fp16 over the whole batch
      (NrcNet(grid_chunk=batch)), and a second step on other records: an entry whose moment moves at step 2 although no record of step 2
      reaches it is a gradient buffer that was not cleared.
  the optimizer                        six steps on fresh records confined to a small box each, both encodings, every step restated from the
      device's OWN previous state (get_params(0..3) before and after): weights and EMA bit for bit, the moments by the rules of
      nrc_train_checks (step 1: some fp32 g within 4 ulp gives m_1 and v_1 bit for bit; later: the derived bound on v_t), untouched
      hash-grid entries keep m, v and w while their EMA moves, the pad rows of Wout carry the L2 term exactly, and the per-encoding eps
      shows on their first step.
  determinism                          two steps in two fresh contexts at 128*37 and at the <2> threshold: all four state arrays identical.

Measured on an MI355X (256 CUs: threshold batch 65 664); "ref" is the oracle's fp16-sum-to-fp32-sum distance, the bound is max(1e-2, 2 ref):

  mode       encoding  hidden  batch   loss (<= 2e-3)  MLP m (<= 1e-2)  touched (> 0.999)  grid gradient   ref       bound
  lds        hash      2          128  1.0e-7          7.0e-8           1.0                2.106e-4        2.110e-4  1e-2
  lds        hash      5          128  0               6.6e-8           1.0                2.166e-4        2.159e-4  1e-2
  lds        hash      2        4 736  3.1e-7          1.3e-7           1.0                1.964e-4        1.954e-4  1e-2
  lds        hash      5        4 736  0               2.9e-6           1.0                2.290e-4        2.094e-4  1e-2
  lds        triangle  5        4 736  6.1e-8          1.3e-6           -                  -               -         -
  lds        hash      2       16 640  4.1e-7          2.7e-7           1.0                1.800e-4        1.726e-4  1e-2
  lds        hash      5       16 640  5.5e-7          1.6e-6           1.0                2.384e-4        2.047e-4  1e-2
  lds  <2>   hash      2       65 664  6.2e-7          4.2e-7           1.0                1.616e-4        1.327e-4  1e-2
  lds  <2>   hash      5       65 664  6.6e-7          8.0e-6           1.0                7.476e-4        1.812e-4  1e-2
  f32        hash      2        4 736  2.0e-7          7.9e-7           1.0                2.40e-5         0         1e-2
  f32        hash      2        2 048  6.1e-7          3.0e-6           1.0                9.89e-5         0         1e-2
  f16atomic  hash      2        4 736  2.0e-7          7.9e-7           1.0                3.232e-4        2.597e-4  1e-2
  f16atomic  hash      2        2 048  4.1e-7          3.0e-6           1.0                2.839e-4        2.453e-4  1e-2
  step 2 of the f32 / f16atomic cases: 0 entries moved that no record reaches (32 % / 60 % of the entries are out of reach at 4 736 /
  2 048 records); touched sets agree for 1.0 / 0.999997 (f16atomic, 4 736) of the entries.
  The reference distance is 1.3e-4 .. 2.6e-4 at every shape, so the floor of 1e-2 -- the project's stated one-step gradient tolerance --
  is the bound everywhere; the device sits at 1.0 .. 1.4 x the reference distance (4 x with five hidden layers at 65 664 records).
  optimizer: weights and EMA BIT-EXACT for all 1 000 448 (hash grid) / 9 216 (triangle wave) parameters at each of the six steps -- the
  2-ulp allowance for std::pow against Python's ** was not needed; 83.6 .. 83.7 % of the grid entries untouched per step, 504 647
  touched at one step and untouched at a later one, 2 fixed-point touches (nrc_train_checks.fixed_point_touch: the oracle has the same 2).
"""
import numpy as np
import pytest

from gfxexp_amd import api
from oracle import nrc_net as N
from tests import nrc_train_checks as K
from tests.test_gpu_nrc_net import _inputs, _random_params, _targets

LR = 1e-2
THRESHOLD = "threshold"        # 64 * 4 * numCUs + 128 records: resolved on the device


def _batch_size(n):
    """The batch of a case; for THRESHOLD one step of 128 past the first batch that nrc_train gives the 64-record tile (numData / 64 >=
    4 numCUs), which also makes every chunk of k_nrc_grid_scatter four full staging batches and a ragged one.  The kernel's rule is
    asserted on this device's CU count so that another device cannot quietly run k_nrc_train<1> instead."""
    if n != THRESHOLD:
        return n
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 64 * 4 * cus + 128
    assert n % 128 == 0 and n // 64 >= 4 * cus, (n, cus)
    print(f"NRC-TRAIN-TILE numCUs {cus}: batch {n} -> {n // 64} blocks of 64 records (k_nrc_train<2>)")
    return n


class _Device:
    """A network in a context of its own; states as (w, ema, m, v)."""

    def __init__(self, pos_enc, hidden, params):
        self.ctx = api.Context(0)
        self.net = api.NeuralRadianceCache(self.ctx, pos_enc, hidden, LR)
        self.net.set_params(params)

    def train(self, x, t, want_loss=False):
        import torch
        dx, dt = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()
        loss = self.net.train(dx.data_ptr(), dt.data_ptr(), x.shape[0], want_loss=want_loss, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return loss

    def state(self):
        return tuple(self.net.get_params(which) for which in range(4))      # gfx_nrc_get_params synchronises the device

    def close(self):
        self.net.close()
        self.ctx.close()


def _one_step(label, pos_enc, hidden, n, seed, mirror_kw, steps=1):
    """One step (or two, on different records) on the device and on the oracle in the mode that mirrors it; the first step through
    check_step_against_oracle, the second through the touched sets."""
    rng = np.random.default_rng(seed)
    p = _random_params(rng, pos_enc, hidden)
    x = _inputs(rng, n)
    t = _targets(x)
    dev = _Device(pos_enc, hidden, p)
    try:
        loss = dev.train(x, t, want_loss=True)
        m_dev = dev.state()[2]
        ref = N.NrcNet(pos_enc, hidden, LR, params=p, **mirror_kw)
        ref_loss, g_mirror = ref.gradients(x, t)
        ref.optimizer_step(g_mirror)
        g32 = g_mirror
        if pos_enc == N.POS_HASHGRID and ref.grid_grad_f16:
            _, g32 = N.NrcNet(pos_enc, hidden, LR, params=p, grid_grad_f16=False).gradients(x, t)
        K.check_step_against_oracle(label, loss, m_dev, ref, ref_loss, g_mirror, g32)
        if steps == 2:
            grid_off = ref.grid_off
            x2 = _inputs(rng, n)
            t2 = _targets(x2)
            m_ref1 = ref.m.copy()
            dev.train(x2, t2)
            ref.train(x2, t2)
            m_dev2 = dev.state()[2]
            touched_dev = (K.bits(m_dev2) != K.bits(m_dev))[grid_off:]
            touched_ref = (K.bits(ref.m) != K.bits(m_ref1))[grid_off:]
            reached = K.reached_entries(x2, ref.total - grid_off)
            assert touched_dev.any() and not reached.all()
            stale = np.flatnonzero(touched_dev & ~reached)
            agree = float(np.mean(touched_dev == touched_ref))
            print("NRC-TRAIN-FIGURES", {"case": label + " step 2", "touched_agree": float(f"{agree:.6g}"), "stale": int(stale.size),
                                        "unreached_fraction": float(f"{1 - reached.mean():.3g}")})
            assert stale.size == 0, f"{label}: {stale.size} entries moved at step 2 that no record of step 2 reaches (first {stale[0]}): a gradient left over from step 1"
            assert agree > 0.999, (label, agree)
    finally:
        dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pos_enc,hidden,n", [
    (N.POS_HASHGRID, 2, 128), (N.POS_HASHGRID, 5, 128),
    (N.POS_HASHGRID, 2, 128 * 37), (N.POS_HASHGRID, 5, 128 * 37), (N.POS_TRIANGLEWAVE, 5, 128 * 37),
    (N.POS_HASHGRID, 2, 128 * 130), (N.POS_HASHGRID, 5, 128 * 130),
    (N.POS_HASHGRID, 2, THRESHOLD), (N.POS_HASHGRID, 5, THRESHOLD)])
def test_one_training_step_matches_oracle_at_ragged_and_large_batches(built_lib, pos_enc, hidden, n):
    n = _batch_size(n)
    _one_step(f"lds enc {pos_enc} hidden {hidden} batch {n}", pos_enc, hidden, n, seed=12 + hidden, mirror_kw={})


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f32", "f16atomic"])
@pytest.mark.parametrize("n", [128 * 37, 128 * 16])
def test_other_grid_gradient_modes_match_oracle_and_clear_their_buffer(built_lib, monkeypatch, mode, n):
    """GFX_NRC_GRID_GRAD is read when a network is created.  f32: fp32 atomics, the buffer cleared inside the optimizer; f16atomic:
    packed fp16 atomics over the whole batch, the buffer cleared by a memset behind the optimizer."""
    monkeypatch.setenv("GFX_NRC_GRID_GRAD", mode)
    mirror = {"grid_grad_f16": False} if mode == "f32" else {"grid_chunk": n}
    _one_step(f"{mode} hidden 2 batch {n}", N.POS_HASHGRID, 2, n, seed=23, mirror_kw=mirror, steps=2)


def _device_trajectory(pos_enc, hidden, n):
    p = _random_params(np.random.default_rng(7), pos_enc, hidden)
    dev = _Device(pos_enc, hidden, p)
    try:
        states = [dev.state()]
        assert np.array_equal(K.bits(states[0][0]), K.bits(p)) and np.array_equal(K.bits(states[0][1]), K.bits(p))
        for x, t in K.boxed_batches(_inputs, _targets, n):
            dev.train(x, t)
            states.append(dev.state())
    finally:
        dev.close()
    return states


@pytest.mark.gpu
@pytest.mark.parametrize("pos_enc", [N.POS_HASHGRID, N.POS_TRIANGLEWAVE], ids=["hashgrid", "trianglewave"])
def test_optimizer_bit_for_bit_from_its_own_state(built_lib, pos_enc):
    """Six steps of 128*8 fresh records, every step from the state the device itself had before it (nrc_train_checks.
    check_optimizer_trajectory): the step counter behind lrT / debiasOld / debiasNew, beta2, the per-encoding eps, the 1e-6 L2 term
    and the untouched-entry rule are all visible here and nowhere else in the suite.  Weights and EMA are compared in every bit: no
    ulp allowance."""
    hidden, n = 2, 128 * 8
    states = _device_trajectory(pos_enc, hidden, n)
    stats = K.check_optimizer_trajectory(states, pos_enc, hidden, LR)
    print("NRC-TRAIN-FIGURES", {"case": f"optimizer enc {pos_enc}", "weights_and_ema": "bit-exact over 6 steps", **stats})
    K.check_pad_row_first_step(states[0][0], states[1][0], states[1][3], hidden, LR, pos_enc)


@pytest.mark.gpu
def test_eps_shortens_the_first_pad_row_step_for_triangle_wave_only(built_lib):
    """The same Wout (one initialisation stream) under both encodings, one step each: sqrt(v_1) of a pad row is ~1e-8, so the
    triangle-wave eps (1e-8) about halves the step and the hash-grid eps (1e-15) leaves it at lr -- entry by entry."""
    hidden, n = 2, 128 * 8
    rel = {}
    for pos_enc in (N.POS_HASHGRID, N.POS_TRIANGLEWAVE):
        p = _random_params(np.random.default_rng(7), pos_enc, hidden)
        x, t = K.boxed_batches(_inputs, _targets, n)[0]
        dev = _Device(pos_enc, hidden, p)
        try:
            dev.train(x, t)
            w1, _, _, v1 = dev.state()
        finally:
            dev.close()
        rel[pos_enc] = K.check_pad_row_first_step(p, w1, v1, hidden, LR, pos_enc)
    assert rel[N.POS_HASHGRID].shape == rel[N.POS_TRIANGLEWAVE].shape          # the same weights selected
    assert (rel[N.POS_TRIANGLEWAVE] < rel[N.POS_HASHGRID]).all()
    ratio = rel[N.POS_TRIANGLEWAVE].mean() / rel[N.POS_HASHGRID].mean()
    assert 0.35 < ratio < 0.65, ratio


@pytest.mark.gpu
@pytest.mark.parametrize("n", [128 * 37, THRESHOLD])
def test_training_is_reproducible_bit_for_bit_at_ragged_and_large_batches(built_lib, n):
    """test_gpu_nrc_net.py::test_training_is_reproducible_bit_for_bit at a batch with a ragged last chunk and a partial count that is no
    multiple of k_nrc_reduce_partials' 16 slices, and at the smallest batch of the 64-record tile: two steps in two fresh contexts
    (default lds mode), parameters, EMA, m and v the same bits.  Half of the records crowd one coarse cell."""
    n = _batch_size(n)
    rng = np.random.default_rng(17)
    x = _inputs(rng, n)
    x[: n // 2, :3] = 0.4 + 0.002 * rng.random((n // 2, 3), dtype=np.float32)
    t = _targets(x)
    p = _random_params(rng, N.POS_HASHGRID, 2)
    runs = []
    for _ in range(2):
        dev = _Device(N.POS_HASHGRID, 2, p)
        try:
            dev.train(x, t)
            dev.train(x, t)
            runs.append([K.bits(a).copy() for a in dev.state()])
        finally:
            dev.close()
    assert not np.array_equal(runs[0][0], K.bits(p)), "the training moved nothing"
    for which, name in enumerate(K.STATE_NAMES):
        bad = np.count_nonzero(runs[0][which] != runs[1][which])
        assert bad == 0, f"{bad} of {runs[0][which].size} {name} differ between the two runs"
