"""No GPU: the optimizer checks of tests/nrc_train_checks.py (what tests/test_gpu_nrc_train.py holds k_nrc_optimizer with) run against
oracle/nrc_net.py itself, NrcNet playing the device -- the bit-for-bit restatement of weights and EMA, the 4-ulp search for the
step-1 gradient, the second-moment bound, the untouched-entry counts of the boxed records and the pad-row L2 identity all hold -- and
against three deliberately wrong optimizers, each of which they reject by the rule it breaks:
    beta2 = 0.999            -> the moments (step 1: no g gives both m_1 and v_1)
    t off by one             -> the weights (lrT)
    eps inside the sqrt      -> the weights
so the GPU tests can fail.  The oracle's gradients are computed once per encoding and replayed into the wrong copies (the checks hold
an optimizer from its own state, whatever gradients it was fed)."""
import numpy as np
import pytest

from oracle import nrc_net as N
from tests import nrc_train_checks as K
from tests.test_gpu_nrc_net import _inputs, _random_params, _targets

HIDDEN, BATCH, LR = 2, 128 * 8, 1e-2


def _state(net):
    return tuple(np.array(a, np.float32) for a in (net.params, net.ema, net.m, net.v))


@pytest.fixture(scope="module", params=[N.POS_HASHGRID, N.POS_TRIANGLEWAVE], ids=["hashgrid", "trianglewave"])
def trajectory(request):
    """(pos_enc, initial parameters, the six loss-scaled gradients, the seven states) of the oracle on the boxed records."""
    pos_enc = request.param
    p = _random_params(np.random.default_rng(7), pos_enc, HIDDEN)
    net = N.NrcNet(pos_enc, HIDDEN, LR, params=p)
    grads, states = [], [_state(net)]
    for x, t in K.boxed_batches(_inputs, _targets, BATCH):
        _, g = net.gradients(x, t)
        net.optimizer_step(g)
        grads.append(g)
        states.append(_state(net))
    return pos_enc, p, grads, states


def test_the_oracle_passes_its_own_checks(trajectory):
    pos_enc, _, grads, states = trajectory
    stats = K.check_optimizer_trajectory(states, pos_enc, HIDDEN, LR)
    if pos_enc == N.POS_HASHGRID:
        # the boxes leave most of the grid alone at every step and drop entries from one step to the next (asserted inside, counted here)
        assert min(stats["untouched_fraction"]) >= 0.2 and stats["touched_then_untouched"] >= 1000, stats
        assert max(stats["untouched_fraction"]) < 1.0
    # the pad rows of Wout receive an exactly zero data gradient at every step
    pad = K.pad_row_slice(HIDDEN)
    assert all(not g[pad].any() for g in grads)


def test_the_step1_search_returns_the_gradient(trajectory):
    pos_enc, p, grads, states = trajectory
    grid_off = N.layout(pos_enc, HIDDEN)[1]
    g, found = K.find_step1_gradient(states[1][2], states[1][3])
    assert found.all()
    want = (grads[0] / np.float32(128.0)).astype(np.float32)
    want[:grid_off] = want[:grid_off] + K.L2_REG * p[:grid_off]
    # several neighbours of g can round to the same m_1 and v_1: the search finds one within the window, not necessarily g itself
    assert (np.abs(K.bits(g).astype(np.int64) - K.bits(want).astype(np.int64))[want != 0] <= 8).all()


class _WrongNet(N.NrcNet):
    """NrcNet.optimizer_step with one deliberate error."""

    def __init__(self, wrong, *args, **kw):
        super().__init__(*args, **kw)
        self.wrong = wrong

    def optimizer_step(self, g, loss_scale=128.0):
        self.step += 1
        t = self.step + (1 if self.wrong == "t_off_by_one" else 0)
        beta2 = np.float32(0.999) if self.wrong == "beta2_0.999" else self.beta2
        grad = (g / np.float32(loss_scale)).astype(np.float32)
        is_grid = np.zeros(self.total, bool)
        is_grid[self.grid_off:] = True
        active = ~(is_grid & (grad == 0))
        grad = np.where(is_grid, grad, grad + self.l2_reg * self.params).astype(np.float32)
        m = np.where(active, self.beta1 * self.m + (np.float32(1) - self.beta1) * grad, self.m).astype(np.float32)
        v = np.where(active, beta2 * self.v + (np.float32(1) - beta2) * grad * grad, self.v).astype(np.float32)
        lr_t = np.float32(float(self.lr) * np.sqrt(1.0 - float(beta2) ** t) / (1.0 - float(self.beta1) ** t))
        if self.wrong == "eps_inside_sqrt":
            upd = (lr_t * m / np.sqrt(v + self.eps)).astype(np.float32)
        else:
            upd = (lr_t * m / (np.sqrt(v) + self.eps)).astype(np.float32)
        self.params = np.where(active, self.params - upd, self.params).astype(np.float32)
        self.m, self.v = m, v
        d = np.float32(self.ema_decay)
        debias_old = np.float32(1.0 - float(d) ** (t - 1))
        debias_new = np.float32(1.0 / (1.0 - float(d) ** t))
        self.ema = (((np.float32(1) - d) * self.params + d * debias_old * self.ema) * debias_new).astype(np.float32)


def _replay(net, grads):
    states = [_state(net)]
    for g in grads:
        net.optimizer_step(g)
        states.append(_state(net))
    return states


def test_the_unbroken_copy_is_the_oracle(trajectory):
    pos_enc, p, grads, states = trajectory
    got = _replay(_WrongNet(None, pos_enc, HIDDEN, LR, params=p), grads[:2])
    for a, b in zip(got, states):
        assert all(np.array_equal(K.bits(x), K.bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("wrong,rule", [("beta2_0.999", r"step 1 moments"), ("t_off_by_one", r"step 1 weights"),
                                        ("eps_inside_sqrt", r"step 1 weights")])
def test_a_wrong_optimizer_is_rejected(trajectory, wrong, rule):
    pos_enc, p, grads, _ = trajectory
    states = _replay(_WrongNet(wrong, pos_enc, HIDDEN, LR, params=p), grads)
    with pytest.raises(AssertionError, match=rule):
        K.check_optimizer_trajectory(states, pos_enc, HIDDEN, LR)


def test_wrong_optimizers_are_caught_at_later_steps_too(trajectory):
    """What step 1 cannot show: beta2 enters v_t through beta2 v_{t-1}, the step counter through lrT and both EMA debias factors.  The
    copy is right at step 1 and wrong from step 2 on."""
    pos_enc, p, grads, _ = trajectory
    for wrong, rule in (("beta2_0.999", r"step 2 second moment"), ("t_off_by_one", r"step 2 weights"), ("eps_inside_sqrt", r"step 2 weights")):
        net = _WrongNet(None, pos_enc, HIDDEN, LR, params=p)
        states = _replay(net, grads[:1])
        net.wrong = wrong
        states += _replay(net, grads[1:])[1:]
        with pytest.raises(AssertionError, match=rule):
            K.check_optimizer_trajectory(states, pos_enc, HIDDEN, LR)
    # and a wrong EMA step counter alone (weights right): the EMA rule names it
    net = N.NrcNet(pos_enc, HIDDEN, LR, params=p)
    states = _replay(net, grads)
    lr_t, old, new = K.host_scalars(LR, 4)
    w, e = states[3][0], states[2][1]
    states[3] = (w, (((K.ONE - K.EMA_DECAY) * w + K.EMA_DECAY * old * e) * new).astype(np.float32), states[3][2], states[3][3])
    with pytest.raises(AssertionError, match=r"step 3 EMA"):
        K.check_optimizer_trajectory(states[:4], pos_enc, HIDDEN, LR, min_untouched=0.0, min_touched_then_untouched=0)


def test_the_eps_shows_on_the_pad_rows(trajectory):
    """sqrt(v_1) of a pad row is 0.1 * 1e-6 |w| ~ 1e-8: the triangle-wave eps (1e-8) roughly halves its first step, the hash-grid eps
    (1e-15) does not -- K.check_pad_row_first_step is what the GPU test asserts for the two encodings."""
    pos_enc, _, _, states = trajectory
    K.check_pad_row_first_step(states[0][0], states[1][0], states[1][3], HIDDEN, LR, pos_enc)


def test_grid_chunk_leaves_the_default_alone_and_sums_the_whole_batch_when_asked():
    rng = np.random.default_rng(5)
    p = _random_params(rng, N.POS_HASHGRID, HIDDEN)
    x = _inputs(rng, 128 * 5)
    t = _targets(x)
    _, g_default = N.NrcNet(N.POS_HASHGRID, HIDDEN, params=p).gradients(x, t)
    _, g_rule = N.NrcNet(N.POS_HASHGRID, HIDDEN, params=p, grid_chunk=256).gradients(x, t)        # 640 records: the rule's chunk is 256
    assert np.array_equal(K.bits(g_default), K.bits(g_rule))
    _, g_whole = N.NrcNet(N.POS_HASHGRID, HIDDEN, params=p).gradients(x, t, grid_chunk=x.shape[0])
    grid_off = N.layout(N.POS_HASHGRID, HIDDEN)[1]
    assert np.array_equal(K.bits(g_default[:grid_off]), K.bits(g_whole[:grid_off]))
    grid = g_whole[grid_off:]
    assert np.array_equal(grid, grid.astype(np.float16).astype(np.float32)), "one chunk: every sum is an fp16 value"
    assert not np.array_equal(grid, g_default[grid_off:])
    _, g32 = N.NrcNet(N.POS_HASHGRID, HIDDEN, params=p, grid_grad_f16=False, grid_chunk=64).gradients(x, t)   # fp32 sums: no chunks
    _, g32_plain = N.NrcNet(N.POS_HASHGRID, HIDDEN, params=p, grid_grad_f16=False).gradients(x, t)
    assert np.array_equal(K.bits(g32), K.bits(g32_plain))
