"""Checking helpers of the NRC training-step tests (tests/test_gpu_nrc_train.py holds gfx_nrc_train with them, tests/test_nrc_optimizer_cpu.py
runs them against oracle/nrc_net.py itself and against three deliberately wrong optimizers).  numpy only: no GPU, no library.

A "device" here is anything that trains and hands out its four state arrays: the C ABI network (get_params(0..3)) or oracle NrcNet.
The optimizer is checked FROM THE DEVICE'S OWN STATE: step t is restated from the device's m_t, v_t, w_{t-1}, ema_{t-1}, so the bf16
drift between a kernel and the restatement never enters and every comparison is bit for bit (or a derived bound, check_moments)."""
import numpy as np

from oracle import nrc_net as N

F32 = np.float32
ONE = F32(1)
BETA1, BETA2, L2_REG, EMA_DECAY = F32(0.9), F32(0.99), F32(1e-6), F32(0.99)
STATE_NAMES = ("weights", "EMA", "Adam m", "Adam v")


def eps_of(pos_enc):
    return F32(1e-15 if pos_enc == N.POS_HASHGRID else 1e-8)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---------------------------------------------------------------- one training step against the oracle (parts 1 and 2)

def grid_reference_distance(g_mirror, g_f32sum, grid_off):
    """|| g(fp16 sums) - g(fp32 sums) || / || g(fp32 sums) || over the hash-grid entries: what the precision contract itself costs."""
    a, b = g_mirror[grid_off:].astype(np.float64), g_f32sum[grid_off:].astype(np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def check_step_against_oracle(label, loss, m_dev, ref, ref_loss, g_mirror, g_f32sum):
    """The assertions of test_gpu_nrc_net.py::test_one_training_step_matches_oracle with its bounds (loss 2e-3 relative, MLP part of
    Adam's first moment 1e-2 relative L2, the same hash-grid entries touched for more than 99.9 %), and the hash-grid gradient
    m[grid_off:] / 0.1 against the oracle's fp32-sum gradient within max(1e-2, 2 x the oracle's own fp16-sum-to-fp32-sum distance).
    ref: the oracle AFTER the same step in the mode that mirrors the device; g_mirror / g_f32sum: its loss-scaled gradient and the
    fp32-sum one (the same array when the device sums in fp32).  Prints the figures before it asserts; returns them."""
    grid_off = ref.grid_off
    fig = {"case": label, "loss_rel": abs(loss - ref_loss) / abs(ref_loss)}
    fig["m_mlp_rel"] = float(np.linalg.norm(m_dev[:grid_off] - ref.m[:grid_off]) / np.linalg.norm(ref.m[:grid_off]))
    if ref.pos_enc == N.POS_HASHGRID:
        fig["touched_agree"] = float(np.mean((m_dev[grid_off:] != 0) == (ref.m[grid_off:] != 0)))
        g_dev = (m_dev[grid_off:] / F32(0.1)).astype(np.float64)
        g32 = (g_f32sum[grid_off:] / F32(128.0)).astype(np.float64)
        fig["grid_rel"] = float(np.linalg.norm(g_dev - g32) / np.linalg.norm(g32))
        fig["grid_ref_distance"] = grid_reference_distance(g_mirror, g_f32sum, grid_off)
        fig["grid_bound"] = max(1e-2, 2.0 * fig["grid_ref_distance"])
    print("NRC-TRAIN-FIGURES", {k: (v if isinstance(v, str) else float(f"{v:.4g}")) for k, v in fig.items()})
    assert abs(loss - ref_loss) <= 2e-3 * abs(ref_loss) + 1e-6, (label, loss, ref_loss)
    assert fig["m_mlp_rel"] <= 1e-2, (label, fig)
    if ref.pos_enc == N.POS_HASHGRID:
        assert fig["touched_agree"] > 0.999, (label, fig)
        assert fig["grid_rel"] <= fig["grid_bound"], (label, fig)
    return fig


def reached_entries(x, total_grid_params):
    """bool per hash-grid PARAMETER: some record's trilinear footprint contains the entry (whatever its weight or gradient)."""
    hit = np.zeros(total_grid_params // N.HASH_FEATURES, bool)
    for idx, _ in N.hash_corners(np.ascontiguousarray(x[:, 0:3], F32)):
        hit[idx.reshape(-1)] = True
    return np.repeat(hit, N.HASH_FEATURES)


# ---------------------------------------------------------------- the optimizer from its own state (part 3)

def host_scalars(lr, t):
    """lrT, debiasOld, debiasNew of step t: double arithmetic rounded to fp32 once, the expressions of NrcNet.optimizer_step."""
    lr_t = F32(float(F32(lr)) * np.sqrt(1.0 - float(BETA2) ** t) / (1.0 - float(BETA1) ** t))
    d = F32(EMA_DECAY)
    debias_old = F32(1.0 - float(d) ** (t - 1))
    debias_new = F32(1.0 / (1.0 - float(d) ** t))
    return lr_t, debias_old, debias_new


def restate_weights_and_ema(m_t, v_t, w_prev, ema_prev, active, lr, t, eps):
    """w_t and ema_t from the moments AFTER the step and the weights / EMA BEFORE it: fp32, NrcNet.optimizer_step's operation order."""
    lr_t, debias_old, debias_new = host_scalars(lr, t)
    with np.errstate(divide="ignore", invalid="ignore"):
        upd = (lr_t * m_t / (np.sqrt(v_t) + eps)).astype(F32)
    w = np.where(active, w_prev - upd, w_prev).astype(F32)
    d = F32(EMA_DECAY)
    ema = (((ONE - d) * w + d * debias_old * ema_prev) * debias_new).astype(F32)
    return w, ema


def find_step1_gradient(m1, v1):
    """Step 1 starts from m = v = 0: some fp32 g within 4 ulp of m_1 / (1 - beta1) must give m_1 = (1 - beta1) g AND
    v_1 = ((1 - beta2) g) g in every bit.  Returns (g, found)."""
    g0 = (m1.astype(np.float64) / float(ONE - BETA1)).astype(F32)
    zero = g0 == 0
    g, found = g0.copy(), np.zeros(m1.shape, bool)
    for k in range(-4, 5):
        cand = np.where(zero, g0, (bits(g0).astype(np.int64) + k).astype(np.uint32).view(F32)).astype(F32)
        with np.errstate(over="ignore", invalid="ignore"):
            ok = (bits((ONE - BETA1) * cand) == bits(m1)) & (bits(((ONE - BETA2) * cand) * cand) == bits(v1)) & ~found
        g[ok] = cand[ok]
        found |= ok
    return g, found


def moment_violations(m_t, v_t, m_prev, v_prev, active):
    """Steps after the first: g^ = (m_t - beta1 m_prev) / (1 - beta1) in double; |v_t - (beta2 v_prev + (1 - beta2) g^2)| must stay within
    (1 - beta2) 2 |g^| delta + 4 ulp(v_t), delta = 10 * 2^-23 (|m_t| + |m_prev|): m_t carries three fp32 roundings of terms no larger than
    |m_t| + |m_prev|, divided by 1 - beta1 = 0.1 (the cancellation error of recovering g), and v_t four roundings of terms <= v_t.
    (The second-order term (1 - beta2) delta^2 is below 1e-11 v_t because m^2 <= 5.5 v for these betas: far inside the 4 ulp.)
    Returns the indices that violate it."""
    b1, b2 = float(BETA1), float(BETA2)
    om1, om2 = float(ONE - BETA1), float(ONE - BETA2)
    m64, mp64 = m_t.astype(np.float64), m_prev.astype(np.float64)
    g_hat = (m64 - b1 * mp64) / om1
    delta = 10.0 * 2.0 ** -23 * (np.abs(m64) + np.abs(mp64))
    want = b2 * v_prev.astype(np.float64) + om2 * g_hat * g_hat
    tol = om2 * 2.0 * np.abs(g_hat) * delta + 4.0 * np.spacing(np.abs(v_t)).astype(np.float64)
    return np.flatnonzero(active & ~(np.abs(v_t.astype(np.float64) - want) <= tol))


def fixed_point_touch(m0, v0, v1):
    """For entries whose m did not change although v or w did: True where some fp32 g within 32 ulp of m_0 (0.1 |g - m| must stay below
    an ulp of m for the rounding to return m) gives beta1 m_0 + (1 - beta1) g = m_0 AND beta2 v_0 + ((1 - beta2) g) g = v_1 in every bit."""
    found = np.zeros(m0.shape, bool)
    for k in range(-32, 33):
        cand = (bits(m0).astype(np.int64) + k).astype(np.uint32).view(F32)
        with np.errstate(over="ignore", invalid="ignore"):
            found |= (bits(BETA1 * m0 + (ONE - BETA1) * cand) == bits(m0)) & (bits(BETA2 * v0 + ((ONE - BETA2) * cand) * cand) == bits(v1)) & (m0 != 0)
    return found


def pad_row_slice(hidden):
    """Rows N_OUT .. OUT_PAD-1 of Wout: no output feeds them, their data gradient is exactly zero."""
    off, rows, cols = N.layout(N.POS_TRIANGLEWAVE, hidden)[0]["Wout"]
    return slice(off + N.N_OUT * cols, off + rows * cols)


def check_optimizer_trajectory(states, pos_enc, hidden, lr, min_untouched=0.2, min_touched_then_untouched=1000):
    """states[t] = (w, ema, m, v) after t training steps (states[0]: before the first), read back from the device.  Every step is held
    from the device's own previous state; raises AssertionError naming the step and the rule.  Returns the counts it measured."""
    grid_off = N.layout(pos_enc, hidden)[1]
    total = states[0][0].size
    is_grid = np.arange(total) >= grid_off
    eps = eps_of(pos_enc)
    assert not states[0][2].any() and not states[0][3].any(), "the moments do not start at zero"
    ever_touched = np.zeros(total, bool)
    dropped = np.zeros(total, bool)            # touched at some step, untouched at a later one
    stats = {"untouched_fraction": [], "fixed_point_touches": 0}
    for t in range(1, len(states)):
        (w0, e0, m0, v0), (w1, e1, m1, v1) = states[t - 1], states[t]
        assert all(np.isfinite(a).all() for a in (w1, e1, m1, v1)), f"step {t}: non-finite state"
        kept = bits(m1) == bits(m0)
        # untouched hash-grid entries: m unchanged <=> v and w unchanged, bit for bit
        untouched = is_grid & kept
        bad = np.flatnonzero(untouched & ((bits(v1) != bits(v0)) | (bits(w1) != bits(w0))))
        # a TOUCHED entry keeps its m when its gradient is m itself to within a few ulp (beta1 m + (1 - beta1) g rounds back to m): a
        # couple of entries in a million-entry run.  Such an entry must prove the touch bit for bit, then it is held like any touched one.
        fixed = fixed_point_touch(m0[bad], v0[bad], v1[bad])
        stats["fixed_point_touches"] += int(fixed.sum())
        untouched[bad[fixed]] = False
        bad = bad[~fixed]
        assert bad.size == 0, f"step {t}: {bad.size} untouched hash-grid entries changed their second moment or weight (first {bad[0]})"
        active = ~untouched
        if total > grid_off:
            stats["untouched_fraction"].append(float(untouched[grid_off:].mean()))
            dropped |= untouched & ever_touched
            ever_touched |= is_grid & ~kept
        # moments
        if t == 1:
            _, found = find_step1_gradient(m1, v1)
            bad = np.flatnonzero(~found)
            assert bad.size == 0, (f"step 1 moments: for {bad.size} of {total} parameters no fp32 g within 4 ulp gives both m_1 = (1 - beta1) g and "
                                   f"v_1 = ((1 - beta2) g) g (first {bad[0]}: m {m1[bad[0]]!r} v {v1[bad[0]]!r})")
            pad = pad_row_slice(hidden)
            want = ((ONE - BETA1) * (L2_REG * w0[pad])).astype(F32)
            bad = np.flatnonzero(bits(m1[pad]) != bits(want))
            assert bad.size == 0, f"step 1 L2 term: {bad.size} of {want.size} pad-row moments are not (1 - beta1) (1e-6 w) bit for bit"
        else:
            bad = moment_violations(m1, v1, m0, v0, active)
            assert bad.size == 0, (f"step {t} second moment: {bad.size} of {total} parameters outside beta2 v + (1 - beta2) g^2 "
                                   f"(first {bad[0]}: v {v1[bad[0]]!r} from {v0[bad[0]]!r}, m {m1[bad[0]]!r} from {m0[bad[0]]!r})")
        # weights and EMA, bit for bit
        w_want, e_want = restate_weights_and_ema(m1, v1, w0, e0, active, lr, t, eps)
        bad = np.flatnonzero(bits(w_want) != bits(w1))
        assert bad.size == 0, (f"step {t} weights: {bad.size} of {total} differ from the restatement (first {bad[0]}: {w1[bad[0]]!r} "
                               f"want {w_want[bad[0]]!r})")
        bad = np.flatnonzero(bits(e_want) != bits(e1))
        assert bad.size == 0, (f"step {t} EMA: {bad.size} of {total} differ from the restatement (first {bad[0]}: {e1[bad[0]]!r} "
                               f"want {e_want[bad[0]]!r})")
    stats["touched_then_untouched"] = int(dropped.sum())
    if total > grid_off:
        assert min(stats["untouched_fraction"]) >= min_untouched, f"untouched hash-grid entries: {stats['untouched_fraction']}"
        assert stats["touched_then_untouched"] >= min_touched_then_untouched, f"touched, then untouched: {stats['touched_then_untouched']}"
    return stats


def check_pad_row_first_step(w0, w1, v1, hidden, lr, pos_enc):
    """Step 1 of a pad row of Wout: g = 1e-6 w exactly, so m_1 / sqrt(v_1) = +-1 and the step is lr s / (s + eps) with s = sqrt(v_1) =
    0.1 * 1e-6 |w| <= 2.8e-8 (Xavier bound sqrt(6 / 80) of Wout).  With the hash-grid eps (1e-15) that is lr itself; with the
    triangle-wave eps (1e-8) it is lr s / (s + 1e-8): below 0.74 lr everywhere and lr / 2 on average.  Returns step / lr per entry
    with |w| > 1e-3 (a smaller weight's s comes near either eps)."""
    pad = pad_row_slice(hidden)
    sel = np.abs(w0[pad]) > 1e-3
    assert sel.sum() > 700, sel.sum()
    rel = (np.abs(w1[pad].astype(np.float64) - w0[pad].astype(np.float64)) / float(F32(lr)))[sel]
    s = np.sqrt(v1[pad].astype(np.float64))[sel]
    want = s / (s + float(eps_of(pos_enc)))
    assert np.abs(rel - want).max() <= 1e-4, ("pad-row first step", float(np.abs(rel - want).max()))     # fp32 rounding of w - upd: ~1e-6
    if pos_enc == N.POS_HASHGRID:
        assert rel.min() > 0.999, ("hash grid: eps 1e-15 must not shorten the first step", float(rel.min()))
    else:
        assert rel.max() < 0.74 and 0.35 < rel.mean() < 0.65, ("triangle wave: eps 1e-8 must about halve the first step", float(rel.max()), float(rel.mean()))
    return rel


# ---------------------------------------------------------------- records

# one small box of positions per step (x[:, :3] = c_t + 0.05 U): the boxes of steps 1-2, 3-4 and 5-6 overlap by half, so entries of the
# fine levels are touched at one step and not at the next, and most of them never
BOX_CENTRES = ((0.10, 0.20, 0.30), (0.125, 0.20, 0.30), (0.60, 0.15, 0.70), (0.60, 0.175, 0.70), (0.35, 0.80, 0.45), (0.35, 0.80, 0.475))
BOX_SIDE = 0.05


def boxed_batches(inputs_fn, targets_fn, n, seed=41):
    """Six batches of fresh records, each confined to its own box."""
    rng = np.random.default_rng(seed)
    out = []
    for c in BOX_CENTRES:
        x = inputs_fn(rng, n)
        x[:, :3] = (np.asarray(c, F32) + F32(BOX_SIDE) * rng.random((n, 3), dtype=F32)).astype(F32)
        out.append((x, targets_fn(x)))
    return out
