"""Checking helpers of the NRC INFERENCE tests (tests/test_gpu_nrc_infer.py holds gfx_nrc_infer with them, tests/test_nrc_infer_checks_cpu.py runs
them against oracle/nrc_net.py and against deliberately wrong encoders and layers).  numpy only: no GPU, no library.

Two constructions make inference checkable without a statistical tolerance:

  selector weights   one +1 and one -1 in two rows of W0 at column f, identity rows for those two neurons in the further hidden matrices,
      +1 / -1 on them in one row of Wout: output o = relu(bf16(feat_f)) - relu(-bf16(feat_f)) = bf16(feat_f), every matrix sum has one
      non-zero term.  The network reads out its own encoding, three features per parameter set, 22 sets for the 64 features
      (selector_params).  A read-out feature is held against a FLOAT64 evaluation of the published definitions (ref_features) by the
      acceptance rule below.
  exactly summable networks   sparse dyadic weights on dyadic features: every product of a neuron is a multiple of one power of two g and
      sum |w a| < 2^24 g, so every partial sum in ANY order is an fp32 number: the accumulation is exact whatever the matrix unit does, the
      bf16 rounding of the activations is then a function of exact numbers, and the outputs are determined bit for bit (exact_network).

The acceptance rule.  A device feature r (a bf16 number) is accepted iff  bf16(F - delta) <= r <= bf16(F + delta)  (round to nearest even;
+0 and -0 compare equal), F the float64 reference, delta a bound on the fp32 evaluation error of ANY faithful implementation of the
definition, whatever its order of operations or use of fused multiply-adds (u = 2^-24, the relative error of one fp32 rounding):

  hash grid      delta = 2^-20 max|entry| over the query's 8 corner entries of the level.  pos = fl(fl(x scale) + 0.5), base = floor(pos) and
      frac = pos - base (exact) are fixed by the contract and taken as they are.  A corner weight is a product of three factors frac or
      fl(1 - frac): at most 3 roundings in the factors and 2 in the products, (1 + u)^5: relative error <= 5 u.  The blend adds eight
      terms w e: the products are exact under a fused multiply-add (one more rounding each without: it merges with the add's below), every
      add rounds a partial sum that is <= sum w |e| <= max|e| (1 + 5 u): 8 u max|e|.  Against sum w = 1: <= 13 u max|e| < 2^-20 max|e|.
  one-blob       delta = 2^-19.  A feature is the difference of two sums of three clamped CDF values Q in [0, 1].  The argument b/4 - x (-+ 1) is
      rounded at <= 2^-24 for |arg| < 2, <= 2^-23 for |arg| < 4 -- and a value off the clamp has |arg| <= 1/4 after the last operation, so
      the rounding that matters is <= 2^-25 in the argument (the first of two subtractions can add 2^-24 for |x| < 2): times Q' <= 3.75,
      <= 1.1e-7 per value; the polynomial itself (7 roundings of numbers <= 1) <= 7 u; a feature has at most two values off the clamp in
      each sum (the kernel spans two bins); the sums reach 3 and round at <= 2^-23 twice each, the difference once more: in all
      < 2 (3.75 (2^-24 + 2^-25) + 7 u) + 5 2^-23 = 3.1 2^-21 < 2^-19.
  triangle wave  delta = 2^-22.  x 2^(f-1) and floor are exact; xs - floor(xs) in [0, 1) rounds at <= 2^-25, - 0.5 is then exact or rounds
      at <= 2^-26 (frac < 2^-2); times 4: <= 2^-23; the last - 1 is exact on that grid or rounds at 2^-25: < 2^-22.
  identity, pad  delta = 0: the input itself, exactly 1.
"""
import numpy as np

from oracle import nrc_net as N

F32 = np.float32
U = 2.0 ** -24
BF16_MAX = (2.0 - 2.0 ** -7) * 2.0 ** 127
N_SETS = 22
N_VARIANTS = 8
PRIME_Y, PRIME_Z = 2654435761, 805459861


# ---------------------------------------------------------------- bf16 on float64

def bf16_rne(v):
    """float64 -> the nearest bf16 number (ties to even), as float64.  Exact: the quotient by the power-of-two spacing is exact."""
    v = np.asarray(v, np.float64)
    finite = np.isfinite(v)
    w = np.where(finite, v, 0.0)
    _, e = np.frexp(w)
    e = np.maximum(e, -125)                                   # subnormal bf16: spacing 2^-133
    ulp = np.ldexp(1.0, e - 8)
    r = np.rint(w / ulp) * ulp
    r = np.where(np.abs(r) > BF16_MAX, np.copysign(np.inf, r), r)
    return np.where(finite, r, v)


def is_bf16(a):
    """fp32 array: every element is a bf16 number (low 16 bits clear)."""
    return (np.ascontiguousarray(a, F32).view(np.uint32) & 0xFFFF) == 0


def canon_bits(a):
    """fp32 bits with -0 folded onto +0."""
    return (np.ascontiguousarray(a, F32) + F32(0)).view(np.uint32)


def rounding_interval(r):
    """[lo, hi] of the reals that round to the bf16 number r (float64 arrays; the end points are ties)."""
    r = np.asarray(r, np.float64)
    a = np.abs(r)
    m, e = np.frexp(a)
    e = np.where(a == 0, -125, np.maximum(e, -125))
    up = np.ldexp(1.0, e - 8)
    down = np.where((m == 0.5) & (e > -125), up / 2, up)
    a_lo, a_hi = np.where(a == 0, -up / 2, a - down / 2), a + up / 2
    return np.where(r >= 0, a_lo, -a_hi), np.where(r >= 0, a_hi, -a_lo)


def accept(r, F, delta):
    """The acceptance rule, element by element.  r: device features (bf16 numbers in any float type)."""
    r = np.asarray(r, np.float64)
    return (r >= bf16_rne(F - delta)) & (r <= bf16_rne(F + delta))


def ambiguous(F, delta):
    """More than one bf16 number is acceptable."""
    return bf16_rne(F - delta) != bf16_rne(F + delta)


def figures(r, F, delta):
    """Of the finite outputs: share equal to bf16(F), share and count that took another (the neighbouring) acceptable value, and the largest
    shift of F, in units of delta, that makes bf16(F) = r (0 where r = bf16(F); accepted means <= 1 up to ties)."""
    r = np.asarray(r, np.float64)
    ok = np.isfinite(r)
    exact = (r == bf16_rne(F)) & ok
    lo, hi = rounding_interval(np.where(ok, r, 0.0))
    dist = np.maximum(np.maximum(lo - F, F - hi), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        shift = np.where(dist == 0, 0.0, dist / delta)
    shift = np.where(ok, shift, 0.0)
    other = accept(r, F, delta) & ~exact & ok
    return {"exact": float(exact.sum() / max(ok.sum(), 1)), "neighbour": float(other.sum() / max(ok.sum(), 1)), "neighbour_count": int(other.sum()),
            "max_shift_over_delta": float(shift.max()) if shift.size else 0.0}


# ---------------------------------------------------------------- the published definitions in float64

def levels():
    """[(scale fp32, resolution, entries, offset, dense)]: scale = 16 * 2^l - 1, resolution = ceil(scale) + 1, a table of
    min(resolution^3 rounded up to 8, 2^15) entries, indexed densely while the level fits."""
    out, offset = [], 0
    for l in range(16):
        scale, res = F32(16 * 2 ** l - 1), 16 * 2 ** l
        entries = min((res ** 3 + 7) // 8 * 8, 1 << 15)
        out.append((scale, res, entries, offset, res ** 3 <= entries))
        offset += entries
    return out


def total_entries():
    return sum(lv[2] for lv in levels())


def _corner_index(ix, iy, iz, res, entries, dense, primes=(PRIME_Y, PRIME_Z)):
    """uint32 coordinates (int64 arrays, already wrapped) -> index inside the level's table; all arithmetic modulo 2^32."""
    M = np.uint64(0xFFFFFFFF)
    ix, iy, iz = ix.astype(np.uint64), iy.astype(np.uint64), iz.astype(np.uint64)       # products wrap modulo 2^64, a multiple of 2^32
    if dense:
        raw = (ix + iy * np.uint64(res) + iz * np.uint64(res * res)) & M
    else:
        raw = (ix ^ (iy * np.uint64(primes[0])) ^ (iz * np.uint64(primes[1]))) & M
    return (raw % np.uint64(entries)).astype(np.int64)


def _cells(x3, scale, half=True):
    """The discrete decisions as the contract fixes them: pos = fl32(fl32(x scale) + 0.5), base = floor(pos), frac = pos - base."""
    t = (np.ascontiguousarray(x3, F32) * scale).astype(F32)
    pos = (t + F32(0.5)).astype(F32) if half else t
    base = np.floor(pos)
    frac = (pos - base).astype(F32)
    if half:        # (a pos within 2^-25 under an integer from below zero would round frac to 1: no input of these tests is)
        assert np.array_equal(frac.astype(np.float64), pos.astype(np.float64) - base.astype(np.float64)), "frac is not exact"
    return base.astype(np.int64) & 0xFFFFFFFF, frac


def ref_hashgrid(x3, grid):
    """[N, 3] fp32, grid [entries, 2] of bf16 numbers -> (F [N, 32] float64, delta [N, 32]); feature 2 level + f."""
    n = x3.shape[0]
    g = np.asarray(grid, np.float64)
    F, D = np.zeros((n, 32)), np.zeros((n, 32))
    for l, (scale, res, entries, offset, dense) in enumerate(levels()):
        b, frac = _cells(x3, scale)
        fr = frac.astype(np.float64)
        acc, big = np.zeros((n, 2)), np.zeros((n, 2))
        for c in range(8):
            o = [(c >> k) & 1 for k in range(3)]
            idx = _corner_index((b[:, 0] + o[0]) & 0xFFFFFFFF, (b[:, 1] + o[1]) & 0xFFFFFFFF, (b[:, 2] + o[2]) & 0xFFFFFFFF, res, entries, dense) + offset
            w = np.ones(n)
            for k in range(3):
                w = w * (fr[:, k] if o[k] else 1.0 - fr[:, k])
            acc += w[:, None] * g[idx]
            big = np.maximum(big, np.abs(g[idx]))
        F[:, 2 * l:2 * l + 2] = acc
        D[:, 2 * l:2 * l + 2] = 2.0 ** -20 * big
    return F, D


def _Q(t):
    """CDF of the quartic kernel 15/16 (1 - u^2)^2 of radius 1/4, u = 4 t: the polynomial inside the radius, 0 and 1 outside."""
    u = 4.0 * t
    return np.clip(15.0 / 16.0 * u * (1.0 - 2.0 / 3.0 * u ** 2 + 1.0 / 5.0 * u ** 4) + 0.5, 0.0, 1.0)


def ref_oneblob(x5):
    """[N, 5] fp32 -> [N, 20] float64; feature 4 d + bin: the kernel centred on x, wrapped with period 1, integrated over the bin."""
    x = np.asarray(x5, F32).astype(np.float64)
    out = np.zeros((x.shape[0], 20))
    for d in range(5):
        cdf = [_Q(b / 4.0 - x[:, d]) + _Q(b / 4.0 - x[:, d] - 1.0) + _Q(b / 4.0 - x[:, d] + 1.0) for b in range(5)]
        for b in range(4):
            out[:, 4 * d + b] = cdf[b + 1] - cdf[b]
    return out


def ref_trianglewave(x3):
    """[N, 3] fp32 -> [N, 36] float64; feature 12 d + f: |frac(x 2^(f-1)) - 0.5| 4 - 1."""
    x = np.asarray(x3, F32).astype(np.float64)
    out = np.zeros((x.shape[0], 36))
    for d in range(3):
        for f in range(12):
            xs = np.ldexp(x[:, d], f - 1)
            out[:, 12 * d + f] = np.abs(xs - np.floor(xs) - 0.5) * 4.0 - 1.0
    return out


def assemble(pos, ob, ident, pad_value=1.0):
    feat = np.concatenate([pos, ob, ident], axis=1)
    return np.concatenate([feat, np.full((feat.shape[0], 64 - feat.shape[1]), pad_value, feat.dtype)], axis=1)


def blocks(pos_enc):
    """{name: slice of the 64 canonical features}."""
    p = 32 if pos_enc == N.POS_HASHGRID else 36
    return {"position": slice(0, p), "oneblob": slice(p, p + 20), "identity": slice(p + 20, p + 26), "pad": slice(p + 26, 64)}


def ref_features(pos_enc, x, grid=None):
    """(F, delta): float64 [N, 64] each, the canonical features of inputs x [N, 14] and their acceptance half-widths."""
    x = np.ascontiguousarray(x, F32)
    n = x.shape[0]
    if pos_enc == N.POS_HASHGRID:
        pos, dpos = ref_hashgrid(x[:, 0:3], grid)
    else:
        pos = ref_trianglewave(x[:, 0:3])
        dpos = np.full(pos.shape, 2.0 ** -22)
    F = assemble(pos, ref_oneblob(x[:, 3:8]), x[:, 8:14].astype(np.float64))
    D = assemble(dpos, np.full((n, 20), 2.0 ** -19), np.zeros((n, 6)), pad_value=0.0)
    return F, D


# ---------------------------------------------------------------- faithful fp32 forms and their mutants (the CPU test)

MUTANTS = ("corner_weight", "primes_swapped", "dense_level_2", "no_half", "oneblob_no_wrap", "oneblob_bins_shifted", "triangle_octave",
           "pad_zero", "identity_permuted")


def fp32_hashgrid(x3, grid, fused=False, mutant=None):
    """oracle/nrc_net.py's encode_hashgrid restated (bit-equal without `fused` and `mutant`); fused: the blend as a chain of fused
    multiply-adds in corner order (product and sum in float64, one rounding to fp32: a float64 product of a 24-bit and an 8-bit
    significand is exact)."""
    n = x3.shape[0]
    g = np.ascontiguousarray(grid, F32)
    out = np.zeros((n, 32), F32)
    for l, (scale, res, entries, offset, dense) in enumerate(levels()):
        b, frac = _cells(x3, scale, half=mutant != "no_half")
        acc = np.zeros((n, 2), F32)
        for c in range(8):
            o = [(c >> k) & 1 for k in range(3)]
            idx = _corner_index((b[:, 0] + o[0]) & 0xFFFFFFFF, (b[:, 1] + o[1]) & 0xFFFFFFFF, (b[:, 2] + o[2]) & 0xFFFFFFFF, res, entries,
                                dense or (mutant == "dense_level_2" and l == 2),
                                (PRIME_Z, PRIME_Y) if mutant == "primes_swapped" else (PRIME_Y, PRIME_Z)) + offset
            w = np.ones(n, F32)
            for k in range(3):
                upper = bool(o[k]) != (mutant == "corner_weight" and l == 11 and c == 5 and k == 1)     # one factor of one corner of one fine level
                w = w * (frac[:, k] if upper else F32(1) - frac[:, k])
            if fused:
                acc = (w.astype(np.float64)[:, None] * g[idx].astype(np.float64) + acc.astype(np.float64)).astype(F32)
            else:
                acc = acc + w[:, None] * g[idx]
        out[:, 2 * l:2 * l + 2] = acc
    return out


def _q32(t):
    u = (t * F32(4)).astype(F32)
    u2 = u * u
    u4 = u2 * u2
    v = F32(15.0 / 16.0) * u * (F32(1) - F32(2.0 / 3.0) * u2 + F32(1.0 / 5.0) * u4) + F32(0.5)
    return np.clip(v, F32(0), F32(1)).astype(F32)


def fp32_oneblob(x5, five=False, mutant=None):
    """encode_oneblob restated; five: the form for x in [0, 1] that takes the ten integrals on the clamp as 0 or 1 (the kernel's)."""
    n = x5.shape[0]
    out = np.zeros((n, 20), F32)
    shift = 1 if mutant == "oneblob_bins_shifted" else 0
    for d in range(5):
        x = np.ascontiguousarray(x5[:, d], F32)
        cdf = []
        for b in range(shift, 5 + shift):
            left = F32(b / 4)
            q = _q32(left - x)
            if five:
                below = _q32(F32(0) - x) if b == 4 else np.zeros(n, F32)
                above = _q32(F32(1) - x) if b == 0 else np.ones(n, F32)
            else:
                below, above = _q32(left - x - F32(1)), _q32(left - x + F32(1))
            if mutant == "oneblob_no_wrap":
                below, above = np.zeros(n, F32), np.zeros(n, F32)
            cdf.append((q + below + above).astype(F32))
        for b in range(4):
            out[:, 4 * d + b] = cdf[b + 1] - cdf[b]
    return out


def fp32_trianglewave(x3, mutant=None):
    out = np.zeros((x3.shape[0], 36), F32)
    for d in range(3):
        for f in range(12):
            xs = np.ldexp(np.ascontiguousarray(x3[:, d], F32), f if mutant == "triangle_octave" else f - 1).astype(F32)
            out[:, 12 * d + f] = np.abs(xs - np.floor(xs) - F32(0.5)) * F32(4) - F32(1)
    return out


def fp32_features(pos_enc, x, grid=None, mutant=None, fused=False):
    """[N, 64] fp32 BEFORE the bf16 rounding, from the forms above."""
    x = np.ascontiguousarray(x, F32)
    pos = fp32_hashgrid(x[:, 0:3], grid, fused, mutant) if pos_enc == N.POS_HASHGRID else fp32_trianglewave(x[:, 0:3], mutant)
    ident = x[:, 8:14]
    if mutant == "identity_permuted":
        ident = np.roll(ident, 1, axis=1)
    return assemble(pos, fp32_oneblob(x[:, 3:8], False, mutant), ident, F32(0 if mutant == "pad_zero" else 1))


# ---------------------------------------------------------------- inputs

def feature_grid(seed=4):
    """[entries, 2] fp32: bf16 numbers of order 1, so that a wrong corner or weight moves a feature by many bf16 steps."""
    rng = np.random.default_rng(seed)
    return N.bf16_round((rng.random((total_entries(), 2)) * 2 - 1).astype(F32))


def _ulps(v):
    v = F32(v)
    return [np.nextafter(v, F32(-np.inf)), v, np.nextafter(v, F32(np.inf))]


def position_edges():
    e = [F32(0), F32(1), np.nextafter(F32(1), F32(0)), F32(-0.0), F32(1e-40), F32(-1e-3), F32(1.001),
         F32(10.37), F32(-12.5), F32(100.123), F32(999.9), F32(-1000.25), F32(3000.0)]
    for scale, res, _, _, _ in levels():                      # on and one ulp either side of a cell boundary, pos = k
        k = res // 3 + 1
        e += _ulps(F32(k - 0.5) / scale)
    return np.array(e, F32)


def oneblob_edges():
    """(in range, out of range)."""
    inside, outside = [F32(1e-40)], [F32(-3), F32(-2.2), F32(-1.25), F32(-1), F32(-0.3), F32(1.1), F32(1.25), F32(1.75), F32(2), F32(2.25), F32(3), F32(-1e-40)]
    for b in range(5):
        for v in _ulps(0.25 * b):
            (inside if 0 <= v <= 1 else outside).append(v)
    inside.append(F32(-0.0))                                  # -0 >= 0: in range
    return np.array(inside, F32), np.array(outside, F32)


IDENTITY_EDGES = np.array([0.0, -0.0, 1.0, -1.0, 1e6, -1e6, 65504.0, -3.0e38, 0.333], F32)


def edge_inputs(n, seed=0):
    """[n, 14] fp32, n a multiple of 128: every edge of the module docstring's three kinds of input, the rest random.  Tiles of 64 queries
    (one wave of k_nrc_infer): in an even tile every one-blob input is in [0, 1] (the five-integral form only), in an odd tile half of
    them are not (both forms inside one wave).  No non-finite value."""
    assert n >= 128 and n % 128 == 0
    rng = np.random.default_rng(seed)
    x = rng.random((n, 14)).astype(F32)
    x[:, 8:14] = x[:, 8:14] * 4 - 2
    pe = position_edges()
    corners = np.array([[0, 0, 0], [1, 1, 1], [-0.0, -0.0, -0.0], [1.001, 1.001, 1.001], [-1e-3, -1e-3, -1e-3], [np.nextafter(F32(1), F32(0))] * 3], F32)
    assert 2 * len(pe) <= n - len(corners)
    for d, rows in enumerate((2 * np.arange(len(pe)), 2 * np.arange(len(pe)) + 1, np.arange(len(pe)))):
        x[rows, d] = pe                                       # every edge in every dimension, beside random or other-edge coordinates
    x[n - len(corners):, 0:3] = corners                       # whole-vector edges in the last tile's lanes
    tile = np.arange(n) // 64
    odd = np.flatnonzero(tile % 2 == 1)
    spread = odd[rng.random(odd.size) < 0.5]
    x[spread, 3:8] = (rng.random((spread.size, 5)) * 6 - 3).astype(F32)
    inside, outside = oneblob_edges()
    even = np.flatnonzero(tile % 2 == 0)
    for d in range(5):
        qi = even[(np.arange(len(inside)) * 2 + d) % even.size]
        x[qi, 3 + d] = inside
        qo = odd[(np.arange(len(outside)) * 2 + d) % odd.size]
        x[qo, 3 + d] = outside
    for d in range(6):
        x[(np.arange(len(IDENTITY_EDGES)) * 3 + d) % n, 8 + d] = IDENTITY_EDGES
    assert np.isfinite(x).all()
    ob = x[:, 3:8]
    in_range = ((ob >= 0) & (ob <= 1)).all(axis=1)
    assert in_range[even].all() and (~in_range[odd]).any() and in_range[odd].any()
    for t in np.unique(tile[odd]):                            # every odd tile holds both forms
        assert 0 < in_range[tile == t].sum() < 64
    return x


# ---------------------------------------------------------------- selector parameter sets

def selector_features(set_index):
    return [(3 * set_index + k) % 64 for k in range(3)]


def selector_neurons(set_index):
    """[(plus, minus)] hidden rows that carry the set's three features: they rotate so that over the 22 sets every row carries one."""
    return [((6 * set_index + 2 * k) % 64, (6 * set_index + 2 * k + 1) % 64) for k in range(3)]


def selector_params(pos_enc, hidden, set_index, grid=None):
    """Parameter blob (gfx_nrc_set_params layout) whose output o is bf16(feature selector_features(set_index)[o]) exactly."""
    assert 1 <= hidden <= 5 and 0 <= set_index < N_SETS
    table, grid_off, total = N.layout(pos_enc, hidden)
    p = np.zeros(total, F32)
    mats = {k: p[off:off + rows * cols].reshape(rows, cols) for k, (off, rows, cols) in table.items()}      # views
    for o, (f, (jp, jm)) in enumerate(zip(selector_features(set_index), selector_neurons(set_index))):
        mats["W0"][jp, f], mats["W0"][jm, f] = 1, -1
        for i in range(1, hidden):
            mats[f"W{i}"][jp, jp] = mats[f"W{i}"][jm, jm] = 1
        mats["Wout"][o, jp], mats["Wout"][o, jm] = 1, -1
    if pos_enc == N.POS_HASHGRID:
        p[grid_off:] = np.ascontiguousarray(grid, F32).reshape(-1)
    return p


# ---------------------------------------------------------------- exactly summable networks

G = 2.0 ** -6           # every product of every neuron is a multiple of G: features k / 32, W0 in {+-1, +-1/2}, deeper weights +-1


def _w0_columns(pos_enc):
    """The 44 W0 columns outside the one-blob block, in an order that puts a live (identity or pad) column
    into every window of 8 also when the 32 hash features are zero."""
    ob = blocks(pos_enc)["oneblob"]
    allowed = [c for c in range(64) if not ob.start <= c < ob.stop]
    return [allowed[(i * 5) % len(allowed)] for i in range(len(allowed))]


def _pattern(pos_enc, hidden, variant):
    """Non-zero positions: {matrix name: bool [rows, 64]}, 8 per row, shifted cyclically by 8 per variant."""
    table, _, _ = N.layout(pos_enc, hidden)
    cols0 = _w0_columns(pos_enc)
    out = {}
    for name, (_, rows, _) in table.items():
        m = np.zeros((rows, 64), bool)
        for r in range(rows):
            for j in range(8):
                if name == "W0":
                    m[r, cols0[(3 * r + 8 * variant + j) % len(cols0)]] = True
                elif name == "Wout":
                    m[r, (21 * r + 8 * variant + j) % 64] = True
                else:
                    m[r, (5 * r + 11 * int(name[1:]) + 8 * variant + j) % 64] = True
        out[name] = m
    return out


def exact_network_coverage(pos_enc, hidden):
    """Over the variants every (out, in) position of every hidden matrix and of Wout is non-zero once, and every W0 position outside the
    one-blob columns (none inside)."""
    seen = None
    for v in range(N_VARIANTS):
        pat = _pattern(pos_enc, hidden, v)
        seen = pat if seen is None else {k: seen[k] | pat[k] for k in pat}
    ob = blocks(pos_enc)["oneblob"]
    for name, m in seen.items():
        if name == "W0":
            assert not m[:, ob].any() and np.delete(m, np.arange(ob.start, ob.stop), axis=1).all(), name
        else:
            assert m.all(), name
    return seen


def exact_network(pos_enc, hidden, variant, n=128):
    """{"params", "x", "ref" [n, 3] fp32, "proof"}: a network and a batch whose outputs are determined bit for bit (module docstring), the
    reference computed in float64 on numbers that float64 holds exactly.  Asserts for every neuron of every layer and every query that all
    products are multiples of G and sum |w a| < 2^24 G, and that the network is not trivial: every hidden neuron non-zero for some query
    (in fact for a quarter of them: a row's signs are re-drawn until it is), the three outputs not constant and not equal."""
    assert 1 <= hidden <= 5 and 0 <= variant < N_VARIANTS and n % 128 == 0
    rng = np.random.default_rng(9000 + 1000 * pos_enc + 10 * hidden + variant)
    table, grid_off, total = N.layout(pos_enc, hidden)
    x = rng.random((n, 14)).astype(F32)
    if pos_enc == N.POS_TRIANGLEWAVE:
        x[:, 0:3] = (rng.integers(0, 64, (n, 3)) / 64.0).astype(F32)
    x[:, 8:14] = (rng.integers(-32, 33, (n, 6)) / 16.0).astype(F32)
    grid = np.zeros((total_entries(), 2), F32)
    a, _ = ref_features(pos_enc, x, grid)
    ob = blocks(pos_enc)["oneblob"]
    assert np.isfinite(a).all()
    a[:, ob] = 0.0                                             # W0 is zero there: finite feature x 0
    assert np.array_equal(a, np.rint(a * 32) / 32) and np.array_equal(a, bf16_rne(a)) and np.abs(a).max() <= 2

    pat = _pattern(pos_enc, hidden, variant)
    p = np.zeros(total, F32)
    names = ["W0"] + [f"W{i}" for i in range(1, hidden)] + ["Wout"]
    proof = {"worst_sum_over_2^24_G": 0.0, "active": []}

    def draw(name, row):
        w = np.zeros(64)
        k = int(pat[name][row].sum())
        mag = rng.choice([1.0, 0.5], k) if name == "W0" else np.ones(k)
        w[pat[name][row]] = mag * rng.choice([1.0, -1.0], k)
        return w

    for name in names:
        off, rows, cols = table[name]
        W = np.zeros((rows, 64))
        for r in range(rows):
            for _ in range(200):
                W[r] = draw(name, r)
                pre = a @ W[r]
                if name == "Wout" or np.mean(pre > 0) >= 0.25:
                    if name != "Wout" or r >= 3 or (np.unique(pre).size >= 4 and all(not np.array_equal(pre, a @ W[q]) for q in range(r))):
                        break
            else:
                raise AssertionError(f"{name} row {r}: no live sign pattern found")
        assert np.array_equal(a, np.rint(a / G) * G), name      # every input a multiple of G; |w| in {1, 1/2} with 1/2 only on multiples of 2 G
        if name == "W0":
            assert np.array_equal(a, np.rint(a / (2 * G)) * (2 * G))
        worst = (np.abs(a) @ np.abs(W).T).max()
        assert worst < 2.0 ** 24 * G, (name, worst)
        proof["worst_sum_over_2^24_G"] = max(proof["worst_sum_over_2^24_G"], float(worst / (2.0 ** 24 * G)))
        pre = a @ W.T                                          # exact: float64 holds every partial sum
        p[off:off + rows * cols] = W.astype(F32).reshape(-1)
        if name == "Wout":
            ref = pre[:, :3].astype(F32)
            assert np.array_equal(ref.astype(np.float64), pre[:, :3])
        else:
            a = bf16_rne(np.maximum(pre, 0.0))
            assert (a > 0).any(axis=0).all(), f"{name}: a neuron is zero for every query"
            assert np.mean(a > 0) >= 0.25, name
            proof["active"].append(float(np.mean(a > 0)))
    assert all(np.unique(ref[:, o]).size > 1 for o in range(3)) and not np.array_equal(ref[:, 0], ref[:, 1]) and not np.array_equal(ref[:, 1], ref[:, 2])
    return {"params": p, "x": x, "ref": ref, "proof": proof}
