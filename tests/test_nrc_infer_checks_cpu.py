"""The checks of tests/nrc_infer_checks.py without a GPU: the float64 reference and the acceptance rule hold oracle/nrc_net.py's encoders
(and the kernel's two other faithful forms: the five-integral one-blob, the fused blend) at no more than half of each delta, reject nine
wrong encoders, leave few outputs ambiguous; the selector parameter sets read the encoding out of NrcNet.infer bit for bit; NrcNet.infer
on the exactly summable networks equals their exact reference bit for bit and two wrong layer layouts do not.  What runs here is what
tests/test_gpu_nrc_infer.py asks of the kernels."""
import numpy as np
import pytest

from oracle import nrc_net as N
from tests import nrc_infer_checks as K

F32 = np.float32
ENCODINGS = [N.POS_HASHGRID, N.POS_TRIANGLEWAVE]
ENC_IDS = ["hashgrid", "trianglewave"]
N_EDGE = 128 * 25


@pytest.fixture(scope="module")
def edge():
    x, grid = K.edge_inputs(N_EDGE), K.feature_grid()
    return {"x": x, "grid": grid, "ref": {enc: K.ref_features(enc, x, grid) for enc in ENCODINGS}}


def _oracle_features(enc, x, grid):
    """oracle/nrc_net.py's own encoders, before the bf16 rounding."""
    pos = N.encode_hashgrid(x[:, 0:3], grid) if enc == N.POS_HASHGRID else N.encode_trianglewave(x[:, 0:3])
    return K.assemble(pos, N.encode_oneblob(x[:, 3:8]), x[:, 8:14], F32(1))


def _distance(v32, F, D, block):
    """max |v - F| / delta over a block (delta = 0: the values must be equal)."""
    v, f, d = v32[:, block].astype(np.float64), F[:, block], D[:, block]
    if not d.any():
        assert np.array_equal(v, f)
        return 0.0
    assert (d > 0).all() or np.array_equal(v[d == 0], f[d == 0])
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(d > 0, np.abs(v - f) / d, 0.0).max())


def test_level_table_is_the_oracle_layout():
    ours, (theirs, total) = K.levels(), N.grid_levels()
    assert total == K.total_entries() and len(ours) == len(theirs) == N.HASH_LEVELS
    for (scale, res, entries, offset, dense), (s2, r2, e2, o2) in zip(ours, theirs):
        assert (scale, res, entries, offset) == (s2, r2, e2, o2) and dense == (r2 ** 3 <= e2)
    assert [lv[4] for lv in ours] == [True, True] + [False] * 14


def test_bf16_on_float64_is_the_oracle_rounding():
    rng = np.random.default_rng(1)
    v = np.concatenate([rng.standard_normal(4096).astype(F32) * F32(10) ** rng.integers(-30, 30, 4096).astype(F32),
                        np.array([0, -0.0, 1, 1.00390625, 1.01171875, -1.00390625, 3.0e38, 3.4e38, 1e-40, 2.0 ** -133, 2.0 ** -134, 0.99609375 + 2.0 ** -9], F32)])
    assert np.array_equal(K.bf16_rne(v.astype(np.float64)).astype(F32), N.bf16_round(v))
    r = N.bf16_round(v[np.isfinite(N.bf16_round(v))]).astype(np.float64)
    lo, hi = K.rounding_interval(r)
    inside = lo + (hi - lo) * 0.25
    assert np.array_equal(K.bf16_rne(inside), r) and np.array_equal(K.bf16_rne(lo + (hi - lo) * 0.75), r)
    assert (K.bf16_rne(lo - (hi - lo) * 0.01) != r).all() and (K.bf16_rne(hi + (hi - lo) * 0.01) != r).all()


def test_edge_inputs_hold_their_edges():
    for n in (128, N_EDGE):
        x = K.edge_inputs(n)
        for d in range(3):
            assert np.isin(K.position_edges().view(np.uint32), x[:, d].view(np.uint32)).all()
        inside, outside = K.oneblob_edges()
        for d in range(5):
            assert np.isin(np.concatenate([inside, outside]).view(np.uint32), x[:, 3 + d].view(np.uint32)).all()
        for d in range(6):
            assert np.isin(K.IDENTITY_EDGES.view(np.uint32), x[:, 8 + d].view(np.uint32)).all()
        for scale, _, _, _, _ in K.levels():                  # |x scale + 0.5| < 2^31: the int conversion is defined
            assert np.abs(x[:, 0:3].astype(np.float64) * float(scale) + 0.5).max() < 2.0 ** 31
    # both sides of a cell boundary are reached at every level
    x = K.edge_inputs(128)
    for scale, res, _, _, _ in K.levels():
        base = np.floor((x[:, 0] * scale).astype(F32) + F32(0.5))
        k = res // 3 + 1
        assert (base == k).any() and (base == k - 1).any(), scale


@pytest.mark.parametrize("enc", ENCODINGS, ids=ENC_IDS)
def test_faithful_forms_sit_within_half_of_each_delta(edge, enc):
    x, grid = edge["x"], edge["grid"]
    F, D = edge["ref"][enc]
    oracle = _oracle_features(enc, x, grid)
    assert np.array_equal(K.fp32_features(enc, x, grid).view(np.uint32), oracle.view(np.uint32)), "fp32_features is not the oracle's arithmetic"
    forms = {"oracle": oracle}
    if enc == N.POS_HASHGRID:
        forms["fused blend"] = K.fp32_features(enc, x, grid, fused=True)
    five = oracle.copy()
    ob = K.blocks(enc)["oneblob"]
    in_range = np.repeat((x[:, 3:8] >= 0) & (x[:, 3:8] <= 1), 4, axis=1)
    five[:, ob] = np.where(in_range, K.fp32_oneblob(x[:, 3:8], five=True), oracle[:, ob])
    assert in_range.mean() > 0.5 and not np.array_equal(five, oracle)
    forms["five-integral one-blob"] = five
    for name, v in forms.items():
        dist = {b: _distance(v, F, D, sl) for b, sl in K.blocks(enc).items()}
        print("NRC-INFER-CPU", ENC_IDS[ENCODINGS.index(enc)], name, "max |v - F| / delta:", {b: float(f"{d:.3g}") for b, d in dist.items()})
        assert all(d <= 0.5 for d in dist.values()), (name, dist)
        assert K.accept(N.bf16_round(v), F, D).all(), name


@pytest.mark.parametrize("enc", ENCODINGS, ids=ENC_IDS)
def test_few_outputs_are_ambiguous(edge, enc):
    """Of the (query, feature) pairs with |F| >= 2^-8, those with more than one acceptable bf16 number are at most 5 %: the rule pins the
    rest to one value."""
    F, D = edge["ref"][enc]
    amb = K.ambiguous(F, D)
    for b, sl in K.blocks(enc).items():
        big = np.abs(F[:, sl]) >= 2.0 ** -8
        share = float(amb[:, sl][big].mean())
        print("NRC-INFER-CPU", ENC_IDS[ENCODINGS.index(enc)], b, f"ambiguous share {share:.4f} of {int(big.sum())} pairs")
        assert share <= 0.05, (b, share)
    big = np.abs(F) >= 2.0 ** -8
    assert amb[big].mean() <= 0.05


@pytest.mark.parametrize("mutant", K.MUTANTS)
def test_rule_rejects_wrong_encoders(edge, mutant):
    x, grid = edge["x"], edge["grid"]
    enc = N.POS_TRIANGLEWAVE if mutant == "triangle_octave" else N.POS_HASHGRID
    F, D = edge["ref"][enc]
    r = N.bf16_round(K.fp32_features(enc, x, grid, mutant=mutant))
    bad = ~K.accept(r, F, D)
    print("NRC-INFER-CPU mutant", mutant, f"{int(bad.sum())} outputs of {int(bad.any(axis=0).sum())} features rejected")
    assert bad.any(), mutant
    good = ~K.accept(N.bf16_round(K.fp32_features(enc, x, grid)), F, D)
    assert not good.any()


def test_selector_neurons_cover_every_hidden_row():
    rows = {j for s in range(K.N_SETS) for pair in K.selector_neurons(s) for j in pair}
    feats = {f for s in range(K.N_SETS) for f in K.selector_features(s)}
    assert rows == set(range(64)) and feats == set(range(64))
    for s in range(K.N_SETS):
        assert len({j for pair in K.selector_neurons(s) for j in pair}) == 6


@pytest.mark.parametrize("enc", ENCODINGS, ids=ENC_IDS)
@pytest.mark.parametrize("hidden", [1, 2, 5])
def test_selector_sets_read_the_encoding_out_of_the_oracle(edge, enc, hidden):
    x, grid = edge["x"][:128 * 4], edge["grid"]
    want = None
    for s in range(K.N_SETS):
        p = K.selector_params(enc, hidden, s, grid)
        net = N.NrcNet(enc, hidden, params=p)
        if want is None:
            want = net.encode(x, p)
        y = net.infer(x)
        assert K.is_bf16(y).all()
        assert np.array_equal(K.canon_bits(y), K.canon_bits(want[:, K.selector_features(s)])), (hidden, s)


@pytest.mark.parametrize("enc", ENCODINGS, ids=ENC_IDS)
@pytest.mark.parametrize("hidden", [1, 2, 3, 5])
def test_oracle_equals_the_exact_reference_on_summable_networks(enc, hidden):
    K.exact_network_coverage(enc, hidden)
    worst = 0.0
    for variant in range(K.N_VARIANTS):
        net = K.exact_network(enc, hidden, variant, 128 if variant else 128 * 25)
        y = N.NrcNet(enc, hidden, params=net["params"]).infer(net["x"])
        assert np.array_equal(K.canon_bits(y), K.canon_bits(net["ref"])), (hidden, variant)
        worst = max(worst, net["proof"]["worst_sum_over_2^24_G"])
    print("NRC-INFER-CPU exact networks", ENC_IDS[ENCODINGS.index(enc)], "hidden", hidden, f"largest sum |w a| / (2^24 G) = {worst:.3g}")


@pytest.mark.parametrize("enc", ENCODINGS, ids=ENC_IDS)
def test_exact_reference_rejects_wrong_layer_layouts(enc):
    hidden = 3
    net = K.exact_network(enc, hidden, 2)
    table, _, _ = N.layout(enc, hidden)

    def infer(p):
        return N.NrcNet(enc, hidden, params=p).infer(net["x"])

    assert np.array_equal(K.canon_bits(infer(net["params"])), K.canon_bits(net["ref"]))
    off, rows, cols = table["W1"]
    p = net["params"].copy()
    p[off:off + rows * cols] = p[off:off + rows * cols].reshape(rows, cols).T.reshape(-1)          # a hidden matrix transposed
    assert not np.array_equal(K.canon_bits(infer(p)), K.canon_bits(net["ref"]))
    off, rows, cols = table["W0"]
    p = net["params"].copy()
    W0 = p[off:off + rows * cols].reshape(rows, cols)
    ident = K.blocks(enc)["identity"]
    a, b = ident.start, ident.start + 1                                                          # two K slots of W0 swapped
    assert not np.array_equal(W0[:, a], W0[:, b])
    W0[:, [a, b]] = W0[:, [b, a]]
    assert not np.array_equal(K.canon_bits(infer(p)), K.canon_bits(net["ref"]))
