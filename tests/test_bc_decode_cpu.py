"""CPU: the block decoders of gfxexp_amd/csrc/bc/bc_decode.hip.h (the functions the expansion kernels call), compiled for the host
by tests/bc_host.py, against tools/dds_convert.py byte for byte: whole images at sizes with partial blocks, BC3-alpha / BC4 / BC5
exhaustively over all endpoint pairs and indices (unsigned and signed), BC1's palette cases, and BC7 blocks constructed to cover
every mode, partition, rotation and index selection."""
import numpy as np
import pytest

from tests import bc_host as B


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return B.compile_host(tmp_path_factory.mktemp("bc_host"))


def _check(host, name, blocks, w, h):
    got = B.host_decode(host, name, blocks, w, h)
    want = B.reference_decode(name, blocks, w, h)
    bad = np.argwhere((got != want).any(-1))
    assert len(bad) == 0, "%s %dx%d: %d texels differ, first at (y, x) = %s: %s, dds_convert %s" % (
        name, w, h, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("name", sorted(B.FORMATS))
def test_whole_images_equal_the_reference_decoder(host, name):
    rng = np.random.default_rng(B.FORMATS[name][0])
    for w, h in B.SIZES:
        _check(host, name, B.random_blocks(rng, name, w, h), w, h)
    assert host.bc_host_block_bytes(B.FORMATS[name][0]) == B.FORMATS[name][1]


@pytest.mark.parametrize("name", ["BC4U", "BC4S", "BC5U", "BC5S", "BC3"])
def test_alpha_blocks_exhaustively(host, name):
    blocks = B.exhaustive_blocks(np.random.default_rng(5), name)
    pairs = {(int(b[0]), int(b[1])) for b in blocks[:: 257]} | {(int(blocks[-1][0]), int(blocks[-1][1]))}
    assert len(blocks) == 65536 and (0, 0) in pairs and (255, 255) in pairs
    _check(host, name, blocks, 1024, 1024)


def test_bc1_palette_cases(host):
    blocks = B.bc1_edge_blocks(np.random.default_rng(6))
    c = blocks.view(np.uint16).reshape(-1, 4)
    n = len(blocks) // 4
    assert (c[n:2 * n, 0] <= c[n:2 * n, 1]).all() and (c[2 * n:3 * n, 0] == c[2 * n:3 * n, 1]).all() and (blocks[3 * n:, 4:] == 255).all()
    assert (c[:n, 0] > c[:n, 1]).any() and (c[3 * n:, 0] > c[3 * n:, 1]).any() and (c[3 * n:, 0] <= c[3 * n:, 1]).any()
    _check(host, "BC1", blocks, 4 * 64, 4 * len(blocks) // 64)
    for name in ("BC2", "BC3"):          # their colour half is four-colour whatever the endpoint order
        both = np.concatenate([np.random.default_rng(7).integers(0, 256, blocks.shape, dtype=np.uint8), blocks], 1)
        _check(host, name, both, 4 * 64, 4 * len(blocks) // 64)


def test_bc7_every_mode_partition_rotation_and_index_selection(host):
    blocks, w, h = B.bc7_texture(np.random.default_rng(8))
    B.assert_bc7_coverage(blocks)
    _check(host, "BC7", blocks, w, h)


def test_random_bc7_blocks_alone_would_not_cover_the_modes():
    """Why the BC7 case constructs its blocks: the mode is the position of the lowest set bit, so random blocks thin out by half per mode."""
    modes, _, _, _ = B.bc7_census(np.random.default_rng(9).integers(0, 256, (2048, 16), dtype=np.uint8))
    assert modes.get(0, 0) > 900 and modes.get(7, 0) < 64
