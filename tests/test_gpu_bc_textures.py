"""-m gpu: block-compressed textures through the C ABI.  gfx_texture_set_bc expands the blocks on the device into the slot's
8-bit format; gfx_texture_read shows the exact bytes of the pool.  The yardstick is tools/dds_convert.py, narrowed by the host
loader's rule (R8 / RG8 keep the first one / two channels): byte for byte for every format and output format, with partial blocks,
the exhaustive BC4 / BC5 / BC3 textures and the constructed BC7 set of tests/test_bc_decode_cpu.py; neighbouring slots stay
intact; the sampler, a rendered OBJ + MTL scene and the command line see a block texture exactly as they see its decoded texels."""
import os

import numpy as np
import pytest

from gfxexp_amd import api
from tests import bc_host as B
from tests import util

pytestmark = pytest.mark.gpu
D = B.D
CHANNELS = {api.TEX_RGBA8_SRGB: 4, api.TEX_RGBA8_UNORM: 4, api.TEX_RG8_UNORM: 2, api.TEX_R8_UNORM: 1}
OUT_FORMATS = [api.TEX_RGBA8_SRGB, api.TEX_RGBA8_UNORM, api.TEX_R8_UNORM, api.TEX_RG8_UNORM]


def _same(tag, got, want):
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bad = np.argwhere((got != want).reshape(got.shape[0], got.shape[1], -1).any(-1))
    assert len(bad) == 0, "%s: %d texels differ, first at (y, x) = %s: %s, dds_convert %s" % (tag, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def _expand(ctx, slot, name, blocks, w, h, fmt):
    ctx.texture_set_bc(slot, blocks, w, h, B.FORMATS[name][0], fmt)
    return ctx.texture_read(slot, w, h, fmt)


@pytest.mark.parametrize("name", sorted(B.FORMATS))
def test_expansion_equals_the_reference_decoder(built_lib, name):
    rng = np.random.default_rng(40 + B.FORMATS[name][0])
    ctx = api.Context(0)
    cases = [(w, h, B.random_blocks(rng, name, w, h)) for w, h in B.SIZES + [(1024, 1024)]]
    if name in ("BC4U", "BC4S", "BC5U", "BC5S", "BC3"):
        cases.append((1024, 1024, B.exhaustive_blocks(rng, name)))
    if name == "BC7":
        blocks, w, h = B.bc7_texture(rng)
        B.assert_bc7_coverage(blocks)
        cases.append((w, h, blocks))
    if name == "BC1":
        edge = B.bc1_edge_blocks(rng)
        cases.append((4 * 64, 4 * len(edge) // 64, edge))
    for w, h, blocks in cases:
        want = B.reference_decode(name, blocks, w, h)
        for slot, fmt in enumerate(OUT_FORMATS, 1):       # four slots alive at once: each expansion lands in its own region
            _same("%s %dx%d -> format %d" % (name, w, h, fmt), _expand(ctx, slot, name, blocks, w, h, fmt), B.narrow(want, CHANNELS[fmt]))
        for slot, fmt in enumerate(OUT_FORMATS, 1):       # and is still there after the pool was rebuilt for the later slots
            _same("%s %dx%d -> format %d, after the rebuilds" % (name, w, h, fmt), ctx.texture_read(slot, w, h, fmt), B.narrow(want, CHANNELS[fmt]))


def test_a_4096_square_bc1(built_lib):
    rng = np.random.default_rng(50)
    blocks = B.random_blocks(rng, "BC1", 4096, 4096)
    ctx = api.Context(0)
    _same("BC1 4096x4096", _expand(ctx, 1, "BC1", blocks, 4096, 4096, api.TEX_RGBA8_UNORM), B.reference_decode("BC1", blocks, 4096, 4096))


@pytest.mark.parametrize("fmt", [api.TEX_R8_UNORM, api.TEX_RG8_UNORM, api.TEX_RGBA8_UNORM])
def test_neighbouring_slots_stay_intact(built_lib, fmt):
    """uncompressed, a 7 x 9 block texture with partial blocks on both edges and an unaligned row pitch, uncompressed: a store past a
    partial block or an unaligned row would land in a neighbour, whichever side of it the pool puts the block texture on."""
    rng = np.random.default_rng(60 + fmt)
    ctx = api.Context(0)
    before = rng.integers(0, 256, (5, 3), dtype=np.uint8)
    after = rng.integers(0, 256, (3, 7, 4), dtype=np.uint8)
    name = {api.TEX_R8_UNORM: "BC4U", api.TEX_RG8_UNORM: "BC5S", api.TEX_RGBA8_UNORM: "BC7"}[fmt]
    blocks = B.random_blocks(rng, name, 7, 9)
    ctx.texture_set(1, before, api.TEX_R8_UNORM)
    ctx.texture_set_bc(2, blocks, 7, 9, B.FORMATS[name][0], fmt)
    ctx.texture_set(3, after, api.TEX_RGBA8_SRGB)
    _same("the block texture", ctx.texture_read(2, 7, 9, fmt), B.narrow(B.reference_decode(name, blocks, 7, 9), CHANNELS[fmt]))
    _same("slot before", ctx.texture_read(1, 3, 5, api.TEX_R8_UNORM), before[:, :, None])
    _same("slot after", ctx.texture_read(3, 7, 3, api.TEX_RGBA8_SRGB), after)
    # a second block texture right behind the first: its region starts where the first one's padding ends
    ctx.texture_set_bc(4, blocks, 7, 9, B.FORMATS[name][0], fmt)
    _same("first block texture", ctx.texture_read(2, 7, 9, fmt), B.narrow(B.reference_decode(name, blocks, 7, 9), CHANNELS[fmt]))
    _same("second block texture", ctx.texture_read(4, 7, 9, fmt), B.narrow(B.reference_decode(name, blocks, 7, 9), CHANNELS[fmt]))
    _same("slot before", ctx.texture_read(1, 3, 5, api.TEX_R8_UNORM), before[:, :, None])


@pytest.mark.parametrize("name,fmt", [("BC7", api.TEX_RGBA8_SRGB), ("BC3", api.TEX_RGBA8_UNORM), ("BC4S", api.TEX_R8_UNORM), ("BC5U", api.TEX_RG8_UNORM)])
def test_sampling_a_block_texture_equals_sampling_its_texels(built_lib, name, fmt):
    import torch
    rng = np.random.default_rng(70 + fmt)
    a, b = api.Context(0), api.Context(0)
    for slot, (w, h) in enumerate([(7, 9), (64, 32), (1, 1)], 1):
        blocks = B.random_blocks(rng, name, w, h)
        a.texture_set_bc(slot, blocks, w, h, B.FORMATS[name][0], fmt)
        texels = B.narrow(B.reference_decode(name, blocks, w, h), CHANNELS[fmt])
        b.texture_set(slot, texels[:, :, 0] if fmt == api.TEX_R8_UNORM else texels, fmt)
    for slot, (w, h) in enumerate([(7, 9), (64, 32), (1, 1)], 1):
        uv = np.concatenate([rng.random((20000, 2)) * 8 - 4, rng.integers(-8, 9, (1000, 2)) / np.array([w, h]),
                             (rng.integers(-8, 9, (1000, 2)) + 0.5) / np.array([w, h])]).astype(np.float32)
        d_uv = torch.from_numpy(uv).cuda()
        out_a = torch.zeros((len(uv), 4), dtype=torch.float32, device="cuda")
        out_b = torch.zeros((len(uv), 4), dtype=torch.float32, device="cuda")
        for gather in (False, True):
            a.texture_sample(slot, d_uv.data_ptr(), len(uv), out_a.data_ptr(), gather)
            b.texture_sample(slot, d_uv.data_ptr(), len(uv), out_b.data_ptr(), gather)
            torch.cuda.synchronize()
            util.assert_same_bits("%s as format %d, %dx%d, gather=%s" % (name, fmt, w, h, gather), out_a.cpu().numpy(), out_b.cpu().numpy())
            assert np.isfinite(out_a.cpu().numpy()).all()


def test_refusals_leave_the_slot_as_it_was(built_lib):
    rng = np.random.default_rng(80)
    ctx = api.Context(0)
    L = ctx.L
    blocks = B.random_blocks(rng, "BC3", 8, 8)
    ctx.texture_set_bc(1, blocks, 8, 8, api.BC3, api.TEX_RGBA8_UNORM)
    plain = rng.integers(0, 256, (4, 4, 4), dtype=np.uint8)
    ctx.texture_set(2, plain, api.TEX_RGBA8_SRGB)
    want = B.reference_decode("BC3", blocks, 8, 8)
    _same("before", ctx.texture_read(1, 8, 8, api.TEX_RGBA8_UNORM), want)
    C = api.C
    big = np.zeros(16 * 4097, np.uint8)

    def call(slot, w, h, bc, ptr, fmt):
        return L.gfx_texture_set_bc(ctx.h, C.c_uint32(slot), C.c_uint32(w), C.c_uint32(h), C.c_uint32(bc), ptr, C.c_uint32(fmt))
    p = blocks.ctypes.data_as(C.c_void_p)
    for args, word in (((1, 8, 8, api.BC3, None, api.TEX_RGBA8_UNORM), "null blocks"),
                       ((1, 0, 8, api.BC3, p, api.TEX_RGBA8_UNORM), "bad size"),
                       ((1, 8, 0, api.BC3, p, api.TEX_RGBA8_UNORM), "bad size"),
                       ((1, 16388, 4, api.BC3, big.ctypes.data_as(C.c_void_p), api.TEX_RGBA8_UNORM), "bad size"),
                       ((1, 8, 8, 8, p, api.TEX_RGBA8_UNORM), "unknown block-compressed format"),
                       ((1, 8, 8, api.BC3, p, api.TEX_RGBA32F), "GFX_TEX_RGBA32F"),
                       ((1, 8, 8, api.BC3, p, 17), "unknown format"),
                       ((0, 8, 8, api.BC3, p, api.TEX_RGBA8_UNORM), "1-based"),
                       ((2, 8, 8, api.BC3, None, api.TEX_RGBA8_UNORM), "null blocks")):
        assert call(*args) == 1
        assert word in L.gfx_last_error(ctx.h).decode(), (args, L.gfx_last_error(ctx.h).decode())
    _same("slot 1 after the refusals", ctx.texture_read(1, 8, 8, api.TEX_RGBA8_UNORM), want)
    _same("slot 2 after the refusals", ctx.texture_read(2, 4, 4, api.TEX_RGBA8_SRGB), plain)
    # gfx_texture_read: a slot never set, a buffer of another size
    out = np.zeros(8 * 8 * 4, np.uint8)
    assert L.gfx_texture_read(ctx.h, None, C.c_uint32(3), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes)) == 1
    assert L.gfx_texture_read(ctx.h, None, C.c_uint32(1), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes - 1)) == 1
    # replacing, by either call: blocks -> texels -> blocks of another format and size
    ctx.texture_set(1, plain, api.TEX_RGBA8_UNORM)
    _same("texels over blocks", ctx.texture_read(1, 4, 4, api.TEX_RGBA8_UNORM), plain)
    b5 = B.random_blocks(rng, "BC5U", 5, 3)
    ctx.texture_set_bc(1, b5, 5, 3, api.BC5_UNORM, api.TEX_RG8_UNORM)
    _same("blocks over texels", ctx.texture_read(1, 5, 3, api.TEX_RG8_UNORM), B.narrow(B.reference_decode("BC5U", b5, 5, 3), 2))
    ctx.texture_set_bc(2, blocks, 8, 8, api.BC2, api.TEX_RGBA8_SRGB)
    _same("blocks over texels, slot 2", ctx.texture_read(2, 8, 8, api.TEX_RGBA8_SRGB), B.reference_decode("BC2", blocks, 8, 8))


# ---------------------------------------------------------------- a rendered scene whose maps are .dds
ROOM_OBJ = ("mtllib room.mtl\n"
            "v -6 0 -6\nv 6 0 -6\nv 6 0 6\nv -6 0 6\nv -6 5 -6\nv 6 5 -6\n"
            "vt 0 0\nvt 4 0\nvt 4 4\nvt 0 4\nvn 0 1 0\nvn 0 0 1\n"
            "usemtl floor\nf 1/1/1 4/4/1 3/3/1 2/2/1\n"
            "usemtl wall\nf 1/1/2 2/2/2 6/3/2 5/4/2\n")
ROOM_MTL = ("newmtl floor\nKd 0.6 0.6 0.6\nKs 0.05 0.05 0.05\nNs 30\nmap_Kd albedo.dds\nmap_Ks specular.dds\nmap_bump normal.dds\n"
            "newmtl wall\nKd 0.7 0.3 0.2\nKs 0.2 0.2 0.2\nNs 80\nmap_bump height.dds\n")


def _smooth_alpha_blocks(rng, n, centre, spread):
    """BC4-style 8-byte blocks whose endpoints stay near `centre`: a bump map that perturbs the normal instead of scrambling it."""
    b = rng.integers(0, 256, (n, 8), dtype=np.uint8)
    b[:, 0] = centre + rng.integers(0, spread, n)
    b[:, 1] = centre - rng.integers(0, spread, n)
    return b


def _write_room(tmp, rng):
    w = h = 16
    n = B.num_blocks(w, h)
    files = {"albedo.dds": B.make_dds("BC7", w, h, B.bc7_constructed_blocks(rng, 1)[rng.permutation(8 * 256)[:n]].tobytes(), srgb=True),
             "specular.dds": B.make_dds("BC1", w, h, B.random_blocks(rng, "BC1", w, h).tobytes()),
             "normal.dds": B.make_dds("BC5U", w, h, np.concatenate([_smooth_alpha_blocks(rng, n, 128, 30), _smooth_alpha_blocks(rng, n, 128, 30)], 1).tobytes()),
             "height.dds": B.make_dds("BC4U", w, h, _smooth_alpha_blocks(rng, n, 128, 100).tobytes())}
    for fn, data in files.items():
        with open(os.path.join(tmp, fn), "wb") as f:
            f.write(data)
    with open(os.path.join(tmp, "room.mtl"), "w") as f:
        f.write(ROOM_MTL)
    with open(os.path.join(tmp, "room.obj"), "w") as f:
        f.write(ROOM_OBJ)
    return os.path.join(tmp, "room.obj")


class _DecodedTextures:
    """A HostScene as the oracle is to see it: block textures replaced by the texels tools/dds_convert.py decodes them to (the oracle
    knows nothing of blocks); everything else is the scene itself."""

    def __init__(self, scene):
        self._scene = scene

    def __getattr__(self, name):
        return getattr(self._scene, name)

    def textures(self):
        names = {v[0]: k for k, v in B.FORMATS.items()}
        out = []
        for t in self._scene.textures():
            if t[4] is None:
                slot, w, h, fmt, _, bc, blocks = t
                texels = B.narrow(B.reference_decode(names[bc], blocks.reshape(-1, B.FORMATS[names[bc]][1]), w, h), CHANNELS[fmt])
                t = (slot, w, h, fmt, texels.reshape(-1))
            out.append(t)
        return out


def _room_scene(obj):
    s = api.HostScene()
    room = s.load_obj(obj)
    panel = s.add_rectangle(2.0, 2.0, (40, 40, 40))
    s.add_instance(room, api.make_transform())
    s.add_instance(panel, api.make_transform(pos=(0.0, 4.5, 0.0)))
    return s


def test_a_scene_with_dds_maps_renders_like_its_decoded_texels(built_lib, tmp_path):
    from tests.test_gpu_restir import run_sequence_both
    obj = _write_room(str(tmp_path), np.random.default_rng(90))
    s = _room_scene(obj)
    fm = {t[0]: (t[3], t[5]) for t in s.textures()}
    floor, wall = [m for m in s.materials() if m.texNormal][:2]
    assert fm[floor.texA] == (api.TEX_RGBA8_SRGB, api.BC7) and fm[floor.texB] == (api.TEX_RGBA8_UNORM, api.BC1)
    assert floor.bumpMapType == api.BUMP_NORMAL_MAP_2CH and fm[floor.texNormal] == (api.TEX_RG8_UNORM, api.BC5_UNORM)
    assert wall.bumpMapType == api.BUMP_HEIGHT_MAP and fm[wall.texNormal] == (api.TEX_R8_UNORM, api.BC4_UNORM)
    cam = api.make_camera(128, 80, pos=(0.0, 2.5, 9.0), yaw=180.0)
    with util.frame_overrides(enableBumpMapping=1):
        diffs = run_sequence_both(_DecodedTextures(s), 128, 80, frames=2, camera=cam)
    assert not diffs, "\n".join(diffs[:12])
    beauty = run_sequence_both.last_beauty
    assert np.isfinite(beauty).all() and beauty[:, :3].mean() > 1e-3


def test_the_command_line_takes_dds_maps(built_lib, tmp_path):
    """-obj with .dds maps and -rect-emitter-tex x.dds through restir_di_headless equal the same scene through the bindings."""
    import torch
    from tests.test_headless_cli import _read_pfm, _run
    rng = np.random.default_rng(91)
    obj = _write_room(str(tmp_path), rng)
    glow = str(tmp_path / "glow.dds")
    with open(glow, "wb") as f:
        f.write(B.make_dds("BC3", 8, 8, B.random_blocks(rng, "BC3", 8, 8).tobytes()))
    W, H, frames = 128, 96, 3
    out = str(tmp_path / "room.pfm")
    d = _run(["-cam-pos", 0, 2.5, 9, "-cam-yaw", 180, "-name", "room", "-obj", obj, 1.0, "trad",
              "-name", "panel", "-emittance", 40, 40, 40, "-rect-emitter-tex", glow, "-rectangle", 2.0, 2.0,
              "-inst", "room", "-begin-pos", 0, 4.5, 0, "-inst", "panel",
              "-size", W, H, "-frames", frames, "-bump", "-out", out])
    assert d["textures"] == 5
    lib = api.lib()
    h2 = api.HostScene()                                             # "panel" sorts before "room"
    g_panel = lib.gfxh_scene_add_rectangle_textured(h2.h, api.C.c_float(2.0), api.C.c_float(2.0), (api.C.c_float * 3)(40, 40, 40), glow.encode())
    g_room = h2.load_obj(obj)
    h2.add_instance(g_room, api.make_transform())
    h2.add_instance(g_panel, api.make_transform(pos=(0.0, 4.5, 0.0)))
    assert all(t[4] is None for t in h2.textures()) and len(h2.textures()) == 5
    ctx = api.Context(0)
    h2.upload(ctx)
    cfg = api.RestirRenderer.default_config(W, H, api.RENDERER_BIASED)
    cam = api.make_camera(W, H, (0.0, 2.5, 9.0))
    for k in range(9):
        cam.orientation[k] = d["camera_orientation"][k]
    cfg.camera = cam
    cfg.enableBumpMapping = 1
    r = api.RestirRenderer(ctx, cfg)
    for _ in range(frames):
        r.render_frame()
    torch.cuda.synchronize()
    want = ctx.read_device(r.beauty_ptr(), W * H * 16).view(np.float32).reshape(H, W, 4)
    assert np.abs(want[..., :3]).sum() > 0
    assert np.array_equal(_read_pfm(out).view(np.uint32), np.ascontiguousarray(want[..., :3]).view(np.uint32))


def test_block_slots_survive_a_second_scene_upload(built_lib, tmp_path):
    obj = _write_room(str(tmp_path), np.random.default_rng(92))
    s = _room_scene(obj)
    ctx = api.Context(0)
    s.upload(ctx)
    ctx.accel_build()
    decoded = {t[0]: t for t in _DecodedTextures(s).textures()}
    first = {slot: ctx.texture_read(slot, t[1], t[2], t[3]) for slot, t in decoded.items()}
    for slot, t in decoded.items():
        _same("slot %d" % slot, first[slot], t[4].reshape(t[2], t[1], -1))
    # a new instance makes the scene dirty: the next upload rebuilds the whole texel pool
    v = np.zeros(3, api.VERTEX_DTYPE)
    v["position"] = [(0, 1, 0), (1, 1, 0), (0, 2, 0)]
    v["normal"] = (0, 0, 1)
    v["texCoord0Dir"] = (1, 0, 0)
    C, L = api.C, ctx.L
    tri = np.array([[0, 1, 2]], np.uint32)
    geom, group, inst = C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert L.gfx_geom_create(ctx.h, v.ctypes.data_as(C.c_void_p), C.c_uint32(v.dtype.itemsize), C.c_uint32(3), tri.ctypes.data_as(C.c_void_p), C.c_uint32(1),
                             C.c_uint32(0), C.byref(geom)) == 0
    assert L.gfx_group_create(ctx.h, C.byref(geom), C.c_uint32(1), C.byref(group)) == 0
    xfm = np.ascontiguousarray(api.make_transform(), np.float32).reshape(12)
    assert L.gfx_instance_create(ctx.h, group, xfm.ctypes.data_as(C.c_void_p), C.byref(inst)) == 0
    ctx.texture_set(len(decoded) + 1, np.full((2, 2, 4), 7, np.uint8), api.TEX_RGBA8_UNORM)      # and the pool's layout changes
    ctx.accel_build()
    for slot, t in decoded.items():
        _same("slot %d after the second upload" % slot, ctx.texture_read(slot, t[1], t[2], t[3]), first[slot])
