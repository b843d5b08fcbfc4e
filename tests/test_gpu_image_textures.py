"""-m gpu: PNG / JPEG textures end to end.  The decoders run on the host (tests/test_image_codecs_cpu.py pins them to the reference's
decoder); here the decoded files go through gfxh_scene_upload / gfx_texture_set into the device pool and are read back, sampled and
rendered: the pool holds the golden bytes, the sampler and a ReSTIR DI sequence on the textured bunny see a PNG / JPEG map exactly as
they see its golden texels (the oracle is handed the golden texels, never the files), and the command line takes an OBJ whose MTL
names .png / .jpg maps and writes a .png that decodes to the pixels of its .bmp."""
import os
import shutil

import numpy as np
import pytest

from gfxexp_amd import api, scenes
from tests import image_fixtures as F
from tests import util

pytestmark = pytest.mark.gpu
CHANNELS = {api.TEX_RGBA8_SRGB: 4, api.TEX_RGBA8_UNORM: 4, api.TEX_RG8_UNORM: 2, api.TEX_R8_UNORM: 1}
BUNNY = os.path.join(util.ASSETS, "stanford_bunny_309_faces.obj")
# map_Kd, map_Ks, map_bump, map_Ke of the bunny's material
BUNNY_MAPS = [("map_Kd", "rgba8.png"), ("map_Ks", "base420.jpg"), ("map_bump", "adam7_rgb8.png"), ("map_Ke", "prog444.jpg")]


def _same(tag, got, want):
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bad = np.argwhere((got != want).reshape(got.shape[0], got.shape[1], -1).any(-1))
    assert len(bad) == 0, "%s: %d texels differ, first at (y, x) = %s: %s, golden %s" % (tag, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def test_uploaded_slots_hold_the_golden_bytes(built_lib, tmp_path):
    """every valid fixture as one slot of one scene, in the four 8-bit formats by turns: after the upload the pool holds the
    reference decoder's bytes"""
    names = F.valid_names()
    formats = [api.TEX_RGBA8_SRGB, api.TEX_RGBA8_UNORM, api.TEX_R8_UNORM, api.TEX_RG8_UNORM]
    s = api.HostScene()
    slots = []
    for k, name in enumerate(names):
        fmt = formats[k % 4]
        slots.append((s.load_texture(F.write_file(tmp_path, name), fmt), name, fmt))
    s.add_instance(s.add_rectangle(1.0, 1.0, (1, 1, 1)), api.make_transform())
    ctx = api.Context(0)
    s.upload(ctx)
    for slot, name, fmt in slots:
        want = F.golden(name)[0]
        _same("%s as format %d" % (name, fmt), ctx.texture_read(slot, want.shape[1], want.shape[0], fmt), want[..., :CHANNELS[fmt]])


@pytest.mark.parametrize("name,fmt", [("rgba8.png", api.TEX_RGBA8_SRGB), ("adam7_rgba16.png", api.TEX_RGBA8_UNORM), ("base422.jpg", api.TEX_RGBA8_SRGB),
                                      ("prog420.jpg", api.TEX_RG8_UNORM), ("grey_prog.jpg", api.TEX_R8_UNORM)])
def test_sampling_a_decoded_file_equals_sampling_its_golden_texels(built_lib, tmp_path, name, fmt):
    import torch
    rng = np.random.default_rng(len(name) + fmt)
    want = F.golden(name)[0]
    h, w = want.shape[:2]
    s = api.HostScene()
    slot = s.load_texture(F.write_file(tmp_path, name), fmt)
    s.add_instance(s.add_rectangle(1.0, 1.0, (1, 1, 1)), api.make_transform())
    a, b = api.Context(0), api.Context(0)
    s.upload(a)
    texels = np.ascontiguousarray(want[..., :CHANNELS[fmt]])
    b.texture_set(slot, texels[:, :, 0] if fmt == api.TEX_R8_UNORM else texels, fmt)
    uv = np.concatenate([rng.random((20000, 2)) * 8 - 4, rng.integers(-8, 9, (1000, 2)) / np.array([w, h]),
                         (rng.integers(-8, 9, (1000, 2)) + 0.5) / np.array([w, h])]).astype(np.float32)
    d_uv = torch.from_numpy(uv).cuda()
    out_a = torch.zeros((len(uv), 4), dtype=torch.float32, device="cuda")
    out_b = torch.zeros((len(uv), 4), dtype=torch.float32, device="cuda")
    for gather in (False, True):
        a.texture_sample(slot, d_uv.data_ptr(), len(uv), out_a.data_ptr(), gather)
        b.texture_sample(slot, d_uv.data_ptr(), len(uv), out_b.data_ptr(), gather)
        torch.cuda.synchronize()
        util.assert_same_bits("%s as format %d, gather=%s" % (name, fmt, gather), out_a.cpu().numpy(), out_b.cpu().numpy())
        assert np.isfinite(out_a.cpu().numpy()).all()


def _write_bunny(directory, as_tga):
    """the bunny with four maps on its material: the fixture files under their own extensions, or .tga files of the golden texels"""
    os.makedirs(directory)
    shutil.copy(BUNNY, os.path.join(directory, "stanford_bunny_309_faces.obj"))
    with open(os.path.splitext(BUNNY)[0] + ".mtl") as f:
        mtl = f.read()
    for key, fixture in BUNNY_MAPS:
        if as_tga:
            fn = os.path.splitext(fixture)[0] + ".tga"
            F.write_tga(os.path.join(directory, fn), F.golden(fixture)[0])
        else:
            fn = fixture
            F.write_file(directory, fixture)
        mtl += "%s %s\n" % (key, fn)
    with open(os.path.join(directory, "stanford_bunny_309_faces.mtl"), "w") as f:
        f.write(mtl)
    return os.path.join(directory, "stanford_bunny_309_faces.obj")


class _GoldenTextures:
    """A HostScene as the oracle is to see it: every texture slot replaced by the golden texels of the fixture the material names"""

    def __init__(self, scene, by_slot):
        self._scene, self._by_slot = scene, by_slot

    def __getattr__(self, name):
        return getattr(self._scene, name)

    def textures(self):
        out = []
        for slot, w, h, fmt, _ in self._scene.textures():
            want = F.golden(self._by_slot[slot])[0]
            assert want.shape[:2] == (h, w)
            out.append((slot, w, h, fmt, np.ascontiguousarray(want[..., :CHANNELS[fmt]]).reshape(-1)))
        return out


def test_the_textured_bunny_renders_like_its_golden_texels(built_lib, tmp_path):
    from tests.test_gpu_restir import run_sequence_both
    s = scenes.bunny_scene(_write_bunny(str(tmp_path / "files"), False))
    m = [m for m in s.materials() if m.texA][0]
    assert m.texA and m.texB and m.texNormal and m.texEmittance and m.hasEmittance == 1
    by_slot = {m.texA: "rgba8.png", m.texB: "base420.jpg", m.texNormal: "adam7_rgb8.png", m.texEmittance: "prog444.jpg"}
    assert len(by_slot) == 4 and len(s.textures()) == 4
    with util.frame_overrides(enableBumpMapping=1):
        diffs = run_sequence_both(_GoldenTextures(s, by_slot), 96, 64, frames=2)
    assert not diffs, "\n".join(diffs[:12])
    beauty = run_sequence_both.last_beauty
    assert np.isfinite(beauty).all() and beauty[:, :3].mean() > 1e-3


def _read_bmp(path):
    with open(path, "rb") as f:
        d = f.read()
    assert d[:2] == b"BM"
    off = int.from_bytes(d[10:14], "little")
    w, h = int.from_bytes(d[18:22], "little"), int.from_bytes(d[22:26], "little")
    stride = (3 * w + 3) & ~3
    rows = np.frombuffer(d, np.uint8, stride * h, off).reshape(h, stride)[::-1, :3 * w].reshape(h, w, 3)
    return rows[..., ::-1]


def test_the_command_line_takes_png_and_jpg_maps_and_writes_a_png(built_lib, tmp_path):
    from tests.test_headless_cli import _read_pfm, _run
    W, H, frames = 128, 96, 2

    def args(obj, out):
        return ["-cam-pos", 1.5, 5.0, 14.0, "-cam-yaw", 180, "-name", "a_bunny", "-obj", obj, 0.1, "trad",
                "-name", "b_panel", "-emittance", 40, 40, 40, "-rectangle", 2.0, 2.0,
                "-inst", "a_bunny", "-begin-pos", 0, 12, 2, "-inst", "b_panel", "-size", W, H, "-frames", frames, "-bump", "-out", out]
    files, tga = _write_bunny(str(tmp_path / "files"), False), _write_bunny(str(tmp_path / "tga"), True)
    outs = {k: str(tmp_path / ("f." + k)) for k in ("pfm", "png", "bmp")}
    d = _run(args(files, outs["pfm"]))
    assert d["textures"] == 4
    _run(args(tga, str(tmp_path / "t.pfm")))
    hdr = _read_pfm(outs["pfm"])
    assert np.abs(hdr).sum() > 0
    assert np.array_equal(hdr.view(np.uint32), _read_pfm(str(tmp_path / "t.pfm")).view(np.uint32))
    _run(args(files, outs["png"]))
    _run(args(files, outs["bmp"]))
    with open(outs["png"], "rb") as f:
        data = f.read()
    png = F.read_png_rgba8(data)
    own, n = api.image_decode_rgba8(data)
    assert n == 4 and np.array_equal(own, png) and png.shape == (H, W, 4)
    assert np.array_equal(png[..., :3], _read_bmp(outs["bmp"])) and (png[..., 3] == 255).all()
    assert len(np.unique(png[..., :3])) > 16
    # -env-texture keeps demanding a float image
    r = _run(["-env-texture", F.write_file(tmp_path, "rgb8.png"), "-name", "a_bunny", "-obj", files, 0.1, "trad", "-inst", "a_bunny", "-size", 32, 32, "-frames", 1], check=False)
    assert r.returncode != 0 and "wants a float image" in r.stderr
