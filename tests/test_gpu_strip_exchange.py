"""-m gpu: band renderers in strip-exchange mode (gfxh_restir_set_exchange) reproduce the whole-frame renderer bit for
bit.  Three bands on one GPU, one host thread each, exchanging through tests/loopback.py: the C++ frame loop, its
exchange descriptors and the band-limited kernels are the production code; only the transport differs from the RCCL
callbacks (whose descriptor handling the world-2 gloo tests cover: tests/test_tilesplit_gloo.py)."""
import os

import numpy as np
import pytest

from gfxexp_amd import api, tilesplit
from tests import util

W, H, FRAMES, WORLD, MOTION_ROWS = 128, 96, 3, 3, 10

CASES = [("biased", api.RENDERER_BIASED, False), ("unbiased_moving", api.RENDERER_UNBIASED, True),
         ("rearch_biased_moving", api.RENDERER_REARCH_BIASED, True), ("rearch_unbiased", api.RENDERER_REARCH_UNBIASED, False),
         ("regir", api.RENDERER_PATH_TRACE_REGIR, False), ("path_trace", api.RENDERER_PATH_TRACE, False)]


def _camera(frame, moving):
    dy = 0.6 * frame if moving else 0.0
    return api.make_camera(W, H, pos=(1.5 + 0.5 * dy, 5.0 + dy, 14.0), pitch=12.0, yaw=186.0)


def _make(hs, renderer, band):
    ctx = api.Context(0)           # one context per band: launch parameters are per-context state
    hs.upload(ctx)
    cfg = api.RestirRenderer.default_config(W, H, renderer)
    cfg.camera = _camera(0, False)
    cfg.spatialNeighborRadius = 6.0
    cfg.enableAccumulation = 0
    cfg.maxPathLength = 4
    cfg.rowBegin, cfg.rowEnd = band
    if renderer == api.RENDERER_PATH_TRACE_REGIR:
        b = hs.bounds()
        for k in range(3):
            cfg.regirAabbMin[k] = float(b[k]); cfg.regirAabbMax[k] = float(b[3 + k]); cfg.regirGridDimension[k] = (8, 4, 8)[k]
    return ctx, api.RestirRenderer(ctx, cfg)


def _read(ctx, r):
    import torch
    torch.cuda.synchronize()
    s, _, last, _, _ = r.params()
    n = W * H
    return {"beauty": ctx.read_device(r.beauty_ptr(), n * 16).view(np.float32).reshape(H, W, 4),
            "res": ctx.read_device(s.reservoirBuffer[last], n * 48).view(np.float32).reshape(3, H, W, 4),
            "info": ctx.read_device(s.reservoirInfoBuffer[last], n * 8).view(np.float32).reshape(H, W, 2),
            "rng": ctx.read_device(s.rngBuffer, n * 8).view(np.uint64).reshape(H, W), "last": last}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_three_band_strip_exchange_matches_whole_frame(built_lib, case):
    from tests import loopback
    name, renderer, moving = case
    hs = util.bunny_scene()
    full_ctx, full = _make(hs, renderer, (0, 0))
    for frame in range(FRAMES):
        if moving:
            full.set_camera(_camera(frame, True))
        full.render_frame()
    want = _read(full_ctx, full)
    assert np.abs(want["beauty"][..., :3]).sum() > 0

    bands = tilesplit.band_rows(H, WORLD)
    assert bands == [(0, 32), (32, 64), (64, 96)]
    made = [_make(hs, renderer, b) for b in bands]
    ex = loopback.LoopbackExchange(WORLD)
    for rank, (_, r) in enumerate(made):
        r.set_exchange(ex.callback(rank), MOTION_ROWS if moving else 0)

    def before(frame, rank, r):
        if moving:
            r.set_camera(_camera(frame, True))
    loopback.run_bands([r for _, r in made], FRAMES, before)
    for rank, ((ctx, r), (b, e)) in enumerate(zip(made, bands)):
        got = _read(ctx, r)
        assert got["last"] == want["last"]
        util.assert_same_bits(f"{name}: band {rank} gathered HDR frame", got["beauty"], want["beauty"])
        util.assert_same_bits(f"{name}: band {rank} final reservoirs", got["res"][:, b:e], want["res"][:, b:e])
        util.assert_same_bits(f"{name}: band {rank} final reservoir infos", got["info"][b:e], want["info"][b:e])
        util.assert_same_bits(f"{name}: band {rank} pixel RNGs", got["rng"][b:e], want["rng"][b:e])
        assert len(ex.calls[rank]) == len(ex.calls[0]) > 0


@pytest.mark.gpu
def test_band_renderer_refuses_motion_it_cannot_exchange(built_lib):
    """A band renderer told the scene is static (maxMotionRows = 0) fails loudly when the camera moves instead of
    dropping temporal reuse along the seams."""
    hs = util.bunny_scene()
    ctx, r = _make(hs, api.RENDERER_BIASED, (32, 64))
    r.set_exchange(lambda stream, d: None, 0)
    r.render_frame()
    r.set_camera(_camera(1, True))
    with pytest.raises(api.GfxError, match="moved"):
        r.render_frame()
    # the refusal changed nothing: with motion rows installed the same frame renders (frame index 1, not 2)
    r.set_exchange(lambda stream, d: None, 8)
    r.render_frame()
    assert r.params()[4] == 2
    # a camera set before the first frame is not "motion" (frame 0 reads no previous frame), nor is it with temporal reuse off
    ctx2, r2 = _make(hs, api.RENDERER_BIASED, (32, 64))
    r2.set_exchange(lambda stream, d: None, 0)
    r2.set_camera(_camera(1, True))
    r2.render_frame()


@pytest.mark.gpu
def test_rccl_exchange_single_rank(built_lib):
    """gfxh_rccl_exchange (the C++ callback over RCCL) with a communicator of one rank: create, all-reduce, band gather and
    an (empty) strip exchange run on the stream and leave the single band's data untouched."""
    import ctypes as C
    import torch
    L = api.lib()
    L.gfxh_rccl_last_error.restype = C.c_char_p
    ident = (C.c_uint8 * 128)()
    assert L.gfxh_rccl_unique_id(ident) == 0, L.gfxh_rccl_last_error()
    comm = C.c_void_p()
    assert L.gfxh_rccl_create(ident, 0, 1, C.c_uint32(H), C.byref(comm)) == 0, L.gfxh_rccl_last_error()
    try:
        counters = torch.arange(64, dtype=torch.int32, device="cuda")
        frame = torch.rand(H * W * 4, device="cuda")
        keep = frame.clone()
        d = api.GfxhExchangeDesc()
        d.kind, d.width, d.height, d.bandBegin, d.bandEnd = api.EXCHANGE_ALLREDUCE_SUM_U32, W, H, 0, H
        d.counters, d.numCounters = counters.data_ptr(), 64
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert L.gfxh_rccl_exchange(comm, stream, C.byref(d)) == 0, L.gfxh_rccl_last_error()
        d.kind, d.numBuffers = api.EXCHANGE_GATHER_BANDS, 1
        d.buffers[0].base, d.buffers[0].bytesPerPixel, d.buffers[0].numPlanes, d.buffers[0].planeStride = frame.data_ptr(), 16, 1, 16 * W * H
        assert L.gfxh_rccl_exchange(comm, stream, C.byref(d)) == 0, L.gfxh_rccl_last_error()
        d.kind = api.EXCHANGE_STRIPS
        assert L.gfxh_rccl_exchange(comm, stream, C.byref(d)) == 0, L.gfxh_rccl_last_error()
        # the NRC kinds: record gather (one rank: the records stay, the host count is the total) and broadcast from rank 0
        records = torch.rand(1000 * 14, device="cuda")
        keep_records = records.clone()
        host_counts = (C.c_uint32 * 2)(600, 0)
        d = api.GfxhExchangeDesc()
        d.kind, d.width, d.height, d.numBuffers = api.EXCHANGE_GATHER_RECORDS, W, H, 1
        d.buffers[0].base, d.buffers[0].bytesPerPixel, d.buffers[0].numPlanes = records.data_ptr(), 56, 1
        d.counters, d.numCounters = C.addressof(host_counts), 1000
        assert L.gfxh_rccl_exchange(comm, stream, C.byref(d)) == 0, L.gfxh_rccl_last_error()
        assert list(host_counts) == [600, 0]
        host_counts[0] = 2000                                   # more records than the arrays hold: refused
        assert L.gfxh_rccl_exchange(comm, stream, C.byref(d)) == 1
        d = api.GfxhExchangeDesc()
        d.kind, d.numBuffers = api.EXCHANGE_BROADCAST, 1
        d.buffers[0].base, d.buffers[0].bytesPerPixel, d.buffers[0].numPlanes, d.buffers[0].planeStride = records.data_ptr(), 1, 1, records.numel() * 4
        assert L.gfxh_rccl_exchange(comm, stream, C.byref(d)) == 0, L.gfxh_rccl_last_error()
        torch.cuda.synchronize()
        assert torch.equal(counters.cpu(), torch.arange(64, dtype=torch.int32))
        assert torch.equal(frame, keep) and torch.equal(records, keep_records)
    finally:
        L.gfxh_rccl_destroy(comm)


@pytest.mark.gpu
@pytest.mark.parametrize("train_on_rank0", [False, True])
def test_three_band_nrc_renderers(built_lib, monkeypatch, train_on_rank0):
    """NRC band renderers (gfxh_nrc_set_exchange) on one GPU: frame 0 -- initial weights everywhere -- is bit-identical to the
    whole-frame renderer and the gathered record count is the whole frame's; then EVERY rank trains its own copy of the network on
    the gathered batch (the training step is reproducible bit for bit) and all ranks hold the same parameters, Adam moments, EMA
    weights and inference images bit for bit (train_on_rank0: the scheme of rounds 3-4 -- rank 0 trains, its inference images are
    broadcast -- behind GFX_NRC_TRAIN_ON_RANK0=1: the images agree, the other ranks' parameters stay untrained); frame 1 (weights
    trained on the same records in another order than the whole-frame renderer's) agrees with the whole-frame renderer to that
    difference, and every rank gathers the same frame."""
    import ctypes as C
    import torch
    from tests import loopback
    monkeypatch.setenv("GFX_NRC_TRAIN_ON_RANK0", "1" if train_on_rank0 else "0")

    def all_params(ctx, r):
        L = api.lib()
        net = r.network()
        count = C.c_uint32()
        ctx._check(L.gfx_nrc_num_params(ctx.h, C.c_uint64(net), C.byref(count)))
        out = []
        for which in range(4):
            a = np.zeros(count.value, np.float32)
            ctx._check(L.gfx_nrc_get_params(ctx.h, C.c_uint64(net), C.c_int(which), a.ctypes.data_as(C.c_void_p), count))
            out.append(a.view(np.uint32))
        return out
    hs = util.bunny_scene()
    cam = api.make_camera(W, H, pos=(1.5, 5.0, 14.0), pitch=12.0, yaw=186.0)

    def make(band):
        ctx = api.Context(0)
        hs.upload(ctx)
        cfg = api.NrcRenderer.default_config(W, H, hs.bounds())
        cfg.camera = cam
        cfg.maxPathLength = 4
        cfg.rowBegin, cfg.rowEnd = band
        return ctx, api.NrcRenderer(ctx, cfg)

    def beauty(ctx, r):
        torch.cuda.synchronize()
        return ctx.read_device(r.beauty_ptr(), W * H * 16).view(np.float32).reshape(H, W, 4).copy()

    full_ctx, full = make((0, 0))
    full.render_frame()
    want0, stats0 = beauty(full_ctx, full), full.stats()
    full.render_frame()
    want1 = beauty(full_ctx, full)
    assert np.abs(want0[..., :3]).sum() > 0 and stats0["numTrainingData"] > 100

    bands = tilesplit.band_rows(H, WORLD)
    made = [make(b) for b in bands]
    ex = loopback.LoopbackExchange(WORLD)
    for rank, (_, r) in enumerate(made):
        r.set_exchange(ex.callback(rank), rank)
    loopback.run_bands([r for _, r in made], 1)
    images = []
    for rank, (ctx, r) in enumerate(made):
        util.assert_same_bits(f"nrc band {rank} frame 0", beauty(ctx, r), want0)
        assert r.stats()["numTrainingData"] == stats0["numTrainingData"] and r.stats()["tileSize"] == stats0["tileSize"]
        imgs = []
        for which in (0, 1):
            ptr, n = ctx.nrc_inference_image(r.network(), which)
            assert ptr and n
            imgs.append(ctx.read_device(ptr, n).copy())
        images.append(imgs)
    initial = api.Context(0)
    for rank in range(1, WORLD):
        for which in (0, 1):
            assert np.array_equal(images[rank][which], images[0][which]), (rank, which)
    params = [all_params(ctx, r) for ctx, r in made]
    fresh_params = None
    for rank in range(1, WORLD):
        for which, name in enumerate(("parameters", "EMA weights", "Adam m", "Adam v")):
            same = np.array_equal(params[rank][which], params[0][which])
            if not train_on_rank0:
                assert same, f"rank {rank}: {name} differ from rank 0's after the same four training steps"
            elif name == "parameters":
                assert not same, "GFX_NRC_TRAIN_ON_RANK0: only rank 0 trains"
    ctx0, fresh = make((0, 0))           # an untrained network: the broadcast images are NOT the initial ones
    p0, n0 = ctx0.nrc_inference_image(fresh.network(), 1)
    assert not np.array_equal(ctx0.read_device(p0, n0), images[1][1])
    loopback.run_bands([r for _, r in made], 1)
    for rank, (ctx, r) in enumerate(made):
        got1 = beauty(ctx, r)
        err = np.abs(got1[..., :3] - want1[..., :3]).mean() / max(1e-6, np.abs(want1[..., :3]).mean())
        assert err < 0.05, (rank, err)
        assert np.array_equal(got1, beauty(made[0][0], made[0][1]))      # every rank gathered the same frame
    del initial


@pytest.mark.gpu
def test_band_nrc_renderers_notice_a_copy_of_the_network_that_drifted(built_lib, monkeypatch):
    """Every rank of a band-split NRC frame trains its own copy of the network; every 16th frame the ranks compare a checksum of
    the images they infer with (one 8-byte all-reduce, gfx_nrc_params_checksum).  Sixteen frames of two identical copies pass the
    comparison; then one rank's parameters are nudged and the next comparison fails the frame on every rank, by name.  And a
    gradient mode whose sum depends on arrival order (GFX_NRC_GRID_GRAD=f32) makes the band renderers train on rank 0."""
    import ctypes as C
    from tests import loopback
    monkeypatch.setenv("GFX_NRC_TRAIN_ON_RANK0", "0")
    hs = util.bunny_scene()
    w, h = 96, 64
    cam = api.make_camera(w, h, pos=(1.5, 5.0, 14.0), pitch=12.0, yaw=186.0)

    def make(band):
        ctx = api.Context(0)
        hs.upload(ctx)
        cfg = api.NrcRenderer.default_config(w, h, hs.bounds())
        cfg.camera, cfg.maxPathLength = cam, 3
        cfg.rowBegin, cfg.rowEnd = band
        return ctx, api.NrcRenderer(ctx, cfg)
    bands = tilesplit.band_rows(h, 2)
    made = [make(b) for b in bands]
    ex = loopback.LoopbackExchange(2)
    for rank, (_, r) in enumerate(made):
        r.set_exchange(ex.callback(rank), rank)
    loopback.run_bands([r for _, r in made], 16)                       # frame 15 compares: equal copies
    assert sum(1 for calls in ex.calls for kind, _ in calls if kind == api.EXCHANGE_ALLREDUCE_SUM_U32) == 2
    ctx1, r1 = made[1]
    L = api.lib()
    n = C.c_uint32()
    ctx1._check(L.gfx_nrc_num_params(ctx1.h, C.c_uint64(r1.network()), C.byref(n)))
    p = np.zeros(n.value, np.float32)
    ctx1._check(L.gfx_nrc_get_params(ctx1.h, C.c_uint64(r1.network()), C.c_int(0), p.ctypes.data_as(C.c_void_p), n))
    p[:64] += np.float32(0.25)
    ctx1._check(L.gfx_nrc_set_params(ctx1.h, C.c_uint64(r1.network()), p.ctypes.data_as(C.c_void_p), n))
    loopback.run_bands([r for _, r in made], 15)                       # frames 16 .. 30: no comparison yet
    with pytest.raises(AssertionError) as e:
        loopback.run_bands([r for _, r in made], 1)                    # frame 31
    assert "diverged" in str(e.value)
    for _, r in made:
        r.close()
    # an order-dependent gradient sum: the ranks do not each train
    monkeypatch.setenv("GFX_NRC_GRID_GRAD", "f32")
    made = [make(b) for b in bands]
    ex = loopback.LoopbackExchange(2)
    for rank, (_, r) in enumerate(made):
        r.set_exchange(ex.callback(rank), rank)
    loopback.run_bands([r for _, r in made], 1)
    assert any(kind == api.EXCHANGE_BROADCAST for kind, _ in ex.calls[1]), "GFX_NRC_GRID_GRAD=f32: rank 0 trains and broadcasts"


@pytest.mark.gpu
def test_strip_exchange_over_torch_nccl_single_rank(built_lib):
    """The code path bench.py --gpus N installs -- tilesplit.StripExchange over torch.distributed's nccl (= RCCL) backend with
    device-memory views -- on a process group of one rank whose band is the whole frame: the strip exchanges have nothing to
    send, the asynchronous band gather and the ReGIR counter all-reduce run through RCCL, and the frames equal the
    whole-frame renderer's."""
    import socket
    import torch
    import torch.distributed as dist
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        hs = util.bunny_scene()
        for renderer in (api.RENDERER_BIASED, api.RENDERER_PATH_TRACE_REGIR):
            ctx_full, full = _make(hs, renderer, (0, 0))
            ctx_band, band = _make(hs, renderer, (0, H))
            ex = tilesplit.StripExchange(dist, 0, 1, H, tilesplit.device_bytes, device="cuda")
            band.set_exchange(ex, 0)
            stream = torch.cuda.current_stream().cuda_stream
            for _ in range(FRAMES):
                full.render_frame(stream)
                band.render_frame(stream)
            ex.finish()
            want, got = _read(ctx_full, full), _read(ctx_band, band)
            util.assert_same_bits("band = whole frame over RCCL", got["beauty"], want["beauty"])
            util.assert_same_bits("band = whole frame over RCCL, reservoirs", got["res"], want["res"])
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_cpp_rccl_callback_drives_a_band_renderer(built_lib):
    """bench.py --exchange rccl: gfxh_rccl_exchange installed as the C callback (no Python between the passes) on a
    communicator of one rank whose band is the whole frame; frames equal the whole-frame renderer's."""
    import ctypes as C
    import torch
    L = api.lib()
    L.gfxh_rccl_last_error.restype = C.c_char_p
    ident = (C.c_uint8 * 128)()
    assert L.gfxh_rccl_unique_id(ident) == 0, L.gfxh_rccl_last_error()
    comm = C.c_void_p()
    assert L.gfxh_rccl_create(ident, 0, 1, C.c_uint32(H), C.byref(comm)) == 0, L.gfxh_rccl_last_error()
    try:
        hs = util.bunny_scene()
        for renderer in (api.RENDERER_BIASED, api.RENDERER_REARCH_BIASED, api.RENDERER_PATH_TRACE_REGIR):
            ctx_full, full = _make(hs, renderer, (0, 0))
            ctx_band, band = _make(hs, renderer, (0, H))
            L.gfxh_restir_set_exchange(band.h, C.cast(L.gfxh_rccl_exchange, C.c_void_p), comm, C.c_uint32(0))
            for _ in range(FRAMES):
                full.render_frame()
                band.render_frame()
            want, got = _read(ctx_full, full), _read(ctx_band, band)
            util.assert_same_bits("band = whole frame through gfxh_rccl_exchange", got["beauty"], want["beauty"])
    finally:
        torch.cuda.synchronize()
        L.gfxh_rccl_destroy(comm)


@pytest.mark.gpu
def test_plain_bench_run_times_the_steps_alone_and_dumps_the_last_frame(built_lib, tmp_path):
    """`bench.py --gpus 1` without --full: the headline line alone (none of the legs --full adds), exactly --steps timed frames, and
    --dump-outputs writes the frame of the last of them as its caller reads it (the float4 HDR beauty buffer)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    W, H = 320, 192
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--width", str(W), "--height", str(H),
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 2 and d["ms_per_step"] > 0 and d["unit"] == "Mpaths/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert abs(d["value"] - W * H / d["ms_per_step"] / 1e3) < 0.01 * d["value"]
    for key in ("roofline", "kernels_ms_per_frame", "mse", "cpu_baseline", "other_configs", "gpu_bvh_build_ms"):
        assert key not in d, key
    assert os.listdir(tmp_path) == ["beauty.npy"]
    frame = np.load(tmp_path / "beauty.npy")
    assert frame.dtype == np.float32 and frame.shape == (H, W, 4) and np.isfinite(frame).all() and frame[..., :3].max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [[], ["--config", "4"], ["--animate"]])
def test_bench_frame_loop_with_two_ranks_on_one_gpu(built_lib, flags):
    """`bench.py --gpus 2` as the driver launches it (torch.distributed.run, one process per rank), on a one-GPU box: GFX_BENCH_ONE_GPU=1
    puts both ranks on device 0 and stages the collectives through host memory over gloo (tilesplit.HostStaged; RCCL refuses two ranks
    on a device).  Everything else is the multi-GPU path: band partition, the cost-balancing rounds that re-create the band renderers,
    strip exchange between the passes, asynchronous band gather + finish(), barrier / max-over-ranks timing, one JSON line from rank 0."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GFX_BENCH_ONE_GPU="1", MASTER_ADDR="127.0.0.1")
    port = 29600 + (os.getpid() + len(flags) * 7) % 300
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "2", "--full", "--mse-ref-spp", "0", "--cpu-sample", "0"] + flags
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                      # rank 0 prints, rank 1 does not
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["value"] > 0 and d["ms_per_step"] > 0
    assert "row-bands x2" in d["config"]["parallelism"] and d["config"]["bands"] is not None and len(d["config"]["bands"]) == 2
    assert d["config"]["bands"][0][0] == 0 and d["config"]["bands"][0][1] == d["config"]["bands"][1][0] and d["config"]["bands"][1][1] == d["config"]["height"]
    # the default: bands cut by cost (every rank's band timed alone behind a callback that moves nothing, gfxh_balance_bands on the times)
    rounds = d["config"]["band_balancing"]
    assert 1 <= len(rounds) <= 2 and all(len(r["band_ms_alone"]) == 2 and min(r["band_ms_alone"]) > 0 for r in rounds)
    assert rounds[0]["bands"] == [[0, 544], [544, 1080]]
    assert d["gathered_frame_matches_bands"] is True
    if not flags:
        # the headline run also measures BASELINE's configs[4] -- the configuration that IS the split across the node -- on the same ranks
        c4 = d["other_configs"]["configs[4]"]
        assert "error" not in c4, c4
        assert c4["n_gpus"] == 2 and c4["value"] > 0 and "unbiased" in c4["workload"] and c4["gathered_frame_matches_bands"] is True
    else:
        assert "other_configs" not in d


@pytest.mark.gpu
def test_bench_starts_its_own_ranks_and_survives_a_transport_that_hangs(built_lib):
    """`python bench.py --gpus 2` with no launcher around it starts the ranks itself and prints their one line; ranks that do not finish
    (--rank-timeout: every rank reports the stage it is in and exits) get ONE more attempt over the conservative transport, and a run
    whose both attempts fail ends with an exit code and the reason instead of hanging."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GFX_BENCH_ONE_GPU="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    tail = ["--steps", "3", "--warmup", "2", "--full", "--cpu-sample", "0"]
    base = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--mse-ref-spp", "0"] + tail
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--mse-ref-spp", "48"] + tail, capture_output=True, text=True, timeout=900, cwd=root, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["value"] > 0 and "fallback" not in d["config"]
    # the ranks together: rank 0's gathered frame is the ranks' bands, and the MSE against the reference every rank accumulated for its
    # rows is the one-GPU run's (same frames, same per-pixel reference streams; fp64 sums in another order)
    assert d["gathered_frame_matches_bands"] is True
    one = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--mse-ref-spp", "48", "--no-roofline", "--other-configs", "0"] + tail,
                         capture_output=True, text=True, timeout=900, cwd=root, env=env)
    assert one.returncode == 0, one.stderr[-3000:]
    d1 = json.loads([ln for ln in one.stdout.splitlines() if ln.startswith("{")][-1])
    for key in ("mse", "rel_mse", "mse_of_one_reference_frame"):
        assert abs(d["mse"][key] - d1["mse"][key]) <= 1e-9 * abs(d1["mse"][key]), (key, d["mse"][key], d1["mse"][key])
    # a rank that fails AFTER the timed frames (in the gathered-frame check / the MSE leg) costs those legs, not the measurement
    r = subprocess.run(base + ["--other-configs", "0"], capture_output=True, text=True, timeout=900, cwd=root, env=dict(env, GFX_BENCH_TEST_FAIL_RANK="1"))
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["n_gpus"] == 2 and d["value"] > 0 and "error" in d["after_the_timed_frames"] and "mse" not in d
    r = subprocess.run(base + ["--rank-timeout", "0.05"], capture_output=True, text=True, timeout=900, cwd=root, env=env)
    assert r.returncode != 0
    assert "did not finish within" in r.stderr and "one more attempt with --exchange torch --sync-gather" in r.stderr, r.stderr[-3000:]
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


@pytest.mark.gpu
def test_lane_schedules_compute_the_same_frames(built_lib):
    """G-buffer strips on the G-buffer lane, band gather on the gather lane, injected latency: bit-identical to the one-stream schedule
    (tests/lane_schedule_check.py, its own process: it names the mirror librccl stand-in)."""
    import subprocess
    import sys
    from tests.native import build as native_build
    native_build.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "lane_schedule_check.py")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().startswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]
