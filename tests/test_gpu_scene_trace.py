"""-m gpu: gfx_trace_scene, plain and displaced instances in one ray query, through the C ABI.

The expected result of every case is the chain the call replaces, bit for bit and in every field: gfx_trace on the BVH8, then
the existing gfx_tfdm_trace per instance in index order on rays the HOST to_object_ray made (tests/scene_trace_host.cpp, the
host compilation of csrc/tfdm/tfdm_instance.hip.h), with tmax the best distance so far; normals through the host
normal_to_world; the merge in numpy (tests/scene_trace_host.py).  Geometry independent of the core is held on the host side
(tests/test_scene_trace_cpu.py), where the same header runs."""
import numpy as np
import pytest

from gfxexp_amd import api
from tests import scene_trace_host as S
from tests import tfdm_host as T
from tests import util

pytestmark = pytest.mark.gpu
INVALID = api.GFX_INVALID_SLOT


@pytest.fixture(scope="module")
def host(built_lib, tmp_path_factory):
    return T.Host(tmp_path_factory.mktemp("tfdm_host"))


@pytest.fixture(scope="module")
def shost(built_lib, tmp_path_factory):
    return S.SceneHost(tmp_path_factory.mktemp("scene_host"))


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def gpu_tfdm_trace(tf, mode, org, dirs):
    import torch
    n = len(org)
    d_org = torch.from_numpy(np.ascontiguousarray(org, np.float32)).cuda()
    d_dir = torch.from_numpy(np.ascontiguousarray(dirs, np.float32)).cuda()
    d_out = torch.zeros(n if mode == api.TRACE_ANY else n * 8, dtype=torch.int32, device="cuda")
    tf.trace(mode, d_org.data_ptr(), d_dir.data_ptr(), n, d_out.data_ptr(), 0, stream=_stream())
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    return out.view(np.uint32) if mode == api.TRACE_ANY else out.view(api.TFDM_HIT_DTYPE).reshape(n)


def gpu_scene_trace(ctx, accel, tset, mode, org, dirs, counters=False):
    import torch
    n = len(org)
    d_org = torch.from_numpy(np.ascontiguousarray(org, np.float32)).cuda()
    d_dir = torch.from_numpy(np.ascontiguousarray(dirs, np.float32)).cuda()
    # the output starts as garbage: every entry must be written
    d_out = torch.full((n if mode == api.TRACE_ANY else n * 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    api.trace_scene(ctx, accel, tset, mode, d_org.data_ptr(), d_dir.data_ptr(), n, d_out.data_ptr(), d_cnt.data_ptr() if counters else 0, stream=_stream())
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    res = out.view(np.uint32) if mode == api.TRACE_ANY else out.view(api.SCENE_HIT_DTYPE).reshape(n)
    return (res, d_cnt.cpu().numpy().astype(np.uint64)) if counters else res


def host_records(host, shost, tset, members):
    """The table of `tset` as the host's make_instance derives it: members = [(Tfdm, gp, objToWorld, userId)].  The device
    pointers are taken from the table itself; everything else is made on the host."""
    table = tset.read()
    recs = []
    for k, (tf, gp, m, uid) in enumerate(members):
        ptrs = [int(table[k][f]) for f in ("nodes", "records", "heights", "pyramid")]
        assert all(ptrs)
        recs.append(shost.make_instance(m, tf.read_nodes()[0], ptrs, host.params(gp, tf.size), uid))
    return table, np.concatenate(recs) if recs else np.zeros(0, api.TFDM_INSTANCE_DTYPE)


def chain(ctx, accel, shost, recs, members, mode, org, dirs):
    if mode == api.TRACE_ANY:
        plain = util.gpu_trace(ctx, accel, mode, org, dirs) if accel else None
        steps = [(lambda o, d, r=recs[k:k + 1]: shost.to_object_rays(r, o, d), lambda oo, od, tf=members[k][0]: gpu_tfdm_trace(tf, api.TRACE_ANY, oo, od))
                 for k in range(len(members))]
        return S.chain_any(plain, steps, org, dirs)
    plain = util.gpu_trace(ctx, accel, mode, org, dirs) if accel else None
    steps = [(lambda o, d, r=recs[k:k + 1]: shost.to_object_rays(r, o, d), lambda oo, od, tf=members[k][0]: gpu_tfdm_trace(tf, api.TRACE_CLOSEST, oo, od),
              lambda n, r=recs[k:k + 1]: shost.normals_to_world(r, n)) for k in range(len(members))]
    return S.chain_closest(plain, steps, org, dirs)


def assert_same_hits(what, got, want):
    for f in api.SCENE_HIT_DTYPE.names:
        util.assert_same_bits("%s: field %s" % (what, f), got[f], want[f])


class MixedScene:
    """The plain bunny in the BVH8 and the three displaced instances of tests/scene_trace_host.py, on one context."""

    def __init__(self):
        self.ctx = api.Context(0)
        S.plain_bunny_scene().upload(self.ctx)
        self.accel = self.ctx.accel_build()
        self.objects = [(api.Tfdm(self.ctx, v, t, h, gp), gp) for v, t, h, gp in S.chain_objects()]
        self.members = [(self.objects[o][0], self.objects[o][1], m, 100 + k) for k, (o, m) in enumerate(S.chain_instances())]
        self.set = self.new_set()

    def new_set(self, members=None):
        s = api.TfdmSet(self.ctx)
        for k, (tf, _, m, uid) in enumerate(self.members if members is None else members):
            assert s.add(tf, m, uid) == k
        s.commit()
        return s


@pytest.fixture(scope="module")
def mixed(built_lib):
    return MixedScene()


@pytest.fixture(scope="module")
def mixed_rays(mixed):
    t = mixed.set.read()
    return S.chain_rays([(t[k]["boxLo"].astype(np.float64), t[k]["boxHi"].astype(np.float64)) for k in range(len(t))])


def test_table_equals_the_host_make_instance(mixed, host, shost):
    table, recs = host_records(host, shost, mixed.set, mixed.members)
    util.assert_same_bits("InstanceRecord table", table, recs)
    assert list(table["userId"]) == [100, 101, 102]


@pytest.mark.parametrize("mode", [api.TRACE_CLOSEST, api.TRACE_ANY])
def test_one_call_equals_the_chain(mixed, mixed_rays, host, shost, mode):
    org, dirs = mixed_rays
    _, recs = host_records(host, shost, mixed.set, mixed.members)
    want = chain(mixed.ctx, mixed.accel, shost, recs, mixed.members, mode, org, dirs)
    got = gpu_scene_trace(mixed.ctx, mixed.accel, mixed.set, mode, org, dirs)
    if mode == api.TRACE_ANY:
        assert np.array_equal(got, want) and np.all(got <= 1) and 0.3 < got.mean() < 0.9
        return
    assert_same_hits("mixed scene", got, want)
    where = got["where"]
    shares = [np.mean(where == api.SCENE_PLAIN)] + [np.mean((where >> 1 == k) & (where < api.SCENE_PLAIN)) for k in range(3)]
    print("closest hits: plain %.1f %%, instances %s %%, miss %.1f %%" % (100 * shares[0], ["%.1f" % (100 * s) for s in shares[1:]], 100 * np.mean(where == INVALID)))
    assert all(s > 0.02 for s in shares), "every part of the scene is hit: %s" % shares
    # the rays made to miss every world box do, the rest of a miss is as the header says
    assert np.all(where[-537:] == INVALID)
    miss = where == INVALID
    assert np.all(got["dist"][miss] == dirs[miss, 3]) and np.all(got["index"][miss] == INVALID) and np.all(got["bcB"][miss] == 0) and np.all(got["normal"][miss] == 0)
    disp = ~miss & (where != api.SCENE_PLAIN)
    assert np.all(np.abs(np.linalg.norm(got["normal"][disp].astype(np.float64), axis=1) - 1) < 1e-5)
    assert set(np.unique(where[disp] & 1)) == {0, 1}


def test_degenerate_forms(mixed, mixed_rays, host, shost):
    org, dirs = mixed_rays
    ctx = mixed.ctx
    # no set, and an empty set: gfx_trace
    empty = api.TfdmSet(ctx)
    empty.commit()
    for mode in (api.TRACE_CLOSEST, api.TRACE_ANY):
        plain = util.gpu_trace(ctx, mixed.accel, mode, org, dirs)
        for tset in (None, empty):
            got = gpu_scene_trace(ctx, mixed.accel, tset, mode, org, dirs)
            if mode == api.TRACE_ANY:
                assert np.array_equal(got, plain)
            else:
                assert_same_hits("no instances", got, S.chain_closest(plain, [], org, dirs))
                hit = plain["triIndex"] != INVALID
                assert np.all(got["where"][hit] == api.SCENE_PLAIN) and np.array_equal(got["index"], plain["triIndex"]) and 0.05 < hit.mean() < 0.9
    # no accel: the instances alone
    _, recs = host_records(host, shost, mixed.set, mixed.members)
    for mode in (api.TRACE_CLOSEST, api.TRACE_ANY):
        want = chain(ctx, 0, shost, recs, mixed.members, mode, org, dirs)
        got = gpu_scene_trace(ctx, 0, mixed.set, mode, org, dirs)
        if mode == api.TRACE_ANY:
            assert np.array_equal(got, want)
        else:
            assert_same_hits("instances alone", got, want)
            assert not np.any(got["where"] == api.SCENE_PLAIN)
    # nothing at all: every ray misses
    got = gpu_scene_trace(ctx, 0, None, api.TRACE_CLOSEST, org, dirs)
    assert np.all(got["where"] == INVALID) and np.all(got["dist"] == dirs[:, 3])
    assert not gpu_scene_trace(ctx, 0, None, api.TRACE_ANY, org, dirs).any()
    # the same object twice under one transform: the lower index on every hit
    tf, gp, m, uid = mixed.members[1]
    twice = mixed.new_set([(tf, gp, m, 1), (tf, gp, m, 2)])
    once = mixed.new_set([(tf, gp, m, 1)])
    a, b = gpu_scene_trace(ctx, 0, twice, api.TRACE_CLOSEST, org, dirs), gpu_scene_trace(ctx, 0, once, api.TRACE_CLOSEST, org, dirs)
    assert_same_hits("twice the same instance", a, b)
    hit = a["where"] != INVALID
    assert hit.mean() > 0.1 and np.all(a["where"][hit] >> 1 == 0)
    for s in (empty, twice, once):
        s.close()


def _grid_scene(ctx):
    v, t = T.quad_mesh()
    gp = api.tfdm_params(h_scale=0.15)
    rng = np.random.default_rng(9)
    tf = api.Tfdm(ctx, v, t, rng.uniform(0, 1, (16, 16)).astype(np.float32), gp)
    members = []
    for j in range(7):
        for i in range(10):
            lin = S.rotation((0.2, 0.1, 1.0), 10.0 * (i - j)) @ np.diag([0.9, 0.9, 1.0 + 0.1 * j])
            members.append((tf, gp, S.affine(lin, (1.1 * i, 1.1 * j, 0.02 * i)), 7 * i + j))
    tset = api.TfdmSet(ctx)
    for tf_, _, m, uid in members:
        tset.add(tf_, m, uid)
    tset.commit()
    cam = T.look_at_camera(97, 65, (5.5, -6.0, 7.0), (5.5, 3.6, 0.0), fov_y_deg=50.0)
    org, dirs = api.camera_rays(cam, 97, 65)
    assert len(org) % 64 != 0
    return tf, members, tset, org, dirs


def test_more_instances_than_a_wave_is_wide(mixed, host, shost):
    ctx = mixed.ctx
    tf, members, tset, org, dirs = _grid_scene(ctx)
    assert len(tset) == 70
    table, recs = host_records(host, shost, tset, members)
    util.assert_same_bits("InstanceRecord table of the grid", table, recs)
    got, cnt = gpu_scene_trace(ctx, mixed.accel, tset, api.TRACE_CLOSEST, org, dirs, counters=True)
    assert_same_hits("10 x 7 grid", got, chain(ctx, mixed.accel, shost, recs, members, api.TRACE_CLOSEST, org, dirs))
    inst = got["where"][(got["where"] != INVALID) & (got["where"] != api.SCENE_PLAIN)] >> 1
    assert len(np.unique(inst)) == 70 and inst.max() == 69, "every instance of the grid is seen by some ray"
    occ = gpu_scene_trace(ctx, mixed.accel, tset, api.TRACE_ANY, org, dirs)
    assert np.array_equal(occ, chain(ctx, mixed.accel, shost, recs, members, api.TRACE_ANY, org, dirs))
    assert np.array_equal(occ == 1, got["where"] != INVALID)
    # counters: rays, world-box tests, traversals -- the cull does its work on a grid
    print("grid: counters %s" % cnt)
    assert cnt[2] == len(org) and cnt[5] <= cnt[4] <= len(org) * 70 and cnt[5] < cnt[4] and cnt[5] > 0
    assert cnt[4] == len(org) * 70            # a closest-hit lane tests every world box
    assert np.all(cnt[6:] == 0)
    tset.close()
    tf.close()


def test_counters_on_the_mixed_scene(mixed, mixed_rays):
    org, dirs = mixed_rays
    for mode in (api.TRACE_CLOSEST, api.TRACE_ANY):
        _, cnt = gpu_scene_trace(mixed.ctx, mixed.accel, mixed.set, mode, org, dirs, counters=True)
        print("mode %d: counters %s" % (mode, cnt))
        assert cnt[2] == len(org) and cnt[5] <= cnt[4] <= len(org) * 3 and cnt[3] >= cnt[5] > 0 and cnt[0] > 0 and cnt[1] > 0
    # they are added to, not overwritten
    import torch
    d_org, d_dir = torch.from_numpy(org).cuda(), torch.from_numpy(dirs).cuda()
    d_out = torch.zeros(len(org) * 8, dtype=torch.int32, device="cuda")
    d_cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    for _ in range(2):
        api.trace_scene(mixed.ctx, mixed.accel, mixed.set, api.TRACE_CLOSEST, d_org.data_ptr(), d_dir.data_ptr(), len(org), d_out.data_ptr(), d_cnt.data_ptr(), stream=_stream())
    torch.cuda.synchronize()
    assert d_cnt.cpu().numpy()[2] == 2 * len(org)


def test_recommit_equals_a_fresh_set(mixed, mixed_rays, host, shost):
    org, dirs = mixed_rays
    ctx = mixed.ctx
    moved = list(mixed.members)
    tf, gp, _, uid = moved[1]
    moved[1] = (tf, gp, S.affine(S.rotation((1.0, 0.2, 0.1), -25.0) @ np.diag([1.2, 1.2, 0.8]), (0.3, 0.1, 0.5)), uid)
    fresh = mixed.new_set(moved)
    again = mixed.new_set()
    before = gpu_scene_trace(ctx, mixed.accel, again, api.TRACE_CLOSEST, org, dirs)
    again.set_transform(1, moved[1][2])
    again.commit()
    util.assert_same_bits("table after set_transform + commit", again.read(), fresh.read())
    table, recs = host_records(host, shost, again, moved)
    util.assert_same_bits("table against the host make_instance", table, recs)
    a, b = gpu_scene_trace(ctx, mixed.accel, again, api.TRACE_CLOSEST, org, dirs), gpu_scene_trace(ctx, mixed.accel, fresh, api.TRACE_CLOSEST, org, dirs)
    assert_same_hits("recommitted set", a, b)
    assert not np.array_equal(a["dist"], before["dist"]), "the moved instance changes the picture"
    # a transform that is refused at commit leaves the committed table in force
    again.set_transform(1, np.zeros(12, np.float32))
    with pytest.raises(api.GfxError, match="singular"):
        again.commit()
    with pytest.raises(api.GfxError, match="not committed"):
        gpu_scene_trace(ctx, mixed.accel, again, api.TRACE_CLOSEST, org[:64], dirs[:64])
    again.set_transform(1, moved[1][2])
    again.commit()
    assert_same_hits("after the repaired transform", gpu_scene_trace(ctx, mixed.accel, again, api.TRACE_CLOSEST, org, dirs), b)
    fresh.close()
    again.close()


def test_refusals_carry_a_text(mixed, mixed_rays):
    import torch
    org, dirs = mixed_rays
    org, dirs = np.ascontiguousarray(org[::19][:1000]), np.ascontiguousarray(dirs[::19][:1000])      # a sample across the picture and the specials
    ctx = mixed.ctx
    v, t = T.quad_mesh()
    tf = api.Tfdm(ctx, v, t, T.two_sine_map(16), api.tfdm_params(h_scale=0.1))
    ident = S.affine(np.eye(3), (0, 0, 0))
    s = api.TfdmSet(ctx)
    s.add(tf, ident)
    # an add that is not committed; a transform that is not committed
    with pytest.raises(api.GfxError, match="not committed"):
        gpu_scene_trace(ctx, mixed.accel, s, api.TRACE_CLOSEST, org, dirs)
    with pytest.raises(api.GfxError, match="not committed"):
        s.read()
    s.commit()
    want = gpu_scene_trace(ctx, mixed.accel, s, api.TRACE_CLOSEST, org, dirs)
    assert np.mean((want["where"] != INVALID) & (want["where"] != api.SCENE_PLAIN)) > 0.05
    s.set_transform(0, ident)
    with pytest.raises(api.GfxError, match="not committed"):
        gpu_scene_trace(ctx, mixed.accel, s, api.TRACE_ANY, org, dirs)
    s.commit()
    # set_params on a member after the commit: the records hold the old buffers
    tf.set_params(api.tfdm_params(h_scale=0.2))
    with pytest.raises(api.GfxError, match="gfx_tfdm_set_params"):
        gpu_scene_trace(ctx, mixed.accel, s, api.TRACE_CLOSEST, org, dirs)
    s.commit()
    changed = gpu_scene_trace(ctx, mixed.accel, s, api.TRACE_CLOSEST, org, dirs)
    assert not np.array_equal(changed["dist"], want["dist"])
    tf.set_params(api.tfdm_params(h_scale=0.1))
    s.commit()
    assert_same_hits("after the parameters came back", gpu_scene_trace(ctx, mixed.accel, s, api.TRACE_CLOSEST, org, dirs), want)
    # misaligned buffers are refused before anything is launched
    for args in [(api.TRACE_CLOSEST, 256 + 4, 256, 1, 256), (api.TRACE_CLOSEST, 256, 256 + 8, 1, 256), (api.TRACE_CLOSEST, 256, 256, 1, 256 + 4),
                 (api.TRACE_ANY, 256, 256, 1, 256 + 2)]:
        with pytest.raises(api.GfxError, match="aligned"):
            api.trace_scene(ctx, mixed.accel, s, *args)
    with pytest.raises(api.GfxError, match="8-byte"):
        api.trace_scene(ctx, mixed.accel, s, api.TRACE_ANY, 256, 256, 1, 256 + 4, d_counters=256 + 4)
    with pytest.raises(api.GfxError, match="mode"):
        api.trace_scene(ctx, mixed.accel, s, 5, 256, 256, 1, 256)
    with pytest.raises(api.GfxError, match="accel"):
        api.trace_scene(ctx, 77, s, api.TRACE_ANY, 256, 256, 1, 256)
    with pytest.raises(api.GfxError, match="no such instance"):
        s.set_transform(3, ident)
    # more than 1024 instances
    big = api.TfdmSet(ctx)
    for k in range(api.TFDM_SET_MAX_INSTANCES):
        big.add(tf, S.affine(np.eye(3), (k, 0, 0)), k)
    with pytest.raises(api.GfxError, match="1024"):
        big.add(tf, ident)
    big.commit()
    assert len(big.read()) == 1024 and big.read()["userId"][1023] == 1023
    # a foreign device: an object or a set of another device's context (needs a second device to exist)
    print("devices: %d" % torch.cuda.device_count())
    if torch.cuda.device_count() > 1:
        other = api.Context(1)
        foreign = api.Tfdm(other, v, t, T.two_sine_map(16), api.tfdm_params(h_scale=0.1))
        with pytest.raises(api.GfxError, match="another device"):
            s.add(foreign, ident)
        fs = api.TfdmSet(other)
        fs.add(foreign, ident)
        fs.commit()
        with pytest.raises(api.GfxError, match="another device"):
            api.trace_scene(ctx, mixed.accel, fs, api.TRACE_ANY, 256, 256, 1, 256)
        with pytest.raises(api.GfxError, match="another device"):
            ctx._check(ctx.L.gfx_tfdm_set_commit(ctx.h, None, fs.h))
        fs.close()
        foreign.close()
    else:
        with pytest.raises(api.GfxError, match="no such HIP device"):
            api.Context(1)
    # the context and the set are alive and well afterwards
    assert_same_hits("after the refusals", gpu_scene_trace(ctx, mixed.accel, s, api.TRACE_CLOSEST, org, dirs), want)
    for x in (big, s):
        x.close()
    tf.close()
