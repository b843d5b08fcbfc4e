"""-m gpu: NRTDSM objects as members of a gfx_tfdm_set beside TFDM ones, traced by gfx_trace_scene (k_scene_instances_mixed),
through the C ABI.

The scene: the plain bunny in the BVH8 and a set of four members (tests/scene_nrtdsm_host.py): TFDM quad, NRTDSM cap (rotated,
scaled (1.5, 0.75, 2)), TFDM bunny base (mirrored), NRTDSM quad (mirrored); maps of 64 x 64 and 32 x 32; the 21 237 rays of
S.chain_rays over the members' world boxes.

Expected results, all bit for bit and in every field:
  * the chain the call replaces: gfx_trace, then per member in index order gfx_tfdm_trace or gfx_nrtdsm_trace on rays the HOST
    to_object_ray made, tmax the best so far, normals through the host normal_to_world, merged by S.chain_closest / S.chain_any;
  * the host walk of csrc/nrtdsm/nrtdsm_instance.hip.h (tests/scene_nrtdsm_host.cpp) over host copies of the objects.
Geometry independent of the core is held on the host side (tests/test_scene_nrtdsm_cpu.py), where the same header runs."""
import numpy as np
import pytest

from gfxexp_amd import api
from tests import nrtdsm_host as NH
from tests import scene_nrtdsm_host as M
from tests import scene_trace_host as S
from tests import tfdm_host as T
from tests import util
from tests.test_gpu_scene_trace import assert_same_hits, gpu_scene_trace, gpu_tfdm_trace

pytestmark = pytest.mark.gpu
INVALID = api.GFX_INVALID_SLOT
MODES = [api.TRACE_CLOSEST, api.TRACE_ANY]


@pytest.fixture(scope="module")
def nhost(built_lib, tmp_path_factory):
    return NH.Host(tmp_path_factory.mktemp("nrtdsm_host"))


@pytest.fixture(scope="module")
def shost(built_lib, tmp_path_factory):
    return S.SceneHost(tmp_path_factory.mktemp("scene_host"))


@pytest.fixture(scope="module")
def mhost(built_lib, tmp_path_factory):
    return M.MixedHost(tmp_path_factory.mktemp("scene_nrtdsm_host"))


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


class MixedKinds:
    """The plain bunny in the BVH8 (and one ungrouped quad geometry to bind a TFDM-only set to) and the four members on one context.
    members: [(kind, object, gp, objToWorld, userId)]."""

    def __init__(self):
        self.ctx = api.Context(0)
        hs = S.plain_bunny_scene()
        qv, qt = T.quad_mesh()
        self.quad_slot = hs.add_geom(qv, qt, hs.add_material_traditional((0.5, 0.5, 0.5), (0, 0, 0), 0.3))      # in no group: not in the BVH8
        hs.upload(self.ctx)
        self.accel = self.ctx.accel_build()
        self.inputs = M.mixed_objects()
        self.objects = [(api.Nrtdsm if k == M.NRTDSM else api.Tfdm)(self.ctx, v, t, h, gp) for k, v, t, h, gp in self.inputs]
        self.members = [(self.inputs[o][0], self.objects[o], self.inputs[o][4], m, 100 + k) for k, (o, m) in enumerate(M.mixed_instances())]
        self.set = self.new_set()

    def new_set(self, members=None):
        s = api.TfdmSet(self.ctx)
        for k, (_, obj, _, m, uid) in enumerate(self.members if members is None else members):
            assert s.add(obj, m, uid) == k
        s.commit()
        return s


@pytest.fixture(scope="module")
def mixed(built_lib):
    return MixedKinds()


@pytest.fixture(scope="module")
def rays(mixed):
    t = mixed.set.read()
    return S.chain_rays([(t[k]["boxLo"].astype(np.float64), t[k]["boxHi"].astype(np.float64)) for k in range(len(t))])


def host_records(nhost, mhost, tset, members):
    """The table of `tset` as the host's make_instance derives it, with the device pointers taken from the table itself."""
    table = tset.read()
    recs = []
    for k, (kind, obj, gp, m, uid) in enumerate(members):
        ptrs = [int(table[k][f]) for f in ("nodes", "records", "heights", "pyramid")]
        assert all(ptrs)
        recs.append(mhost.make_instance(kind, m, obj.read_nodes()[0], ptrs, nhost.T.params(gp, obj.size), uid))
    return table, np.concatenate(recs)


def chain(ctx, accel, shost, recs, members, mode, org, dirs):
    plain = util.gpu_trace(ctx, accel, mode, org, dirs) if accel else None
    to_object = [lambda o, d, r=recs[k:k + 1]: shost.to_object_rays(r, o, d) for k in range(len(members))]
    trace = [lambda oo, od, obj=members[k][1]: gpu_tfdm_trace(obj, mode, oo, od) for k in range(len(members))]       # gfx_tfdm_trace or gfx_nrtdsm_trace
    if mode == api.TRACE_ANY:
        return S.chain_any(plain, list(zip(to_object, trace)), org, dirs)
    to_world = [lambda n, r=recs[k:k + 1]: shost.normals_to_world(r, n) for k in range(len(members))]
    return S.chain_closest(plain, list(zip(to_object, trace, to_world)), org, dirs)


def shares_of(where, members):
    return [np.mean(where == api.SCENE_PLAIN)] + [np.mean((where >> 1 == k) & (where < api.SCENE_PLAIN)) for k in range(members)] + [np.mean(where == INVALID)]


# ---------------------------------------------------------------- the table
def test_table_equals_the_host_make_instance(mixed, nhost, mhost):
    table, recs = host_records(nhost, mhost, mixed.set, mixed.members)
    util.assert_same_bits("InstanceRecord table", table, recs)
    assert list(table["pad0"]) == [M.TFDM, M.NRTDSM, M.TFDM, M.NRTDSM] and list(table["userId"]) == [100, 101, 102, 103]
    # a TFDM member's record is the one a set of only that member gives: every byte it had before there were kinds
    for k in (0, 2):
        alone = mixed.new_set([mixed.members[k]])
        util.assert_same_bits("the record of TFDM member %d" % k, table[k:k + 1], alone.read())
        alone.close()


def test_transform_move_and_the_motion_table_work_for_an_nrtdsm_member(mixed, rays):
    """They depend only on transforms: the motion table of a set whose moved member is NRTDSM equals, bit for bit, that of a set with a
    TFDM object in its place; the moved set traces as a set freshly built at the new transform."""
    org, dirs = rays
    org, dirs = np.ascontiguousarray(org[::7]), np.ascontiguousarray(dirs[::7])
    ctx = mixed.ctx
    quad, cap = mixed.members[0], mixed.members[1]
    to = S.affine(S.rotation((1.0, 0.2, 0.1), -25.0) @ np.diag([1.2, 1.2, 0.8]), (0.3, 0.1, -0.5))
    a, b = mixed.new_set([quad, cap]), mixed.new_set([quad, (quad[0], quad[1], quad[2], cap[3], cap[4])])
    for s in (a, b):
        s.move(1, to)
        s.commit()
    util.assert_same_bits("motion table after a move", a.read_motion(), b.read_motion())
    assert not np.array_equal(a.read_motion()["curToPrev"][1], a.read_motion()["curToPrev"][0])
    fresh = mixed.new_set([quad, (cap[0], cap[1], cap[2], to, cap[4])])
    util.assert_same_bits("table after the move", a.read(), fresh.read())
    assert_same_hits("moved set", gpu_scene_trace(ctx, mixed.accel, a, api.TRACE_CLOSEST, org, dirs), gpu_scene_trace(ctx, mixed.accel, fresh, api.TRACE_CLOSEST, org, dirs))
    a.set_transform(1, cap[3])          # the teleport: back where it was, no motion
    a.commit()
    assert np.array_equal(a.read_motion()["curToPrev"][1], a.read_motion()["curToPrev"][0])
    util.assert_same_bits("table after the teleport", a.read()[1:2], mixed.set.read()[1:2])
    for s in (a, b, fresh):
        s.close()


# ---------------------------------------------------------------- one call = the chain = the host walk
@pytest.mark.parametrize("mode", MODES)
def test_one_call_equals_the_chain(mixed, rays, nhost, shost, mhost, mode):
    org, dirs = rays
    _, recs = host_records(nhost, mhost, mixed.set, mixed.members)
    want = chain(mixed.ctx, mixed.accel, shost, recs, mixed.members, mode, org, dirs)
    got = gpu_scene_trace(mixed.ctx, mixed.accel, mixed.set, mode, org, dirs)
    if mode == api.TRACE_ANY:
        assert np.array_equal(got, want) and np.all(got <= 1) and 0.3 < got.mean() < 0.9
        return
    assert_same_hits("mixed kinds", got, want)
    where = got["where"]
    shares = shares_of(where, 4)
    print("closest hits: plain %.1f %%, members %s %%, miss %.1f %%" % (100 * shares[0], ["%.1f" % (100 * s) for s in shares[1:5]], 100 * shares[5]))
    assert all(s > 0.02 for s in shares), "every part of the scene (plain, each member, miss) gets some rays: %s" % shares
    assert np.all(where[-537:] == INVALID)
    miss = where == INVALID
    assert np.all(got["dist"][miss] == dirs[miss, 3]) and np.all(got["index"][miss] == INVALID) and np.all(got["bcB"][miss] == 0) and np.all(got["normal"][miss] == 0)
    disp = ~miss & (where != api.SCENE_PLAIN)
    assert np.all(np.abs(np.linalg.norm(got["normal"][disp].astype(np.float64), axis=1) - 1) < 1e-5)
    for k in range(4):
        assert set(np.unique(where[disp & (where >> 1 == k)] & 1)) == {0, 1}, "member %d is seen from both sides" % k


@pytest.mark.parametrize("mode", MODES)
def test_device_equals_the_host_walk(mixed, rays, nhost, mhost, mode):
    org, dirs = rays
    states = [(nhost if k == M.NRTDSM else nhost.T).state(v, t, h, gp) for k, v, t, h, gp in mixed.inputs]
    table = np.concatenate([mhost.instance_of_state(mixed.inputs[o][0], states[o], m, 100 + k) for k, (o, m) in enumerate(M.mixed_instances())])
    plain = util.gpu_trace(mixed.ctx, mixed.accel, mode, org, dirs)
    want, hc = mhost.trace(table, plain, mode, org, dirs, counters=True)
    got, dc = gpu_scene_trace(mixed.ctx, mixed.accel, mixed.set, mode, org, dirs, counters=True)
    if mode == api.TRACE_ANY:
        assert np.array_equal(got, want)
    else:
        assert_same_hits("device against the host walk", got, want)
    print("mode %d: counters device %s, host %s" % (mode, dc[:6], hc[:6]))
    assert np.array_equal(dc[:6], hc[:6]), "the per-ray counters of the device are the host walk's"


# ---------------------------------------------------------------- degenerate forms
def test_degenerate_forms(mixed, rays, nhost, shost, mhost):
    import torch
    org, dirs = rays
    ctx = mixed.ctx
    # NRTDSM members only, with and without the BVH8
    only = [mixed.members[1], mixed.members[3]]
    nset = mixed.new_set(only)
    table, recs = host_records(nhost, mhost, nset, only)
    util.assert_same_bits("table of the NRTDSM-only set", table, recs)
    for accel in (mixed.accel, 0):
        for mode in MODES:
            want = chain(ctx, accel, shost, recs, only, mode, org, dirs)
            got = gpu_scene_trace(ctx, accel, nset, mode, org, dirs)
            if mode == api.TRACE_ANY:
                assert np.array_equal(got, want)
            else:
                assert_same_hits("NRTDSM members only, accel %d" % accel, got, want)
                assert (accel != 0) == bool(np.any(got["where"] == api.SCENE_PLAIN)) and all(np.mean(got["where"] >> 1 == k) > 0.02 for k in (0, 1))
    # no accel, all four members
    _, recs4 = host_records(nhost, mhost, mixed.set, mixed.members)
    for mode in MODES:
        want = chain(ctx, 0, shost, recs4, mixed.members, mode, org, dirs)
        got = gpu_scene_trace(ctx, 0, mixed.set, mode, org, dirs)
        if mode == api.TRACE_ANY:
            assert np.array_equal(got, want)
        else:
            assert_same_hits("members alone", got, want)
    # the same NRTDSM object twice under one transform: the lower index on every hit, and the answer of the set that has it once
    twice, once = mixed.new_set([mixed.members[1], mixed.members[1]]), mixed.new_set([mixed.members[1]])
    a, b = gpu_scene_trace(ctx, 0, twice, api.TRACE_CLOSEST, org, dirs), gpu_scene_trace(ctx, 0, once, api.TRACE_CLOSEST, org, dirs)
    assert_same_hits("twice the same NRTDSM instance", a, b)
    hit = a["where"] != INVALID
    assert hit.mean() > 0.05 and np.all(a["where"][hit] >> 1 == 0)
    # zero rays: nothing is launched, nothing is written
    d_out = torch.full((64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    for mode in MODES:
        api.trace_scene(ctx, mixed.accel, mixed.set, mode, 0, 0, 0, d_out.data_ptr(), stream=_stream())
    torch.cuda.synchronize()
    assert np.all(d_out.cpu().numpy() == 0x5A5A5A5A)
    # ray counts that are no multiple of 64 (the whole set: 21 237), and the garbage gpu_scene_trace fills the output with is gone
    assert len(org) % 64 != 0
    for n in (1, 63, 65):
        got = gpu_scene_trace(ctx, mixed.accel, mixed.set, api.TRACE_CLOSEST, org[4000:4000 + n], dirs[4000:4000 + n])
        assert_same_hits("%d rays" % n, got, gpu_scene_trace(ctx, mixed.accel, mixed.set, api.TRACE_CLOSEST, org, dirs)[4000:4000 + n])
    full = gpu_scene_trace(ctx, mixed.accel, mixed.set, api.TRACE_CLOSEST, org, dirs)
    assert not np.any(full.view(np.uint32).reshape(-1, 8) == 0x5A5A5A5A)
    for s in (nset, twice, once):
        s.close()


# ---------------------------------------------------------------- staleness and recommit
def test_stale_member_is_refused_and_recommit_equals_a_fresh_set(mixed, rays):
    org, dirs = rays
    org, dirs = np.ascontiguousarray(org[::7]), np.ascontiguousarray(dirs[::7])
    ctx = mixed.ctx
    kind, v, t, h, gp = mixed.inputs[3]
    obj = api.Nrtdsm(ctx, v, t, h, gp)
    members = list(mixed.members)
    members[3] = (kind, obj, gp, members[3][3], members[3][4])
    s = mixed.new_set(members)
    before = gpu_scene_trace(ctx, mixed.accel, s, api.TRACE_CLOSEST, org, dirs)
    assert_same_hits("a second object of the same inputs", before, gpu_scene_trace(ctx, mixed.accel, mixed.set, api.TRACE_CLOSEST, org, dirs))
    obj.set_params(api.tfdm_params(h_scale=0.15))
    for mode in MODES:
        with pytest.raises(api.GfxError, match="gfx_nrtdsm_set_params"):
            gpu_scene_trace(ctx, mixed.accel, s, mode, org, dirs)
    s.commit()
    fresh = mixed.new_set(members)
    util.assert_same_bits("table after the recommit", s.read(), fresh.read())
    a, b = gpu_scene_trace(ctx, mixed.accel, s, api.TRACE_CLOSEST, org, dirs), gpu_scene_trace(ctx, mixed.accel, fresh, api.TRACE_CLOSEST, org, dirs)
    assert_same_hits("recommitted set", a, b)
    assert not np.array_equal(a["dist"], before["dist"]), "the new parameters change the picture"
    # a stale TFDM member of the same set keeps its own message
    mixed.objects[0].set_params(mixed.inputs[0][4])
    with pytest.raises(api.GfxError, match="gfx_tfdm_set_params"):
        gpu_scene_trace(ctx, mixed.accel, s, api.TRACE_CLOSEST, org, dirs)
    mixed.set.commit()
    for x in (s, fresh):
        x.close()
    obj.close()


# ---------------------------------------------------------------- what is refused
def test_a_set_with_an_nrtdsm_member_is_traced_but_not_rendered(mixed, rays):
    org, dirs = rays
    org, dirs = np.ascontiguousarray(org[::7]), np.ascontiguousarray(dirs[::7])
    ctx = mixed.ctx
    want = gpu_scene_trace(ctx, mixed.accel, mixed.set, api.TRACE_CLOSEST, org, dirs)
    for restir in (False, True):
        with pytest.raises(api.GfxError, match="traced .* but not rendered"):
            ctx.bind_displaced(mixed.set, [mixed.quad_slot] * 4, restir=restir)
    # a TFDM-only set still binds, with and without the ReSTIR passes; a null object and a 1025th member are refused as for gfx_tfdm_set_add
    tonly = mixed.new_set([mixed.members[0]])
    for restir in (False, True):
        ctx.bind_displaced(tonly, [mixed.quad_slot], restir=restir)
        ctx.bind_displaced(None)
    index = api.C.c_uint32()
    ident = np.ascontiguousarray(S.affine(np.eye(3), (0, 0, 0)).reshape(-1))
    with pytest.raises(api.GfxError, match="null object"):
        ctx._check(ctx.L.gfx_tfdm_set_add_nrtdsm(tonly.h, None, ident.ctypes.data_as(api.C.c_void_p), api.C.c_uint32(0), api.C.byref(index)))
    big = api.TfdmSet(ctx)
    for k in range(api.TFDM_SET_MAX_INSTANCES):
        assert big.add(mixed.objects[k & 1], S.affine(np.eye(3), (k, 0, 0)), k) == k         # both kinds, one index sequence
    with pytest.raises(api.GfxError, match="1024"):
        big.add(mixed.objects[1], ident)
    # nothing was launched and the context goes on working
    assert_same_hits("after the refusals", gpu_scene_trace(ctx, mixed.accel, mixed.set, api.TRACE_CLOSEST, org, dirs), want)
    for x in (tonly, big):
        x.close()


# ---------------------------------------------------------------- counters
def test_counters(mixed, rays):
    import torch
    org, dirs = rays
    ctx = mixed.ctx
    for mode in MODES:
        _, cnt = gpu_scene_trace(ctx, mixed.accel, mixed.set, mode, org, dirs, counters=True)
        print("mode %d: counters %s" % (mode, cnt))
        assert cnt[2] == len(org) and 0 < cnt[5] <= cnt[4] <= len(org) * 4 and cnt[3] >= cnt[5] and cnt[0] > 0 and cnt[1] > 0 and np.all(cnt[6:] == 0)
    # NRTDSM only, no accel, the identity: [0..3] are gfx_nrtdsm_trace's own counters on the same rays
    obj = mixed.objects[1]
    s = api.TfdmSet(ctx)
    s.add(obj, S.affine(np.eye(3), (0, 0, 0)))
    s.commit()
    o, d = T.mesh_rays(mixed.inputs[1][1], 5000, 5)
    d_org, d_dir = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    for mode in MODES:
        d_out = torch.zeros(len(o) * 8, dtype=torch.int32, device="cuda")
        d_cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
        obj.trace(mode, d_org.data_ptr(), d_dir.data_ptr(), len(o), d_out.data_ptr(), d_cnt.data_ptr(), stream=_stream())
        torch.cuda.synchronize()
        own = d_cnt.cpu().numpy().astype(np.uint64)
        _, cnt = gpu_scene_trace(ctx, 0, s, mode, o, d, counters=True)
        print("mode %d: gfx_nrtdsm_trace %s, the scene query %s" % (mode, own, cnt))
        assert np.array_equal(cnt[:4], own) and own[3] > 0 and cnt[5] <= cnt[4] <= len(o)
    s.close()
