"""MI355X: batched instanced ray queries (bvh3X_instance_prepare / bvh3X_intersect_rays_instanced, bvh_amd.instance_prepare /
intersect_instanced). The device's hit records, instances, counters and prepared instances are bit-equal to the host harness's (the
same text compiled by g++, tests/test_instanced_host.py) on that file's scenes, with a ragged last block; bit-equal to the composition of
the compiled reference's single-level query on the 12-instance scene; the moving-geometry loop (new matrices -> instance_prepare ->
refit_boxes of the top tree -> trace) against a top tree built afresh; two host threads on two streams; refusals."""
import threading

import numpy as np
import pytest

import instanced_scenes as sc
from instanced_scenes import INVALID, MODES4
from test_instanced_host import expect_single_leaf

pytestmark = pytest.mark.gpu

N_RAYS = 4096 + 37                                            # a ragged last block
ANY_HIT, ROBUST, SORTED, ORIGINAL_IDS, UNSORTED = 1, 2, 4, 8, 16


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return sc.compile_harness(tmp_path_factory.mktemp("instanced_gpu"))


def _cuda(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


class DeviceScene:
    """A Scene of instanced_scenes on the device: its geometries and its top tree through from_nodes, the arrays in HBM."""

    def __init__(self, scene, top=True):
        import bvh_amd
        self.scene = scene
        self.geoms = [(bvh_amd.Bvh.from_nodes(g.nodes, g.ids), _cuda(g.tris12)) for g in scene.geoms]
        self.obj2world = _cuda(scene.obj2world)
        self.gids = None if scene.gids is None else _cuda(scene.gids)
        self.world2obj = _cuda(scene.world2obj)
        self.top = bvh_amd.Bvh.from_nodes(scene.top_nodes, scene.top_ids) if top else None

    def trace(self, rays, any_hit, robust, original_ids=False, top=None, world2obj=None):
        import bvh_amd
        hits, inst, cnt = bvh_amd.intersect_instanced(top or self.top, self.geoms, self.world2obj if world2obj is None else world2obj, rays, self.gids,
                                                      any_hit=any_hit, robust=robust, counters=True, original_ids=original_ids)
        return bvh_amd.hits_to_numpy(hits), inst.cpu().numpy().view(np.uint32), cnt.cpu().numpy().astype(np.uint64)


def same_as_host(dev, scene, rays, any_hit, robust, original_ids=False, deep_cap=0):
    want, want_inst, want_cnt = sc.host_walk(scene, rays, any_hit, robust, original_ids, deep_cap=deep_cap, threads=8)
    got, got_inst, got_cnt = dev.trace(_cuda(rays), any_hit, robust, original_ids)
    assert sc.same_records(got, want), (any_hit, robust, original_ids)
    assert (got_inst == want_inst).all() and (got_cnt == want_cnt).all(), (got_cnt, want_cnt)
    return got, got_inst


def prepared_equals_host(dev):
    import bvh_amd
    w, bb, cc = bvh_amd.instance_prepare(dev.geoms, dev.obj2world, dev.gids)
    s = dev.scene
    assert w.cpu().numpy().tobytes() == s.world2obj.tobytes()
    assert bb.cpu().numpy().tobytes() == s.bboxes.tobytes() and cc.cpu().numpy().tobytes() == s.centers.tobytes()


# ---- G1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_device_equals_host_single_leaf_top(dll, orc, dtype):
    scene = sc.scene12(dll, orc, dtype)
    dev = DeviceScene(scene)
    prepared_equals_host(dev)
    rays = sc.scene_rays(scene, N_RAYS, seed=6)
    for any_hit, robust in MODES4:
        got, _ = same_as_host(dev, scene, rays, any_hit, robust)
        same_as_host(dev, scene, rays, any_hit, robust, original_ids=True)
        assert 1000 < (got["prim"] != INVALID).sum() < N_RAYS


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_device_equals_host_built_top(dll, orc, dtype):
    scene = sc.scene200(dll, orc, dtype)
    dev = DeviceScene(scene)
    prepared_equals_host(dev)
    rays = sc.scene_rays(scene, N_RAYS, seed=10)
    for any_hit, robust in MODES4:
        same_as_host(dev, scene, rays, any_hit, robust)


@pytest.mark.parametrize("depth", [65, 300])
def test_device_equals_host_deep_stack(dll, restatement, depth):
    scene, rays, deep_cap = sc.chain_scene(dll, restatement, depth, N_RAYS)
    dev = DeviceScene(scene)
    prepared_equals_host(dev)
    got = {mode: same_as_host(dev, scene, rays, *mode, deep_cap=deep_cap)[0] for mode in MODES4}
    assert (got[(False, True)]["prim"] == depth).sum() > 100  # closest-hit walks the whole chain: the deepest triangle is the nearest


def test_many_geometries_take_the_table_through_scratch(dll, orc):
    """More geometries than travel by value in the kernel arguments: the same scene with its three geometries listed 7 times over."""
    scene = sc.scene12(dll, orc, np.float32)
    gids = scene.gids + 3 * (np.arange(12, dtype=np.uint32) % 6)
    gids[9] = 40                                              # still outside the table
    many = sc.Scene(dll, scene.geoms * 7, scene.obj2world, gids).single_leaf_top()
    dev = DeviceScene(many)
    assert len(dev.geoms) == 21
    prepared_equals_host(dev)
    rays = sc.scene_rays(many, N_RAYS, seed=6)
    got, _ = same_as_host(dev, many, rays, False, True)
    same_as_host(dev, many, rays, True, False, original_ids=True)
    assert (got["prim"] != INVALID).sum() > 1000


# ---- G2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_device_equals_the_reference_composition(dll, orc, dtype):
    scene = sc.scene12(dll, orc, dtype)                       # (`orc` is the compiled reference here: its builder, its intersect_tri)
    dev = DeviceScene(scene)
    rays = sc.scene_rays(scene, N_RAYS, seed=12)
    for any_hit, robust in MODES4:
        for original_ids in (False, True):
            want, want_inst, want_cnt = expect_single_leaf(scene, rays, any_hit, robust, original_ids)
            got, got_inst, got_cnt = dev.trace(_cuda(rays), any_hit, robust, original_ids)
            assert sc.same_records(got, want), (any_hit, robust, original_ids)
            assert (got_inst == want_inst).all() and (got_cnt == want_cnt).all(), (got_cnt, want_cnt)


# ---- G3 ---------------------------------------------------------------------------------------------------------------------------
def test_moving_geometry_loop(dll, orc):
    import bvh_amd
    scene0 = sc.scene200(dll, orc, np.float32, seed=77)
    scene1 = sc.scene200(dll, orc, np.float32, seed=78)       # every instance somewhere else, the same geometries
    dev = DeviceScene(scene0, top=False)
    before = [g.serialize_device().cpu().numpy().tobytes() for g, _ in dev.geoms]
    w0, bb0, cc0 = bvh_amd.instance_prepare(dev.geoms, dev.obj2world, dev.gids)
    top = bvh_amd.DefaultBuilder.build(bb0, cc0)
    rays = sc.scene_rays(scene1, N_RAYS, seed=14)
    hits0, _, _ = dev.trace(_cuda(rays), False, True, top=top, world2obj=w0)
    # move: new matrices -> instance_prepare -> refit_boxes on the small top tree -> trace
    dev.gids = _cuda(scene1.gids)
    w1, bb1, cc1 = bvh_amd.instance_prepare(dev.geoms, _cuda(scene1.obj2world), dev.gids)
    assert w1.cpu().numpy().tobytes() == scene1.world2obj.tobytes() and bb1.cpu().numpy().tobytes() == scene1.bboxes.tobytes()
    top.refit_boxes(bb1)
    moved, moved_inst, _ = dev.trace(_cuda(rays), False, True, top=top, world2obj=w1)
    fresh_top = bvh_amd.DefaultBuilder.build(bb1, cc1)
    fresh, fresh_inst, _ = dev.trace(_cuda(rays), False, True, top=fresh_top, world2obj=w1)
    # the precondition of the order-free comparison: the reference alone does not care about the order of the instances
    forward, _, _ = sc.compose(scene1, rays, range(scene1.n), False, True)
    backward, _, _ = sc.compose(scene1, rays, range(scene1.n - 1, -1, -1), False, True)
    assert forward["t"].tobytes() == backward["t"].tobytes()
    assert moved["t"].tobytes() == fresh["t"].tobytes() == forward["t"].tobytes()
    hit = forward["prim"] != INVALID
    assert ((moved["prim"] != INVALID) == hit).all() and ((fresh["prim"] != INVALID) == hit).all() and 1000 < hit.sum() < N_RAYS
    assert moved["t"].tobytes() != hits0["t"].tobytes()       # the scene did move
    # the two trees may order a tie between two instances differently: there, each reported instance alone must give that t
    for k in np.nonzero(moved_inst != fresh_inst)[0]:
        for i in (moved_inst[k], fresh_inst[k]):
            alone, _, _ = sc.compose(scene1, rays[k:k + 1], [int(i)], False, True, tmax=forward["t"][k:k + 1])
            assert alone["prim"][0] != INVALID and alone["t"][0] == forward["t"][k]
    assert (moved_inst != fresh_inst).sum() <= N_RAYS // 100
    after = [g.serialize_device().cpu().numpy().tobytes() for g, _ in dev.geoms]
    assert before == after                                    # no geometry tree was touched


# ---- G4 ---------------------------------------------------------------------------------------------------------------------------
def test_two_threads_two_streams(dll, orc):
    import torch
    scene = sc.scene200(dll, orc, np.float32)
    dev = DeviceScene(scene)
    rays = _cuda(sc.scene_rays(scene, N_RAYS, seed=16))
    want = [dev.trace(rays, a, True) for a in (False, True)]
    torch.cuda.synchronize()
    out, errors = [None, None], []

    def work(k):
        try:
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                for _ in range(4):
                    out[k] = dev.trace(rays, bool(k), True)
            stream.synchronize()
        except BaseException as exc:                          # noqa: BLE001 (reported by the asserting thread)
            errors.append(exc)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(2):
        assert sc.same_records(out[k][0], want[k][0]) and (out[k][1] == want[k][1]).all() and (out[k][2] == want[k][2]).all()


def test_argument_errors(dll, orc):
    import torch
    import bvh_amd
    from bvh_amd import _lib
    lib = _lib.load()
    scene = sc.scene12(dll, orc, np.float32)
    dev = DeviceScene(scene)
    n = 64
    rays = _cuda(sc.scene_rays(scene, n, seed=18))
    table = (_lib.Geometry * 3)()
    for k, (g, t) in enumerate(dev.geoms):
        table[k].bvh, table[k].d_tris12 = g._h, t.data_ptr()
    hits = torch.full((n, 4), 7.0, dtype=torch.float32, device="cuda")
    inst = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    w, gid = dev.world2obj, dev.gids

    def call(top=dev.top._h, geoms=table, n_geoms=3, w2o=w.data_ptr(), g=gid.data_ptr(), n_inst=12, r=rays.data_ptr(), n_rays=n, flags=0,
             h=hits.data_ptr(), i=inst.data_ptr()):
        return lib.bvh3f_intersect_rays_instanced(top, geoms, n_geoms, w2o, g, n_inst, r, n_rays, flags, h, i, None, None)

    def refused(rc, text):
        assert rc < 0 and text in _lib.last_error(), (rc, _lib.last_error())

    refused(call(top=None), "null bvh")
    refused(call(r=None), "null device pointer")
    refused(call(h=None), "null device pointer")
    refused(call(i=None), "null device pointer")
    refused(call(w2o=None), "null device pointer")
    refused(call(r=rays.data_ptr() + 4), "aligned")
    refused(call(flags=SORTED), "unsupported flags")
    refused(call(flags=32), "unsupported flags")
    refused(call(n_geoms=0), "no geometries")
    refused(call(geoms=None), "no geometries")
    refused(call(n_inst=11), "instances given")
    bad = (_lib.Geometry * 3)()
    for k in range(3):
        bad[k].bvh, bad[k].d_tris12 = table[k].bvh, table[k].d_tris12
    bad[1].d_tris12 = None
    refused(call(geoms=bad), "geometry 1: null triangle array")
    bad[1].d_tris12, bad[2].bvh = table[1].d_tris12, None
    refused(call(geoms=bad), "geometry 2: null bvh")
    circles = np.array([[0, 0, 1.0], [3, 0, 1.0]], dtype=np.float32)
    flat = bvh_amd.DefaultBuilder.build(*bvh_amd.sphere_bounds(circles))
    bad[2].bvh = flat._h
    refused(call(geoms=bad), "geometry 2 belongs to another family")
    refused(lib.bvh3f_instance_prepare(bad, 3, dev.obj2world.data_ptr(), gid.data_ptr(), 12, w.data_ptr(), hits.data_ptr(), hits.data_ptr(), None),
            "geometry 2 belongs to another family")
    refused(lib.bvh3f_instance_prepare(table, 3, None, gid.data_ptr(), 12, w.data_ptr(), hits.data_ptr(), hits.data_ptr(), None), "null device pointer")
    torch.cuda.synchronize()
    assert (hits == 7.0).all() and (inst == 7).all()          # nothing was launched
    # an empty batch succeeds and touches nothing, whatever else is passed
    assert call(n_rays=0, r=None, h=None) == 0
    assert call(flags=UNSORTED | ROBUST) == 0
    torch.cuda.synchronize()
    assert not (inst == 7).all()
    with pytest.raises(TypeError):
        bvh_amd.intersect_instanced(dev.top, dev.geoms, w.double(), rays)
