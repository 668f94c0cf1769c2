"""MI355X: the instanced ray queries (bvh3X_instance_prepare / bvh3X_intersect_rays_instanced) on the adversarial scenes, rays and tree
shapes of tests/instanced_adversarial.py, through the C entry points, with `hits` and `hit_instances` between guard zones of sentinels
and the padding word of the double record pre-filled and checked (the ray queries store the record whole: the word comes back 0).

Device == host harness (the kernels' text compiled by g++) byte for byte — records, instances, counters, and the prepared instances —
on every class, tiny shape and ray kind of tests/test_instanced_fuzz_host.py, on top trees and a soup geometry built by the device
builders (read back for the harness), on tables of 16 and 17 geometries, and on the chain-shaped top trees over chain geometries,
where the device assembles its own stack bound and spill from the trees' depths. The exact tier and the float64 tier are run on the
device's own output, without the harness; the order-free and the one-sided properties likewise. The reference tree is not read: the
checker comes through the `orc` fixture."""
import numpy as np
import pytest

import instanced_adversarial as ia
import instanced_scenes as sc
import oracle
import test_instanced_fuzz_host as host
from conftest import parse_stream
from instanced_scenes import INVALID, MODES4
from test_gpu_overlap import _cuda, _np
from test_gpu_query_fuzz import device_build
from test_radius_search_host import GUARD, SENT_DIST

pytestmark = pytest.mark.gpu

ANY_HIT, ROBUST, ORIGINAL_IDS = 1, 2, 8
SENT_WORD = 0xABABABAB
N_RAYS = 4096 + 37                                             # more than one block spills; a ragged last block


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return sc.compile_harness(tmp_path_factory.mktemp("instanced_fuzz_gpu"))


class Device:
    """A Scene of instanced_scenes on the device, traced and prepared through the C entry points. Geometries and top tree come through
    from_nodes unless device trees are handed in."""

    def __init__(self, scene, geoms=None, top=None):
        import bvh_amd
        from bvh_amd import _lib
        self.lib, self.error, self.scene = _lib.load(), _lib.last_error, scene
        self.s = "3d" if scene.double else "3f"
        self.geoms = geoms if geoms is not None else [(bvh_amd.Bvh.from_nodes(g.nodes, g.ids), _cuda(g.tris12)) for g in scene.geoms]
        self.table = (_lib.Geometry * len(self.geoms))()
        for k, (g, t) in enumerate(self.geoms):
            self.table[k].bvh, self.table[k].d_tris12 = g._h, t.data_ptr()
        self.obj2world, self.world2obj = _cuda(scene.obj2world), _cuda(scene.world2obj)
        self.gids = None if scene.gids is None else _cuda(scene.gids)
        self.top = top

    def set_top(self, top=None):
        import bvh_amd
        self.top = top if top is not None else bvh_amd.Bvh.from_nodes(self.scene.top_nodes, self.scene.top_ids)
        return self

    def _gid(self):
        return None if self.gids is None else self.gids.data_ptr()

    def prepare(self):
        """bvh3X_instance_prepare with every output between guard zones. -> (world2obj, bboxes, centers) device tensors without the guards."""
        n, dt = self.scene.n, self.scene.dtype
        size = np.dtype(dt).itemsize
        out = [_cuda(np.full(k * n + 2 * GUARD, SENT_DIST, dtype=dt)) for k in (12, 6, 3)]
        f = getattr(self.lib, f"bvh{self.s}_instance_prepare")
        rc = f(self.table, len(self.geoms), self.obj2world.data_ptr(), self._gid(), n, *[o.data_ptr() + GUARD * size for o in out], None)
        assert rc == 0, self.error()
        inner = []
        for o, k in zip(out, (12, 6, 3)):
            a = _np(o)
            assert (a[:GUARD] == SENT_DIST).all() and (a[GUARD + k * n:] == SENT_DIST).all()
            inner.append(o[GUARD:GUARD + k * n].reshape(n, k).clone())
        return inner

    def prepared_equals_host(self):
        w, bb, cc = self.prepare()
        s = self.scene
        assert _np(w).tobytes() == s.world2obj.tobytes() and _np(bb).tobytes() == s.bboxes.tobytes() and _np(cc).tobytes() == s.centers.tobytes()
        return w, bb, cc

    def trace(self, rays, any_hit, robust, original_ids=False, world2obj=None):
        """bvh3X_intersect_rays_instanced. -> (hit records, instances, counters) as numpy, shaped like the harness's."""
        import torch
        n = len(rays)
        words = 8 if self.scene.double else 4
        d_rays = _cuda(np.ascontiguousarray(rays, dtype=self.scene.dtype))
        hits = _cuda(np.full(words * n + 2 * GUARD, SENT_WORD, dtype=np.uint32))
        inst = _cuda(np.full(n + 2 * GUARD, SENT_WORD, dtype=np.uint32))
        cnt = torch.zeros(3, dtype=torch.int64, device="cuda")
        flags = (ANY_HIT if any_hit else 0) | (ROBUST if robust else 0) | (ORIGINAL_IDS if original_ids else 0)
        w = self.world2obj if world2obj is None else world2obj
        f = getattr(self.lib, f"bvh{self.s}_intersect_rays_instanced")
        rc = f(self.top._h, self.table, len(self.geoms), w.data_ptr(), self._gid(), self.scene.n, d_rays.data_ptr(), n, flags,
               hits.data_ptr() + 4 * GUARD, inst.data_ptr() + 4 * GUARD, cnt.data_ptr(), None)
        assert rc == 0, self.error()
        torch.cuda.synchronize()
        h, i = _np(hits, np.uint32), _np(inst, np.uint32)
        for a, total in ((h, words * n), (i, n)):
            assert (a[:GUARD] == SENT_WORD).all() and (a[GUARD + total:] == SENT_WORD).all()
        inner = h[GUARD:GUARD + words * n].copy()
        if self.scene.double:
            assert (inner[1::8] == 0).all()                    # bvh_hit3d is stored whole, as bvh3d_intersect_rays_tri stores it: pad = 0
        i = i[GUARD:GUARD + n].copy()
        assert not (i == SENT_WORD).any()
        return inner.view(oracle.HITD if self.scene.double else oracle.HITF).reshape(-1), i, _np(cnt).astype(np.uint64)


def same_as_host(dev, rays, modes=MODES4, ids=(False, True), deep_cap=0):
    """Device == harness byte for byte in every mode. -> {(any_hit, robust): the device's (records, instances)} under default ids."""
    out = {}
    for any_hit, robust in modes:
        for original_ids in ids:
            want, want_inst, want_cnt = sc.host_walk(dev.scene, rays, any_hit, robust, original_ids, deep_cap=deep_cap, threads=8)
            got, inst, cnt = dev.trace(rays, any_hit, robust, original_ids)
            assert sc.same_records(got, want), (any_hit, robust, original_ids)
            assert (inst == want_inst).all() and (cnt == want_cnt).all(), (any_hit, robust, original_ids, cnt, want_cnt)
            if not original_ids:
                out[(any_hit, robust)] = (got, inst)
    return out


# ---- single-leaf top trees: classes, tiny shapes, special rays ------------------------------------------------------------------------

@pytest.mark.parametrize("case", host.single_leaf_cases() + host.TINY, ids=host.case_id)
def test_single_leaf_device_equals_host(dll, orc, case):
    n = case[2]
    which = None
    if case in host.TINY and n == 15:
        slots = host.single_leaf_scene(dll, orc, case, dead=0)[0].top_ids
        which = [int(slots[0]), int(slots[7]), int(slots[14])]
    scene, rays, _ = host.single_leaf_scene(dll, orc, case, dead=0 if case in host.TINY else 0.1, which=which)
    dev = Device(scene).set_top()
    dev.prepared_equals_host()
    same_as_host(dev, rays)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_all_dead_scene(dll, orc, dtype):
    scene, rays, dead_ids = host.single_leaf_scene(dll, orc, ("dead", ("benign", "far"), 12, 0, dtype, 257, 350), dead=0, which=list(range(12)))
    dev = Device(scene).set_top()
    dev.prepared_equals_host()
    for (any_hit, robust), (got, inst) in same_as_host(dev, rays).items():
        assert (got["prim"] == INVALID).all() and (inst == INVALID).all()
    import bvh_amd
    w, bb, cc = dev.prepare()
    dev.set_top(bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(min_leaf_size=1, max_leaf_size=1)))
    scene.top_nodes, scene.top_ids = dev.top.nodes, dev.top.prim_ids
    for (any_hit, robust), (got, inst) in same_as_host(dev, rays).items():
        assert (got["prim"] == INVALID).all() and (inst == INVALID).all()


# ---- the exact tier and the float64 tier on the device's own output ----------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("seed,n_inst,n_rays", [(401, 15, 1021), (402, 1, 65), (403, 6, 257)])
def test_exact_tier_on_the_device(dll, orc, seed, n_inst, n_rays, dtype):
    scene, tris, rays = host.exact_scene(dll, orc, seed, n_inst, n_rays, dtype)
    dev = Device(scene).set_top()
    w, _, _ = dev.prepare()
    results = {}
    for any_hit in (False, True):
        for robust in (False, True):
            got, inst, _ = dev.trace(rays, any_hit, robust, world2obj=w)
            if any_hit in results:
                assert sc.same_records(got, results[any_hit][0]) and (inst == results[any_hit][1]).all()
            results[any_hit] = (got, inst)
    witnesses = host.check_exact(_np(w), scene.top_ids, scene.obj2world, tris, scene.gids, rays, results, (seed, np.dtype(dtype).name))
    if n_rays >= 1021:
        assert min(witnesses[False]) > 0


@pytest.mark.parametrize("kind,dtype,seed", host.TRUTH_CASES, ids=[f"{k}-{np.dtype(d).name}" for k, d, _ in host.TRUTH_CASES])
def test_float64_truth_on_the_device(dll, orc, kind, dtype, seed):
    """test_instanced_fuzz_host.test_float64_truth's checks on the device's records (its docstring has the measured tolerances)."""
    import bvh_amd
    scene, rays = host.truth_scene(dll, orc, kind, dtype, seed)
    truth, excused, ref_err = host.reference_against_truth(scene, rays, kind, dtype)
    dev = Device(scene)
    w, bb, cc = dev.prepared_equals_host()
    dev.set_top(bvh_amd.DefaultBuilder.build(bb, cc))
    got, inst, _ = dev.trace(rays, False, True, original_ids=True, world2obj=w)
    err, _ = ia.check_against_truth(truth, got, inst, "the device", excused)
    assert err <= 4 * ref_err, (err, ref_err)
    got_any, _, _ = dev.trace(rays, True, True, original_ids=True, world2obj=w)
    clear = ~truth[4] & ~excused
    assert ((got_any["prim"] != INVALID)[clear] == truth[0][clear]).all()


# ---- top trees and a geometry from the device builders ----------------------------------------------------------------------------------

def device_soup(orc, dtype, lim, bq):
    """The 300-triangle soup on a tree from a device builder, read back through serialize_device / parse_stream for the harness.
    -> (Geometry, (Bvh, BVH-order triangles in HBM))."""
    import bvh_amd
    raw = ia.soup300(dtype)
    bb, cc = bvh_amd.tri_bounds(raw)
    bvh = device_build(bb, cc, lim, bq)
    nodes, ids = parse_stream(_np(bvh.serialize_device()).tobytes(), dtype == np.float64)
    geom = sc.Geometry(orc, raw, nodes, ids)
    tris = bvh_amd.precompute_tris(raw, bvh.device_prim_ids())
    assert _np(tris).tobytes() == geom.tris12.tobytes()
    return geom, (bvh, tris)


BUILT_CASES = host.built_cases(7, 2)


@pytest.mark.parametrize("case", BUILT_CASES, ids=host.built_id)
def test_device_built_top_trees(dll, orc, case):
    import bvh_amd
    kind, n, lim, bq, dtype, table, seed = case
    soup, soup_dev = device_soup(orc, dtype, (1, 8) if seed % 2 else (3, 15), bq)
    scene, rng = host.built_scene_parts(dll, orc, case, soup)
    geoms = [soup_dev if g is soup else (bvh_amd.Bvh.from_nodes(g.nodes, g.ids), _cuda(g.tris12)) for g in scene.geoms]
    dev = Device(scene, geoms)
    w, bb, cc = dev.prepared_equals_host()
    dev.set_top(device_build(bb, cc, lim, bq))
    scene.top_nodes, scene.top_ids = dev.top.nodes, dev.top.prim_ids
    counts = scene.top_nodes["index"].astype(np.uint64) & np.uint64(15)
    assert counts.max() <= lim[1] and sorted(scene.top_ids.tolist()) == list(range(n))
    rays = host.built_rays(scene, rng, seed)
    out = same_as_host(dev, rays)
    (got, inst), (got_any, inst_any) = out[(False, True)], out[(True, True)]
    assert ia.order_free(orc, scene, rays, got, inst, got_any, inst_any) > 500
    stable = ia.order_insensitive(scene, rays)
    assert stable.mean() > 0.98
    for any_hit in (False, True):
        common, _, _ = sc.compose(scene, rays, range(scene.n), any_hit, True)      # (robust: see one_sided)
        if any_hit:
            common["t"] = np.where(common["prim"] != INVALID, -np.inf, common["t"]).astype(scene.dtype)
        fast, fast_inst = out[(any_hit, False)]
        lost, of = ia.one_sided(orc, scene, rays, common, fast, fast_inst, False, host.built_id(case), stable)
        print(f"{host.built_id(case)} {'any' if any_hit else 'closest'}-hit fast mode on the device: lost {lost} of {of} hits of the composition")


# ---- deep stacks: the device's own bound and spill -------------------------------------------------------------------------------------

@pytest.mark.parametrize("top_depth,geom_depth", ia.CHAIN_CASES)
def test_chain_top_tree_device_equals_host(dll, restatement, top_depth, geom_depth):
    """The only test of launch_instanced's bound = depth(top) + 1 + deepest geometry and cap = bound - 64 + 1 with a top depth above 0."""
    scene, rays, deep_cap, _ = ia.chain_top_scene(dll, restatement, top_depth, geom_depth, N_RAYS)   # (trees deeper than 64: conftest.restatement)
    dev = Device(scene).set_top()
    dev.prepared_equals_host()
    out = same_as_host(dev, rays, ids=(False,), deep_cap=deep_cap)
    got, inst = out[(False, True)]
    deepest = inst == top_depth
    assert deepest.sum() > N_RAYS // 4 and (got["prim"][deepest] == geom_depth).mean() > 0.9
