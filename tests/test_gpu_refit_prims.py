"""-m gpu: refit of a resident tree from moved primitives (Bvh.refit_boxes / Bvh.refit_tris / Bvh.traversal_cost) against the checker.
Expected leaf boxes come from the numpy model of the reference's fold (tests/test_refit_prims_host.py: leaf_boxes), inner boxes from
the checker's unmodified Bvh::refit on those arrays; every comparison is `==` on bytes (traversal_cost: the truncation bound of its
integer sum)."""
import ctypes as C

import numpy as np
import pytest

import oracle
from bvh_amd import synth
from conftest import MODES
from test_refit_prims_host import leaf_boxes

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


def _scene(name, n, dtype):
    return {"soup": lambda: synth.soup(n, dtype=dtype), "sponza": lambda: synth.sponza_proxy(n, dtype=dtype),
            "terrain": lambda: synth.terrain(n, dtype=dtype)}[name]()


def _build(bb, cc, mode):
    import bvh_amd
    name, builder, quality = mode
    if name == "binned":
        return bvh_amd.BinnedSahBuilder.build(bb, cc)
    if name == "sweep":
        return bvh_amd.SweepSahBuilder.build(bb, cc)
    return bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality(quality)),
                                        thread_pool=bvh_amd.ThreadPool() if builder == oracle.BUILDER_DEFAULT_PARALLEL else None)


def _extent(points):
    v = np.asarray(points, np.float64)
    return float((v.max(0) - v.min(0)).max())


def displaced(tris, frac, seed, part=1.0):
    """Every vertex (of a `part` of the triangles) moved by up to `frac` of the scene extent per component, seeded."""
    rng = np.random.default_rng(seed)
    d = ((rng.random(tris.shape) - 0.5) * 2 * frac * _extent(tris.reshape(-1, 3))).astype(tris.dtype)
    if part < 1.0:
        d[rng.random(len(tris)) >= part] = 0
    return np.ascontiguousarray(tris + d)


def displaced_centres(sph, frac, seed):
    dim = sph.shape[1] - 1
    rng = np.random.default_rng(seed)
    out = sph.copy()
    out[:, :dim] += ((rng.random((len(sph), dim)) - 0.5) * 2 * frac * _extent(sph[:, :dim])).astype(sph.dtype)
    return np.ascontiguousarray(out)


def expected_tree(orc, nodes, ids, bb, dim=3):
    """The reference's tree after refit(leaf_fn): leaf boxes from the model of its fold, inner boxes from its own Bvh::refit."""
    want = nodes.copy()
    leaves, boxes = leaf_boxes(nodes, ids, bb, dim)
    want["bounds"][leaves] = boxes
    tree = orc.from_arrays(want, ids)
    tree.refit()
    return tree


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scene", ["soup", "sponza", "terrain"])
def test_identity_and_moved_geometry_all_modes(orc, scene, dtype):
    """1 + 2: with the build's own boxes a refit leaves the stream unchanged (boxes and triangles, first call and steady state);
    after every vertex moved by 2 % of the extent, the stream equals model + reference refit, from boxes and from triangles."""
    import bvh_amd
    tris = _scene(scene, 20_000, dtype)
    bb, cc = orc.prep_tris(tris)
    tris2 = displaced(tris, 0.02, 11)
    bb2, _ = orc.prep_tris(tris2)
    d_bb2, _ = bvh_amd.tri_bounds(tris2)
    assert d_bb2.cpu().numpy().tobytes() == bb2.tobytes()
    for mode in MODES:
        gpu = _build(bb, cc, mode)
        fresh = _build(bb, cc, mode)                          # never touched by the host before its first refit: the resident path from call one
        fresh.refit_boxes(bb)
        s0 = gpu.serialize()
        assert fresh.serialize() == s0, (mode[0], "refit_boxes on a tree whose mirror was never filled")
        gpu.refit_boxes(bb)                                   # mirror valid (serialize filled it): pushed first
        gpu.refit_boxes(bb)                                   # steady state
        assert gpu.serialize() == s0, (mode[0], "refit_boxes")
        out = gpu.refit_tris(tris)
        out = gpu.refit_tris(tris, out=out)
        assert gpu.serialize() == s0, (mode[0], "refit_tris")
        assert out.cpu().numpy().tobytes() == bvh_amd.precompute_tris(tris, gpu.device_prim_ids()).cpu().numpy().tobytes(), mode[0]
        nodes, ids = gpu.nodes, gpu.prim_ids
        want = expected_tree(orc, nodes, ids, bb2)
        gpu.refit_boxes(d_bb2)
        assert gpu.serialize() == want.serialize(), (mode[0], "moved, refit_boxes")
        fresh.refit_tris(tris2)
        out2 = fresh.refit_tris(tris2)
        assert fresh.serialize() == want.serialize(), (mode[0], "moved, refit_tris")
        assert out2.cpu().numpy().tobytes() == orc.precompute_tris(tris2, ids).tobytes(), mode[0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_moved_spheres_and_circles(orc, dtype):
    """2: spheres (3D) and circles (2D, 20 / 40-byte nodes): sphere_bounds -> refit_boxes."""
    import bvh_amd
    sph = synth.spheres(20_000, dtype=dtype)
    circ = synth.circles(20_000, dtype=dtype)
    for prims, dim in ((sph, 3), (circ, 2)):
        bb, cc = orc.sphere_bboxes(prims)
        for quality in (bvh_amd.Quality.Low, bvh_amd.Quality.High):
            gpu = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=quality))
            assert gpu.dim == dim
            gpu.refit_boxes(bb)
            s0 = orc.build(bb, cc, builder=oracle.BUILDER_DEFAULT_SERIAL, quality=int(quality)).serialize()
            assert gpu.serialize() == s0, (dim, quality, "identity")
            moved = displaced_centres(prims, 0.02, 5)
            bb2, _ = orc.sphere_bboxes(moved)
            d_bb2, _ = bvh_amd.sphere_bounds(moved)
            assert d_bb2.cpu().numpy().tobytes() == bb2.tobytes()
            want = expected_tree(orc, gpu.nodes, gpu.prim_ids, bb2, dim)
            gpu.refit_boxes(d_bb2)
            gpu.refit_boxes(d_bb2)
            assert gpu.serialize() == want.serialize(), (dim, quality, "moved")
            assert gpu.nodes.dtype.itemsize == {(3, 4): 28, (3, 8): 56, (2, 4): 20, (2, 8): 40}[(dim, np.dtype(dtype).itemsize)]


def _trace_all(bvh_amd, gpu, prims, ref, oprims, rays, srays, what, leaf="tri"):
    cpu_trace = ref.intersect_tri if leaf == "tri" else ref.intersect_sphere
    for any_hit, robust in ((False, True), (False, False), (True, True), (True, False)):
        want = cpu_trace(oprims, srays if any_hit else rays, any_hit, robust, threads=8)
        for sort_rays in (None, True):
            got = bvh_amd.intersect(gpu, prims, srays if any_hit else rays, any_hit=any_hit, robust=robust, sort_rays=sort_rays, leaf=leaf)
            assert bvh_amd.hits_to_numpy(got).tobytes() == want.tobytes(), (what, any_hit, robust, sort_rays)


@pytest.mark.parametrize("dtype", DTYPES)
def test_tracing_and_closest_points_on_the_refitted_tree(orc, dtype):
    """3: hits equal the reference's on ITS refitted tree with ITS re-precomputed triangles, also reordered, also after the whole scene
    moved by ten times its extent (the root box the reordering keys are scaled by must have followed); closest_points equals the
    same query on a fresh upload of the expected arrays."""
    import bvh_amd
    tris = synth.soup(20_000, dtype=dtype)
    bb, cc = orc.prep_tris(tris)
    gpu = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.High), thread_pool=bvh_amd.ThreadPool())
    nodes, ids = gpu.nodes, gpu.prim_ids
    lo, hi = synth.scene_bounds(tris)
    prims0 = bvh_amd.precompute_tris(tris, gpu.device_prim_ids())
    bvh_amd.intersect(gpu, prims0, synth.rays_closest(50_000, lo, hi, dtype=dtype), sort_rays=True)      # the old root box has been used
    tris2 = displaced(tris, 0.02, 3)
    shift = (10.0 * (hi - lo)).astype(dtype)
    tris3 = np.ascontiguousarray((tris2.reshape(-1, 3, 3) + shift).reshape(-1, 9).astype(dtype))
    for what, moved in (("moved", tris2), ("translated", tris3)):
        prims = gpu.refit_tris(moved)
        ref = expected_tree(orc, nodes, ids, orc.prep_tris(moved)[0])
        oprims = orc.precompute_tris(moved, ids)
        lo2, hi2 = synth.scene_bounds(moved)
        rays = synth.rays_closest(50_000, lo2, hi2, dtype=dtype)
        srays = synth.rays_shadow(50_000, lo2, hi2, dtype=dtype)
        _trace_all(bvh_amd, gpu, prims, ref, oprims, rays, srays, what)
        upload = bvh_amd.Bvh.from_nodes(ref.nodes(), ids)     # an upload path the refit does not touch
        pts = np.concatenate([synth.points_uniform(20_000, lo2, hi2, dtype=np.float64),
                              synth.points_near_surface(moved.astype(np.float64), 20_000, sigma=0.01 * float(np.max(hi2 - lo2)))]).astype(dtype)
        for sort_queries in (False, True):
            got = bvh_amd.closest_points(gpu, prims, pts, sort_queries=sort_queries)
            want = bvh_amd.closest_points(upload, torch_from(oprims), pts, sort_queries=sort_queries)
            assert bvh_amd.hits_to_numpy(got).tobytes() == bvh_amd.hits_to_numpy(want).tobytes(), (what, sort_queries)
            assert (bvh_amd.hits_to_numpy(got)["prim"] != bvh_amd.INVALID).all()
        assert gpu.serialize() == ref.serialize(), what


def torch_from(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("dtype", DTYPES)
def test_tracing_refitted_circles(orc, dtype):
    """3, 2D: circles moved, then the whole scene translated by ten times its extent."""
    import bvh_amd
    circ = synth.circles(20_000, dtype=dtype)
    bb, cc = orc.sphere_bboxes(circ)
    gpu = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.High))
    nodes, ids = gpu.nodes, gpu.prim_ids
    perm = ids.astype(np.int64)
    moved = displaced_centres(circ, 0.02, 8)
    far = moved.copy()
    far[:, :2] += dtype(10.0 * _extent(circ[:, :2]))
    for what, cur in (("moved", moved), ("translated", far)):
        bb2, _ = orc.sphere_bboxes(cur)
        gpu.refit_boxes(bb2)
        ref = expected_tree(orc, nodes, ids, bb2, 2)
        lo, hi = cur[:, :2].min(0).astype(np.float64), cur[:, :2].max(0).astype(np.float64)
        rays = synth.rays_2d(50_000, lo, hi, dtype=dtype)
        srays = synth.rays_2d(50_000, lo, hi, seed=99, dtype=dtype, segment=True)
        _trace_all(bvh_amd, gpu, bvh_amd.gather(cur, gpu.device_prim_ids()), ref, np.ascontiguousarray(cur[perm]), rays, srays, what, leaf="sphere")
        assert gpu.serialize() == ref.serialize(), what


@pytest.mark.parametrize("dtype", DTYPES)
def test_frames_on_a_side_stream(orc, dtype):
    """4: five frames on a non-default stream, refit_tris then intersect with nothing in between; the scratch cache does not grow."""
    import torch
    import bvh_amd
    lib = bvh_amd._lib.load()
    tris = synth.sponza_proxy(20_000, dtype=dtype)
    bb, cc = orc.prep_tris(tris)
    gpu = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.High), thread_pool=bvh_amd.ThreadPool())
    nodes, ids = gpu.nodes, gpu.prim_ids
    gpu.refit_tris(tris)                                      # the one-offs (mirror pushed, largest id) happen before the loop
    lo, hi = synth.scene_bounds(tris)
    rays = synth.rays_closest(50_000, lo, hi, dtype=dtype)
    frames = [displaced(tris, 0.02, 100 + f) for f in range(5)]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    hits, cached = [], []
    with torch.cuda.stream(side):
        d_frames = [torch.from_numpy(f).cuda() for f in frames]
        d_rays = torch.from_numpy(rays).cuda()
        prims = torch.empty((len(tris), 12), dtype=d_frames[0].dtype, device="cuda")
        for f in range(5):
            gpu.refit_tris(d_frames[f], out=prims)
            hits.append(bvh_amd.intersect(gpu, prims, d_rays, robust=True))
            cached.append(lib.bvh_amd_cached_scratch_bytes())
        side.synchronize()
    assert cached[4] <= cached[1], cached
    for f in range(5):
        ref = expected_tree(orc, nodes, ids, orc.prep_tris(frames[f])[0])
        want = ref.intersect_tri(orc.precompute_tris(frames[f], ids), rays, False, True, threads=8)
        assert bvh_amd.hits_to_numpy(hits[f]).tobytes() == want.tobytes(), f
    assert gpu.serialize() == ref.serialize()


class _Million:
    def __init__(self, dtype):
        import torch
        import bvh_amd
        self.dtype = dtype
        self.tris = synth.soup(1_000_000, dtype=dtype)
        self.d_tris = torch.from_numpy(self.tris).cuda()
        d_bb, d_cc = bvh_amd.tri_bounds(self.d_tris)
        self.gpu = bvh_amd.DefaultBuilder.build(d_bb, d_cc, bvh_amd.Config(quality=bvh_amd.Quality.High), thread_pool=bvh_amd.ThreadPool())
        self.prims = bvh_amd.precompute_tris(self.d_tris, self.gpu.device_prim_ids())
        self.lo, self.hi = synth.scene_bounds(self.tris)


@pytest.fixture(scope="module", params=DTYPES, ids=["float32", "float64"])
def million(request):
    m = _Million(request.param)
    yield m
    del m


def test_measured_plan_survives_a_refit(orc, million):
    """5: the measured launch plan of a 1M-triangle tree (records beyond the L2) is settled after ten batches of 2^20 rays and is the
    plan of EACH of the three batches after refit_tris; the first of them equals the reference on its refitted tree."""
    import torch
    import bvh_amd
    lib = bvh_amd._lib.load()
    m = million
    rays = synth.rays_closest(1 << 20, m.lo, m.hi, seed=5, dtype=m.dtype)
    d_rays = torch.from_numpy(rays).cuda()
    plan = (C.c_int * 4)()
    plans = []
    for _ in range(10):
        bvh_amd.intersect(m.gpu, m.prims, d_rays, robust=True)
        torch.cuda.synchronize()                              # a caller that consumes each batch: the search reads a finished measurement at the next call
        lib.bvh_amd_last_launch_plan(plan)
        plans.append(list(plan))
    assert plans[8] == plans[9], plans
    settled = plans[9]
    tris2 = displaced(m.tris, 0.005, 21)
    prims2 = m.gpu.refit_tris(tris2)
    after, first = [], None
    for k in range(3):
        got = bvh_amd.intersect(m.gpu, prims2, d_rays, robust=True)
        torch.cuda.synchronize()
        lib.bvh_amd_last_launch_plan(plan)
        after.append(list(plan))
        if k == 0:
            first = bvh_amd.hits_to_numpy(got)
    assert after == [settled] * 3, (plans, after)
    nodes, ids = m.gpu.nodes, m.gpu.prim_ids                  # (the host mirror is read only now: a read before would have been a push at the refit)
    ref = expected_tree(orc, nodes, ids, orc.prep_tris(tris2)[0])
    assert nodes.tobytes() == ref.nodes().tobytes()
    want = ref.intersect_tri(orc.precompute_tris(tris2, ids), rays, False, True, threads=16)
    assert first.tobytes() == want.tobytes()
    m.gpu.refit_tris(m.d_tris)                                # back to the start for the next test


def test_cross_xcd_hand_off_at_a_million_triangles(orc, million):
    """6: half the triangles of the 1M tree moved, three repetitions from the same start: the 1.9M-node climb hands boxes between
    lanes on all eight XCDs, and a stale box anywhere would show in the stream (tests/test_gpu_build.py's pattern)."""
    m = million
    m.gpu.refit_tris(m.d_tris)
    start = m.gpu.serialize()
    nodes, ids = m.gpu.nodes, m.gpu.prim_ids
    tris2 = displaced(m.tris, 0.01, 33, part=0.5)
    assert 0.4 < float((tris2 != m.tris).any(axis=1).mean()) < 0.6
    want = expected_tree(orc, nodes, ids, orc.prep_tris(tris2)[0]).serialize()
    assert want != start
    for rep in range(3):
        m.gpu.refit_tris(m.d_tris)                            # (pushes the mirror the serialize above filled, then) the start again
        m.gpu.refit_tris(tris2)                               # steady state: no host copy in this call
        assert m.gpu.serialize() == want, rep
    m.gpu.refit_tris(m.d_tris)
    assert m.gpu.serialize() == start


def _wide_array(nodes):
    """tests/test_gpu_build.py's array with unused sibling pairs: an unused subtree and a deep unused chain behind the reachable tree."""
    n = len(nodes)
    leaves = np.flatnonzero(nodes["index"] & 15)
    extra = np.zeros(4, dtype=nodes.dtype)
    extra["bounds"] = nodes["bounds"][1]
    extra["index"][0] = (n + 2) << 4                          # inner: children at n + 2, n + 3
    extra["index"][1] = (0 << 4) | 1
    extra["index"][2] = (0 << 4) | 1
    extra["index"][3] = (1 << 4) | 1
    extra["bounds"][2] = nodes["bounds"][leaves[0]]
    extra["bounds"][3] = nodes["bounds"][leaves[1]]
    chain = np.zeros(160, dtype=nodes.dtype)
    base = n + 4
    for lvl in range(80):
        chain["bounds"][2 * lvl] = nodes["bounds"][2]
        chain["bounds"][2 * lvl + 1] = nodes["bounds"][2]
        chain["index"][2 * lvl] = ((base + 2 * (lvl + 1)) << 4) if lvl < 79 else ((0 << 4) | 1)
        chain["index"][2 * lvl + 1] = (0 << 4) | 1
    return np.concatenate([nodes, extra, chain])


@pytest.mark.parametrize("dtype", DTYPES)
def test_mirror_coherence(orc, dtype):
    """7: the mirror follows a refit; a host edit of an inner box made before it does not survive; trees that start on the host
    (from_nodes, deserialize) and an array with unused sibling pairs refit correctly."""
    import bvh_amd
    tris = synth.soup(20_000, seed=21, jitter=0.02, dtype=dtype)
    bb, cc = orc.prep_tris(tris)
    bb2, _ = orc.prep_tris(displaced(tris, 0.02, 4))
    bb3, _ = orc.prep_tris(displaced(tris, 0.02, 5))
    gpu = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.Medium))
    nodes, ids = gpu.nodes, gpu.prim_ids
    want2, want3 = expected_tree(orc, nodes, ids, bb2), expected_tree(orc, nodes, ids, bb3)
    gpu.refit_boxes(bb2)
    assert gpu.nodes.tobytes() == want2.nodes().tobytes() and gpu.nodes.tobytes() != nodes.tobytes()
    inner = int(np.flatnonzero((nodes["index"] & 15) == 0)[7])
    gpu.set_node_bbox(inner, [-100.0, -100.0, -100.0], [100.0, 100.0, 100.0])
    gpu.refit_boxes(bb3)
    assert gpu.serialize() == want3.serialize()
    assert gpu.node_count == len(nodes) and (gpu.prim_ids == ids).all()
    prims = bvh_amd.precompute_tris(tris, gpu.device_prim_ids())
    lo, hi = synth.scene_bounds(tris)
    rays = synth.rays_closest(20_000, lo, hi, dtype=dtype)
    assert bvh_amd.hits_to_numpy(bvh_amd.intersect(gpu, prims, rays, robust=True)).tobytes() == \
        want3.intersect_tri(orc.precompute_tris(tris, ids), rays, False, True, threads=8).tobytes()
    # trees without resident nodes yet
    for make in (lambda: bvh_amd.Bvh.from_nodes(nodes, ids), lambda: bvh_amd.Bvh.deserialize(want3.serialize(), dtype=dtype)):
        t = make()
        t.refit_boxes(bb2)
        t.refit_boxes(bb2)
        assert t.serialize() == want2.serialize()
    # unused sibling pairs: every leaf of the ARRAY is refitted, like the reference's traverse_bottom_up
    wide = _wide_array(nodes)
    t = bvh_amd.Bvh.from_nodes(wide, ids)
    want = expected_tree(orc, wide, ids, bb2)
    t.refit_boxes(bb2)
    assert t.serialize() == want.serialize()
    t.refit_boxes(bb3)
    assert t.serialize() == expected_tree(orc, wide, ids, bb3).serialize()


@pytest.mark.parametrize("dtype", DTYPES)
def test_edges_and_refusals(orc, dtype):
    """8."""
    import torch
    import bvh_amd
    lib = bvh_amd._lib.load()
    sfx = "3f" if dtype == np.float32 else "3d"
    # one primitive: the root is a leaf
    one = synth.soup(1, dtype=dtype)
    bb, cc = orc.prep_tris(one)
    gpu = bvh_amd.DefaultBuilder.build(bb, cc)
    assert gpu.node_count == 1
    moved = np.ascontiguousarray(one + dtype(0.25))
    out = gpu.refit_tris(moved)
    want = expected_tree(orc, gpu.nodes, gpu.prim_ids, orc.prep_tris(moved)[0])
    assert gpu.serialize() == want.serialize()
    assert (gpu.nodes["bounds"][0, 0::2] == orc.prep_tris(moved)[0][0, :3]).all()
    assert out.cpu().numpy().tobytes() == orc.precompute_tris(moved, gpu.prim_ids).tobytes()
    rays = synth.rays_closest(1000, *synth.scene_bounds(moved), dtype=dtype)
    assert bvh_amd.hits_to_numpy(bvh_amd.intersect(gpu, out, rays, robust=True, sort_rays=True)).tobytes() == \
        want.intersect_tri(orc.precompute_tris(moved, gpu.prim_ids), rays, False, True, threads=1).tobytes()
    assert gpu.traversal_cost() == 0.0
    # leaves of up to 15 primitives
    tris = synth.soup(20_000, dtype=dtype)
    bb, cc = orc.prep_tris(tris)
    for quality in (bvh_amd.Quality.Low, bvh_amd.Quality.High):
        gpu = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=quality, min_leaf_size=9, max_leaf_size=15))
        assert int((gpu.nodes["index"] & 15).max()) > 8
        tris2 = displaced(tris, 0.02, 6)
        want = expected_tree(orc, gpu.nodes, gpu.prim_ids, orc.prep_tris(tris2)[0])
        gpu.refit_tris(tris2)
        assert gpu.serialize() == want.serialize(), quality
    # refusals leave the tree alone
    before = gpu.serialize()
    largest = int(gpu.prim_ids.max())
    with pytest.raises(bvh_amd.BvhAmdError, match="indexed by original primitive id"):
        gpu.refit_boxes(bb[:largest])
    with pytest.raises(bvh_amd.BvhAmdError, match="indexed by original primitive id"):
        gpu.refit_tris(tris[:largest])
    d_bb = torch.from_numpy(bb).cuda()
    for call in (lambda: getattr(lib, f"bvh{sfx}_refit_boxes")(None, d_bb.data_ptr(), len(bb), None),
                 lambda: getattr(lib, f"bvh{sfx}_refit_boxes")(gpu._h, None, len(bb), None),
                 lambda: getattr(lib, f"bvh{sfx}_refit_tris")(gpu._h, None, len(bb), None, None),
                 lambda: getattr(lib, f"bvh{sfx}_traversal_cost")(gpu._h, None, None)):
        assert call() < 0 and bvh_amd._lib.last_error()
    other = np.float64 if dtype == np.float32 else np.float32
    with pytest.raises(TypeError):
        gpu.refit_boxes(bb.astype(other))
    with pytest.raises(TypeError):
        gpu.refit_tris(tris.astype(other))
    with pytest.raises(TypeError):
        gpu.refit_tris(torch.from_numpy(tris.astype(other)).cuda())
    assert gpu.serialize() == before
    gpu.refit_boxes(bb[:largest + 1] if largest + 1 < len(bb) else bb)     # exactly enough is accepted


def _cost_model(nodes):
    b = nodes["bounds"].astype(np.float64)
    x, y, z = b[:, 1] - b[:, 0], b[:, 3] - b[:, 2], b[:, 5] - b[:, 4]
    area = x * y + y * z + z * x
    inner = np.flatnonzero((nodes["index"] & 15) == 0)
    inner = inner[inner != 0]                                 # the root is nobody's child: k_expected_visits has no term for it
    return float((area[inner] / area[0]).sum()), len(inner)


def _check_cost(gpu):
    got = gpu.traversal_cost()
    want, n_inner = _cost_model(gpu.nodes)
    assert n_inner * 2.0 ** -16 < 0.4
    assert (want - n_inner * 2.0 ** -16) * (1 - 1e-9) <= got <= want * (1 + 1e-9), (got, want, n_inner)
    return got


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scene", ["soup", "sponza", "terrain"])
def test_traversal_cost(orc, scene, dtype):
    """9: the float64 sum over the inner nodes other than the root of half_area(node) / half_area(root), each term truncated to
    units of 2^-16 by the kernel; it grows when a refit scatters the primitives."""
    import bvh_amd
    tris = _scene(scene, 20_000, dtype)
    bb, cc = orc.prep_tris(tris)
    gpu = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.High), thread_pool=bvh_amd.ThreadPool())
    before = _check_cost(gpu)
    gpu.refit_tris(displaced(tris, 0.02, 2))
    _check_cost(gpu)
    if scene == "soup":
        gpu.refit_tris(displaced(tris, 0.5, 3))
        assert _check_cost(gpu) > before
