"""CPU: the second and later launches of a batch that point_query_run (bvh_amd/csrc/point_query.h) and the instanced driver
(instanced.hip) cut into slices because the tree is deeper than 64 levels. The harnesses' slice entries (tests/cpp/*_body_host.cpp:
*_host_walk_slice, driven by tests/query_slices.py) run the bodies as one launch of slots [first, first + n) does: a.first = first,
slot = first + lane, the HBM spill indexed by lane, sized launch_lanes * deep_cap, shared by the launch's lanes and reused by the next
launch, tid = lane % block in one LDS stand-in.

For every slice layout (at least 3 slices, a ragged last one that is no multiple of 64), every query, float and double, default
flags, ORIGINAL_IDS and an explicit non-identity order: every output is byte-equal to the existing unsliced harness run, the slices'
counters add up to the unsliced counters, the guard zones around the spill stay intact, every slice wrote to its spill, and the known
answers of the chain hold. A slot / lane mix-up in the spill index lands in the guard zone behind the spill here, on the CPU.

The cut of SHALLOW trees at kPointMaxLaunch = 2^30 queries per launch cannot be reached at test size and is not covered."""
import numpy as np
import pytest

import instanced_scenes as sc
import query_slices as qs
import test_closest_point_host as closest_host
import test_knn_host as knn_host
import test_overlap_host as overlap_host
import test_radius_search_host as radius_host
from test_closest_point_host import chain_tree, precompute

# (depth, slots per launch); the batch is 3 launches and 37 slots more. 320 lanes: tid wraps (lane % 256), the [depth][lane] stride of
# the LDS arrays is used beyond lane 64
LAYOUTS = [(70, 320), (70, 64), (300, 320), (3000, 128)]
DTYPES = [np.float32, np.float64]
SELF_PER = {70: 32, 300: 64, 3000: 640}                        # overlap_self: n is the primitive count, depth + 1 = 71, 301, 3001


@pytest.fixture(scope="module")
def dlls(tmp_path_factory):
    d = tmp_path_factory.mktemp("query_slices")
    return qs.bind({"closest": closest_host.compile_harness(d), "radius": radius_host.compile_harness(d), "knn": knn_host.compile_harness(d),
                    "overlap": overlap_host.compile_harness(d), "instanced": sc.compile_harness(d)})


def modes(n, ids):
    """(name, order, prim ids): default flags, ORIGINAL_IDS, an explicit order that is not the identity."""
    perm = np.random.default_rng(n).permutation(n).astype(np.uint32)
    assert (perm != np.arange(n)).any()
    return [("default", None, None), ("original_ids", None, ids), ("order", perm, None)]


def _same(got, want, what):
    for j, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (what, j)


def test_chain_is_chain_tree(restatement):
    """query_slices.chain restates test_closest_point_host.chain_tree (float, depth <= 3000) node for node."""
    for depth in (65, 70, 300):
        tris, nodes, ids = chain_tree(depth, restatement.prep_tris)
        t2, n2, _ = qs.chain(depth, np.float32)
        assert tris.tobytes() == t2.tobytes() and nodes.tobytes() == n2.tobytes()
        _, stacked, _ = overlap_host.chain(depth, restatement.prep_tris, True)
        assert stacked.tobytes() == qs.chain(depth, np.float32, stacked=True)[1].tobytes()
    for depth, dtype in ((3000, np.float64), (14500, np.float32)):             # shifted: the far end stays behind the queries
        tris, nodes, bb = qs.chain(depth, dtype, stacked=True)
        assert tris[:, 0].min() >= 1000 and (np.diff(tris[:, 0]) == -1).all() and nodes["bounds"].dtype == dtype
        assert (radius_host.dfs_prim_order(nodes["index"]) == np.arange(depth, -1, -1)).all()


def test_launch_size_mirror():
    """The figures of the drivers' formula that the GPU tests size their batches by."""
    assert qs.deep_cap(3000) == 2937
    assert (qs.per_launch(3000, 8), qs.per_launch(3000, 12), qs.per_launch(3000, 4)) == (11264, 7424, 22784)
    assert qs.deep_cap(14500) == 14437 and qs.per_launch(14500, 4) == 4608 and 14501 > 3 * 4608
    assert qs.per_launch(3000, 8, n=11264) == 11264 and qs.per_launch(3000, 8, n=100) == 256
    assert qs.per_launch(10**6, 12) == 256                     # a single block needs more than the budget: one block per launch
    # knn_block_lanes: the table of DESIGN.md, "k-nearest queries"
    assert [qs.knn_block_lanes(k, 4) for k in (1, 8, 17, 9, 32, 16, 33, 64)] == [256, 256, 256, 128, 128, 64, 64, 64]
    assert [qs.knn_block_lanes(k, 8) for k in (5, 9, 7, 16, 17, 1, 8, 32, 64)] == [256, 256, 128, 128, 128, 64, 64, 64, 64]


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("depth,per", LAYOUTS)
def test_closest_points(dlls, depth, per, dtype):
    n, cap = 3 * per + 37, qs.deep_cap(depth)
    tris, nodes, _ = qs.chain(depth, dtype)
    tree = radius_host.Tree(nodes["bounds"], nodes["index"], precompute(tris, dtype), 0)
    q = qs.nearest_queries(depth, n, dtype)
    ids = qs.prim_ids(depth + 1)
    for name, order, pid in modes(n, ids):
        want, want_cnt = closest_host.host_walk(dlls["closest"], nodes["bounds"], nodes["index"], tree.prims, q, 0, order=order, prim_ids=pid,
                                                deep_cap=cap, threads=4)
        hits, run = qs.closest_sliced(dlls["closest"], tree, q, per, cap, order=order, ids=pid)
        run.check(4)
        assert hits.tobytes() == want.tobytes(), name
        assert (run.total() == want_cnt).all(), (name, run.total(), want_cnt)
        assert (hits["prim"] == (depth if pid is None else pid[depth])).all(), name          # the deepest triangle is the nearest


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("depth,per", LAYOUTS)
def test_radius_search(dlls, depth, per, dtype):
    n, cap = 3 * per + 37, qs.deep_cap(depth)
    tris, nodes, _ = qs.chain(depth, dtype, stacked=True)
    tree = radius_host.Tree(nodes["bounds"], nodes["index"], precompute(tris, dtype), 0)
    dfs = radius_host.dfs_prim_order(nodes["index"])
    q = qs.radius_queries(depth, n, dtype)
    everything = np.flatnonzero(np.isinf(q[:, 3]))
    ids = qs.prim_ids(depth + 1)
    for name, order, pid in modes(n, ids):
        want = radius_host.host_radius(dlls["radius"], tree, q, order=order, prim_ids=pid, deep_cap=cap, threads=4)
        got, count_run, fill_run = qs.radius_sliced(dlls["radius"], tree, q, per, cap, order=order, ids=pid)
        count_run.check(4)
        fill_run.check(4)
        _same(got, want, name)
        assert (count_run.total() == want[4]).all() and count_run.spill == fill_run.spill, name
        offsets, lst, _, counts, _ = got
        assert (counts[everything] == depth + 1).all() and 0 < counts.min() and np.delete(counts, everything).max() <= 12
        listed = dfs if pid is None else pid[dfs]
        for j in everything[[0, len(everything) // 2, -1]]:    # r = inf: the whole chain in the walk's depth-first order
            assert (lst[int(offsets[j]):int(offsets[j + 1])] == listed).all(), (name, j)
        assert everything[-1] >= n - 37                        # (one of them in the ragged last slice)


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("depth,per", LAYOUTS)
def test_knn(dlls, depth, per, dtype):
    n, cap = 3 * per + 37, qs.deep_cap(depth)
    tris, nodes, _ = qs.chain(depth, dtype)
    tree = radius_host.Tree(nodes["bounds"], nodes["index"], precompute(tris, dtype), 0)
    q = qs.nearest_queries(depth, n, dtype)
    finite = np.isfinite(q[:, 3])
    ids = qs.prim_ids(depth + 1)
    for k in (1, 5, 64):
        stride = qs.knn_block_lanes(k, np.dtype(dtype).itemsize)
        for name, order, pid in modes(n, ids):
            want = knn_host.host_knn(dlls["knn"], tree, q, k, order=order, prim_ids=pid, deep_cap=cap, threads=4)
            got, run = qs.knn_sliced(dlls["knn"], tree, q, k, per, cap, stride=stride, order=order, ids=pid)
            run.check(4)
            _same(got, want, (name, k))
            rows, _, counts, _ = got
            nearest = np.arange(depth, depth - k, -1)          # the k nearest: the k deepest, nearest first
            assert (rows[~finite] == (nearest if pid is None else pid[nearest])).all() and (counts[~finite] == k).all(), (name, k)
            assert (counts[finite] == min(k, 3)).all() and finite.sum() > n // 6, (name, k)


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("depth,per", LAYOUTS)
def test_overlap_boxes(dlls, depth, per, dtype):
    n, cap = 3 * per + 37, qs.deep_cap(depth)
    ids = qs.prim_ids(depth + 1)
    tree, _ = qs.box_chain(depth, dtype, ids)
    q = qs.box_queries(depth, n, dtype)
    brute = overlap_host.expected_lists(overlap_host.brute(tree.ordered_boxes(), q), tree.dfs)
    for name, order, original in [(m[0], m[1], m[2] is not None) for m in modes(n, ids)]:
        want = overlap_host.host_overlap(dlls["overlap"], tree, q, order=order, original_ids=original, deep_cap=cap, threads=4)
        got, count_run, fill_run = qs.overlap_sliced(dlls["overlap"], tree, q, per, cap, order=order, original_ids=original)
        count_run.check(4)
        fill_run.check(4)
        _same(got, want, name)
        assert (count_run.total() == want[3]).all() and count_run.spill == fill_run.spill, name
        assert (got[2] == brute[0]).all() and (got[1] == (tree.ids[brute[1]] if original else brute[1])).all(), name
        assert (got[2][::4] == depth + 1).all() and 0 < got[2][1::4].min() and got[2][1::4].max() < 16


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("depth", sorted(SELF_PER))
def test_overlap_self(dlls, depth, dtype):
    """Self mode takes its boxes from the primitive array at first + lane: the fattened chain, every 16th box as long as the chain
    (one in every slice)."""
    per, cap = SELF_PER[depth], qs.deep_cap(depth)
    ids = qs.prim_ids(depth + 1)
    tree, _ = qs.fat_chain(depth, dtype, ids, every=16)
    n_slices = len(qs.slices(tree.n, per))
    assert n_slices >= 3 and (tree.n % per) % 64 != 0
    _, (want_counts, want_ids) = overlap_host.self_expected(tree)
    for original in (False, True):
        want = overlap_host.host_overlap(dlls["overlap"], tree, None, original_ids=original, deep_cap=cap, threads=4)
        got, count_run, fill_run = qs.overlap_sliced(dlls["overlap"], tree, None, per, cap, original_ids=original)
        count_run.check(n_slices)
        fill_run.check(n_slices)
        _same(got, want, original)
        assert (count_run.total() == want[3]).all()
        assert (got[2] == want_counts).all() and (got[1] == (tree.ids[want_ids] if original else want_ids)).all()
    assert got[2].max() >= depth - 64 and int(got[0][-1]) > 5 * depth          # a box as long as the chain pairs with everything after it


def test_instanced_scenes_are_the_float_ones(dlls, restatement):
    """query_slices.chain_scene / chain_top_scene restate instanced_scenes.chain_scene / instanced_adversarial.chain_top_scene, which
    are float only: in float the same trees, matrices and rays."""
    import instanced_adversarial as ia
    for mine, theirs in ((qs.chain_scene(dlls["instanced"], restatement, 70, 96), sc.chain_scene(dlls["instanced"], restatement, 70, 96)),
                         (qs.chain_top_scene(dlls["instanced"], restatement, 70, 70, 96), ia.chain_top_scene(dlls["instanced"], restatement, 70, 70, 96)[:3])):
        (a, rays_a, cap_a), (b, rays_b, cap_b) = mine, theirs
        assert cap_a == cap_b and rays_a.tobytes() == rays_b.tobytes()
        assert a.top_nodes.tobytes() == b.top_nodes.tobytes() and (a.top_ids == b.top_ids).all() and a.world2obj.tobytes() == b.world2obj.tobytes()
        assert a.geoms[0].nodes.tobytes() == b.geoms[0].nodes.tobytes() and a.geoms[0].tris12.tobytes() == b.geoms[0].tris12.tobytes()


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("depth,per", LAYOUTS)
def test_instanced(dlls, restatement, depth, per, dtype):
    """The instanced walk has its own copy of the driver; its batch is never reordered, so there is no order to pass. Closest-hit takes
    the nearer child first and stacks one entry per level of the chain scene's geometry; any-hit never reorders, so it gets the
    geometry with every inner child on the left: it stacks one leaf per level there."""
    n = 3 * per + 37
    for any_hit, robust in ((False, True), (True, False)):
        scene, rays, cap = qs.chain_scene(dlls["instanced"], restatement, depth, n, stacked=any_hit, dtype=dtype)
        assert scene.dtype == dtype and cap == qs.deep_cap(scene.top_depth() + 1 + depth)
        for original in (False, True):
            want, want_inst, want_cnt = sc.host_walk(scene, rays, any_hit, robust, original, deep_cap=cap, threads=4)
            hits, inst, run = qs.instanced_sliced(scene, rays, any_hit, robust, per, cap, original_ids=original)
            run.check(4)
            assert hits.tobytes() == want.tobytes() and (inst == want_inst).all(), (any_hit, original)
            assert (run.total() == want_cnt).all(), (any_hit, original)
        if not any_hit:                                        # closest-hit walks the whole chain: the deepest triangle is the nearest
            deepest = hits["prim"] == scene.geoms[0].ids32[depth]                          # (about a third of the rays hit the chain)
            assert deepest[-37:].any() and deepest.sum() > n // 8


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
def test_instanced_chain_top(dlls, restatement, dtype):
    """A chain-shaped top tree of depth 70 over instances of a chain of depth 300: the marker of the two-level stack sits at height 70,
    the spill begins inside the first instance's walk. Closest-hit robust."""
    top_depth, geom_depth, per = 70, 300, 64
    n = 3 * per + 37
    scene, rays, cap = qs.chain_top_scene(dlls["instanced"], restatement, top_depth, geom_depth, n, dtype=dtype)
    assert scene.dtype == dtype and cap == qs.deep_cap(top_depth + 1 + geom_depth)
    want, want_inst, want_cnt = sc.host_walk(scene, rays, False, True, False, deep_cap=cap, threads=4)
    hits, inst, run = qs.instanced_sliced(scene, rays, False, True, per, cap)
    run.check(4)
    assert hits.tobytes() == want.tobytes() and (inst == want_inst).all() and (run.total() == want_cnt).all()
    hit = hits["prim"] != 0xFFFFFFFF
    assert hit[-37:].any() and hit.sum() > n // 8 and (inst[hit] == top_depth).mean() > 0.9
