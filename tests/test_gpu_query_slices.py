"""MI355X: batches that point_query_run (bvh_amd/csrc/point_query.h) and the instanced driver (instanced.hip) cut into several launches
because the tree is deeper than 64 levels and the HBM stack spill of a launch is bounded (256 MiB): the launches with first > 0.

Every batch here is 3 * per_launch + 37 queries, per_launch mirrored from the drivers' formula (tests/query_slices.py), and
bvh_amd_last_query_launches() must report 4 launches after every call — and 1 for a batch of per_launch — so a changed constant cannot
turn these tests into single-launch ones unnoticed. Scenes: the chain of depth 3000 (tests/query_slices.py: chain) in float and double;
for overlap_self, whose batch is the primitives, a chain of depth 14500 with fattened boxes; for the instanced walk
instanced_scenes.chain_scene and instanced_adversarial.chain_top_scene. Flags: 0, SORTED, ORIGINAL_IDS where the query takes them; counters on; every output between guard
zones. Expected: byte equality with the host harness on the whole batch (tests/cpp/*_body_host.cpp, one lane's spill), byte equality
with the device's own results for the same queries submitted in chunks of at most per_launch (the single-launch path), counters equal
to the sum over those chunks, and the chain's known answers, in the last slice too. Then closest / radius / knn from two host
threads on two streams, and a refit followed by a query on a side stream.

The cut of SHALLOW trees at kPointMaxLaunch = 2^30 queries per launch cannot be reached at test size and is not covered.
tests/test_query_slices_host.py holds the CPU tier: the same bodies under an emulated slice, with guard zones around the spill."""
import threading

import numpy as np
import pytest

import instanced_scenes as sc
import query_slices as qs
import test_closest_point_host as closest_host
import test_knn_host as knn_host
import test_overlap_host as overlap_host
import test_radius_search_host as radius_host
from test_closest_point_host import precompute
from test_gpu_overlap import _cuda, _np
from test_gpu_query_fuzz import Device, _guarded, _inner
from test_radius_search_host import GUARD, SENT_DIST, SENT_PRIM, Tree

pytestmark = pytest.mark.gpu

INVALID = 0xFFFFFFFF
ORIGINAL_IDS, SORTED, ANY_HIT, ROBUST = 8, 4, 1, 2
FLAGS = (0, SORTED, ORIGINAL_IDS)
DEPTH, SELF_DEPTH = 3000, 14500
DTYPES = [np.float32, np.float64]
DTYPE_IDS = ["float32", "float64"]
COUNTS_FILL = 0xABABABAB
HOST_THREADS = 16


@pytest.fixture(scope="module")
def dlls(tmp_path_factory):
    d = tmp_path_factory.mktemp("query_slices_gpu")
    return {"closest": closest_host.compile_harness(d), "radius": radius_host.compile_harness(d), "knn": knn_host.compile_harness(d),
            "overlap": overlap_host.compile_harness(d), "instanced": sc.compile_harness(d)}


def launches():
    from bvh_amd import _lib
    return _lib.load().bvh_amd_last_query_launches()


class Counting:
    """The library with bvh_amd_last_query_launches() noted after every call."""

    def __init__(self, lib):
        self._lib, self.launches = lib, []

    def __getattr__(self, name):
        f = getattr(self._lib, name)

        def call(*args):
            rc = f(*args)
            self.launches.append(self._lib.bvh_amd_last_query_launches())
            return rc
        return call


def device(bvh, dprims, q):
    """test_gpu_query_fuzz.Device (the C entry points, every output between guard zones) that notes the launches of its calls."""
    dev = Device(bvh, dprims, q, 0)
    dev.lib = Counting(dev.lib)
    return dev


@pytest.fixture(scope="module")
def chains():
    """(dtype, stacked) -> the chain of depth 3000 on the device: (Bvh, nodes, BVH-order PrecomputedTri, prim ids, the same in HBM)."""
    made = {}

    def get(dtype, stacked):
        import bvh_amd
        import torch
        key = (np.dtype(dtype).name, stacked)
        if key not in made:
            tris, nodes, _ = qs.chain(DEPTH, dtype, stacked)
            ids = qs.prim_ids(DEPTH + 1)
            prims = precompute(tris, dtype)
            made[key] = (bvh_amd.Bvh.from_nodes(nodes, ids), nodes, prims, ids, torch.from_numpy(prims).cuda())
        return made[key]
    return get


def sizes(entry, lanes=qs.BLOCK, bound=DEPTH):
    per = qs.per_launch(bound, entry, lanes)
    n = 3 * per + 37
    assert qs.per_launch(bound, entry, lanes, n) == per and per % 64 == 0
    return per, n


def report(what, n, per, got):
    print(f"{what}: n = {n}, per_launch = {per}, launches reported = {got}")


def same(got, want, what):
    for j, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (what, j)


# ---- closest ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_closest_points(dlls, chains, dtype):
    bvh, nodes, prims, ids, dprims = chains(dtype, False)
    per, n = sizes(4 + np.dtype(dtype).itemsize)
    cap = qs.deep_cap(DEPTH)
    q = qs.mixed_queries(DEPTH, n, dtype)
    host = {o: closest_host.host_walk(dlls["closest"], nodes["bounds"], nodes["index"], prims, q, 0, prim_ids=ids if o else None, deep_cap=cap,
                                      threads=HOST_THREADS) for o in (False, True)}
    dev = device(bvh, dprims, q)
    for flags in FLAGS:
        want, want_cnt = host[bool(flags & ORIGINAL_IDS)]
        hits, cnt = dev.closest(flags)
        assert dev.lib.launches[-1] == 4, (flags, dev.lib.launches)
        assert hits.tobytes() == want.tobytes(), flags
        assert (cnt == want_cnt).all(), (flags, cnt, want_cnt)
        parts = []
        for first, m in qs.slices(n, per):                     # the same queries, one launch per call
            part = device(bvh, dprims, q[first:first + m])
            parts.append(part.closest(flags))
            assert part.lib.launches == [1], (flags, first, part.lib.launches)
        assert np.concatenate([p[0] for p in parts]).tobytes() == hits.tobytes(), flags
        assert (np.sum([p[1] for p in parts], axis=0) == cnt).all(), flags
    report(f"closest_points {np.dtype(dtype).name}", n, per, dev.lib.launches[-1])
    hits = host[False][0]
    near = ~np.isin(np.arange(n) % 8, (3, 6))
    assert (hits["prim"][near] == 0).all() and (hits["prim"][~near] == DEPTH).all()      # the deepest triangle is the nearest
    assert (~near[-37:]).sum() >= 8


# ---- radius -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_radius_count_and_fill(dlls, chains, dtype):
    """Both passes of radius_search (test_gpu_query_fuzz.Device.radius: the count pass, then the fill pass with the lists between guard
    zones): a finite radius on most queries, +inf on every 64th (a list of all 3001 triangles in depth-first order)."""
    bvh, nodes, prims, ids, dprims = chains(dtype, True)
    per, n = sizes(4)
    cap = qs.deep_cap(DEPTH)
    q = qs.mixed_queries(DEPTH, n, dtype, lists=True)
    tree = Tree(nodes["bounds"], nodes["index"], prims, 0)
    dfs = radius_host.dfs_prim_order(nodes["index"])
    host = {o: radius_host.host_radius(dlls["radius"], tree, q, prim_ids=ids if o else None, deep_cap=cap, threads=HOST_THREADS) for o in (False, True)}
    dev = device(bvh, dprims, q)
    for flags in FLAGS:
        want = host[bool(flags & ORIGINAL_IDS)]
        got = dev.radius(flags)
        assert dev.lib.launches[-2:] == [4, 4], (flags, dev.lib.launches)                # the count pass and the fill pass
        same(got, want, flags)
        parts = []
        for first, m in qs.slices(n, per):
            part = device(bvh, dprims, q[first:first + m])
            parts.append(part.radius(flags))
            assert part.lib.launches == [1, 1], (flags, first, part.lib.launches)
        for j in (1, 2, 3):                                    # lists, distances, counts: the chunks' one after the other
            assert np.concatenate([p[j] for p in parts]).tobytes() == got[j].tobytes(), (flags, j)
        assert (np.sum([p[4] for p in parts], axis=0) == got[4]).all(), flags
    report(f"radius_search {np.dtype(dtype).name}", n, per, dev.lib.launches[-1])
    offsets, lst, _, counts, _ = host[False]
    everything = np.flatnonzero(np.isinf(q[:, 3]))
    assert (counts[everything] == DEPTH + 1).all() and everything[-1] >= n - 37 and np.delete(counts, everything).max() <= 12 and counts.min() == 1
    for j in everything[[0, len(everything) // 2, -1]]:
        assert (lst[int(offsets[j]):int(offsets[j + 1])] == dfs).all(), j


def test_radius_search_python_layer(dlls, chains):
    """bvh_amd.radius_search with max_per_query (_two_pass_lists: one pass into fixed slots) on the sliced batch."""
    import bvh_amd
    bvh, nodes, prims, ids, dprims = chains(np.float32, True)
    per, n = sizes(4)
    q = qs.mixed_queries(DEPTH, n, np.float32, lists=True)
    tree = Tree(nodes["bounds"], nodes["index"], prims, 0)
    offsets, lst, dist, counts, _ = radius_host.host_radius(dlls["radius"], tree, q, deep_cap=qs.deep_cap(DEPTH), threads=HOST_THREADS)
    k = 4
    o, i, d, c = bvh_amd.radius_search(bvh, dprims, q, max_per_query=k)
    assert launches() == 4
    assert (_np(o) == k * np.arange(n + 1)).all() and (_np(c, np.uint32) == counts).all()
    want_i, want_d = np.full((n, k), INVALID, dtype=np.uint32), np.repeat(q[:, 3:4], k, axis=1)
    for j in range(k):
        has = counts > j
        want_i[has, j], want_d[has, j] = lst[offsets[:-1][has].astype(np.int64) + j], dist[offsets[:-1][has].astype(np.int64) + j]
    assert _np(i, np.uint32).tobytes() == want_i.tobytes() and _np(d).tobytes() == want_d.tobytes()
    assert (counts > k).any() and (counts < k).any()


# ---- knn --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("k", [1, 5, 64])
def test_knn(dlls, chains, k, dtype):
    """The block, and with it the rounding of per_launch, depends on k and the scalar type (knn_block_lanes)."""
    bvh, nodes, prims, ids, dprims = chains(dtype, False)
    lanes = qs.knn_block_lanes(k, np.dtype(dtype).itemsize)
    per, n = sizes(4 + np.dtype(dtype).itemsize, lanes)
    cap = qs.deep_cap(DEPTH)
    q = qs.mixed_queries(DEPTH, n, dtype)
    tree = Tree(nodes["bounds"], nodes["index"], prims, 0)
    host = {o: knn_host.host_knn(dlls["knn"], tree, q, k, prim_ids=ids if o else None, deep_cap=cap, threads=HOST_THREADS) for o in (False, True)}
    dev = device(bvh, dprims, q)
    for flags in FLAGS:
        want = host[bool(flags & ORIGINAL_IDS)]
        got = dev.knn(k, flags)
        assert dev.lib.launches[-1] == 4, (flags, dev.lib.launches)
        same(got, want, flags)
        parts = []
        for first, m in qs.slices(n, per):
            part = device(bvh, dprims, q[first:first + m])
            parts.append(part.knn(k, flags))
            assert part.lib.launches == [1], (flags, first, part.lib.launches)
        for j in (0, 1, 2):
            assert np.concatenate([p[j] for p in parts]).tobytes() == got[j].tobytes(), (flags, j)
        assert (np.sum([p[3] for p in parts], axis=0) == got[3]).all(), flags
    report(f"knn k = {k} {np.dtype(dtype).name} ({lanes} lanes)", n, per, dev.lib.launches[-1])
    rows, _, counts, _ = host[False]
    i = np.arange(n)
    assert (rows[i % 8 == 3] == np.arange(DEPTH, DEPTH - k, -1)).all() and (counts[i % 8 == 3] == k).all()      # nearest first: the k deepest
    assert (counts[i % 8 == 6] == min(k, 3)).all() and (counts[~np.isin(i % 8, (3, 6))] == 1).all()
    assert (rows[n - 37:][(i % 8 == 3)[n - 37:]][:, 0] == DEPTH).all()


# ---- overlap ----------------------------------------------------------------------------------------------------------------------

def overlap_device(bvh, bb, queries, flags):
    """Count pass, offsets, fill pass of bvh3X_overlap_boxes (queries None: bvh3X_overlap_self), counts and list between guard zones:
    what test_overlap_host.host_overlap returns, and the launches of the two calls."""
    import bvh_amd
    import torch
    from bvh_amd import _lib
    lib = _lib.load()
    n = bvh.prim_count if queries is None else queries.shape[0]

    def call(counts, offsets, lp, cnt):
        P = lambda t, skip=0: None if t is None else t.data_ptr() + skip
        if queries is None:
            rc = getattr(lib, f"bvh{bvh._s}_overlap_self")(bvh._h, bb.data_ptr(), bb.shape[0], flags, P(counts, 4 * GUARD), P(offsets), P(lp, 4 * GUARD), P(cnt), None)
        else:
            rc = getattr(lib, f"bvh{bvh._s}_overlap_boxes")(bvh._h, bb.data_ptr(), bb.shape[0], queries.data_ptr(), n, flags, P(counts, 4 * GUARD), P(offsets),
                                                            P(lp, 4 * GUARD), P(cnt), None)
        assert rc == 0, _lib.last_error()
        return lib.bvh_amd_last_query_launches()

    c0, cnt0 = _guarded(n, COUNTS_FILL, np.uint32), torch.zeros(3, dtype=torch.int64, device="cuda")
    made = [call(c0, None, None, cnt0)]
    counts = _inner(c0, n, COUNTS_FILL, np.uint32)
    offsets = bvh_amd.offsets_from_counts(_cuda(counts))
    h_off = _np(offsets, np.uint64)
    total = int(h_off[-1])
    c1, lp, cnt = _guarded(n, COUNTS_FILL, np.uint32), _guarded(total, SENT_PRIM, np.uint32), torch.zeros(3, dtype=torch.int64, device="cuda")
    made.append(call(c1, offsets, lp, cnt))
    assert (_inner(c1, n, COUNTS_FILL, np.uint32) == counts).all() and (_np(cnt) == _np(cnt0)).all()
    return (h_off, _inner(lp, total, SENT_PRIM, np.uint32), counts, _np(cnt).astype(np.uint64)), made


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_overlap_boxes(dlls, dtype):
    import bvh_amd
    ids = qs.prim_ids(DEPTH + 1)
    tree, nodes = qs.box_chain(DEPTH, dtype, ids)
    bvh = bvh_amd.Bvh.from_nodes(nodes, ids)
    bb = _cuda(tree.bboxes)
    per, n = sizes(4)
    cap = qs.deep_cap(DEPTH)
    q = qs.mixed_boxes(DEPTH, n, dtype)
    dq = _cuda(q)
    host = {o: overlap_host.host_overlap(dlls["overlap"], tree, q, original_ids=o, deep_cap=cap, threads=HOST_THREADS) for o in (False, True)}
    for flags in FLAGS:
        want = host[bool(flags & ORIGINAL_IDS)]
        got, made = overlap_device(bvh, bb, dq, flags)
        assert made == [4, 4], (flags, made)                   # the count pass and the fill pass
        same(got, want, flags)
        parts = []
        for first, m in qs.slices(n, per):
            part, one = overlap_device(bvh, bb, dq[first:first + m], flags)
            parts.append(part)
            assert one == [1, 1], (flags, first, one)
        for j in (1, 2):
            assert np.concatenate([p[j] for p in parts]).tobytes() == got[j].tobytes(), (flags, j)
        assert (np.sum([p[3] for p in parts], axis=0) == got[3]).all(), flags
    report(f"overlap_boxes {np.dtype(dtype).name}", n, per, made[-1])
    offsets, lst, counts, _ = host[False]
    i = np.arange(n)
    assert (counts[i % 64 == 3] == DEPTH + 1).all() and (counts[~np.isin(i % 8, (3, 6))] == 1).all() and 0 < counts[i % 8 == 6].min()
    last = int(np.flatnonzero(i % 64 == 3)[-1])
    assert last >= n - 37 and (lst[int(offsets[last]):int(offsets[last + 1])] == tree.dfs).all()
    # the Python layer: one pass into max_per_query slots (_two_pass_lists)
    k = 3
    o, li, c = bvh_amd.overlap_search(bvh, bb, dq, max_per_query=k)
    assert launches() == 4
    want_l = np.full((n, k), INVALID, dtype=np.uint32)
    for j in range(k):
        has = counts > j
        want_l[has, j] = lst[offsets[:-1][has].astype(np.int64) + j]
    assert li.cpu().numpy().view(np.uint32).tobytes() == want_l.tobytes() and (c.cpu().numpy().view(np.uint32) == counts).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_overlap_self(dlls, dtype):
    """Self mode takes the box of a lane from the primitives at first + lane, and its batch is the primitives: a chain deep enough that
    depth + 1 > 3 * per_launch(depth). Its boxes are fattened so that neighbours pair, every 64th reaches to the far end and stacks a
    leaf per level from its own level on (query_slices.fat_chain). The batch cannot be submitted in chunks, so the device is compared
    with the harness (and through it, exactly, with a count of the pairs in numpy)."""
    import bvh_amd
    n = SELF_DEPTH + 1
    per = qs.per_launch(SELF_DEPTH, 4)
    assert 3 * per < n <= 4 * per and (n - 3 * per) % 64 != 0
    ids = qs.prim_ids(n)
    tree, nodes = qs.fat_chain(SELF_DEPTH, dtype, ids, whole=False)
    bvh = bvh_amd.Bvh.from_nodes(nodes, ids)
    bb = _cuda(tree.bboxes)
    cap = qs.deep_cap(SELF_DEPTH)
    for flags in (0, ORIGINAL_IDS):
        want = overlap_host.host_overlap(dlls["overlap"], tree, None, original_ids=bool(flags), deep_cap=cap, threads=HOST_THREADS)
        got, made = overlap_device(bvh, bb, None, flags)
        assert made == [4, 4], (flags, made)
        same(got, want, flags)
    report(f"overlap_self {np.dtype(dtype).name}", n, per, made[-1])
    # Box k = [x_k - 2.5, x_k + 2.5] with x_k = base - k, or from the far end to x_k + 2.5 where k = 0 mod 64. Lane k lists the i > k
    # (x_i < x_k) whose box reaches back to x_k - 2.5: the next 5 — or, from a long box, all of them.
    k = np.arange(n)
    counts = want[2]
    assert (counts == np.where(k % 64 == 0, n - 1 - k, np.minimum(5, n - 1 - k))).all() and counts[3 * per:].max() > 64


# ---- the instanced walk -----------------------------------------------------------------------------------------------------------

def instanced_device(dev, rays, flags):
    """bvh3X_intersect_rays_instanced (X from the scene's scalar type) with hits and instances between guard zones: (records, instances,
    counters, launches)."""
    import torch
    from bvh_amd import _lib, api
    lib = _lib.load()
    table, s, _, keep = api._geometry_table(dev.geoms, "test")
    n = rays.shape[0]
    dt = dev.scene.dtype
    hits, inst = _guarded(4 * n, SENT_DIST, dt), _guarded(n, COUNTS_FILL, np.uint32)
    cnt = torch.zeros(3, dtype=torch.int64, device="cuda")
    rc = getattr(lib, f"bvh{s}_intersect_rays_instanced")(dev.top._h, table, len(table), dev.world2obj.data_ptr(), None, dev.world2obj.shape[0], rays.data_ptr(), n,
                                                         flags, hits.data_ptr() + np.dtype(dt).itemsize * GUARD, inst.data_ptr() + 4 * GUARD, cnt.data_ptr(), None)
    assert rc == 0, _lib.last_error()
    made = lib.bvh_amd_last_query_launches()
    del keep
    records = _inner(hits, 4 * n, SENT_DIST, dt).view(closest_host.HITD if dt == np.float64 else closest_host.HITF).reshape(-1)
    return records, _inner(inst, n, COUNTS_FILL, np.uint32), _np(cnt).astype(np.uint64), made


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("any_hit", [False, True], ids=["closest_robust", "any_hit"])
def test_instanced(dlls, restatement, any_hit, dtype):
    """instanced.hip has its own copy of the driver, and its stack bound is depth(top) + 1 + the deepest geometry. Closest-hit robust on
    instanced_scenes.chain_scene (query_slices.chain_scene: the same in either scalar type); any-hit, which never reorders, on that
    scene with the geometry's inner children on the left, where it stacks a leaf per level. One ray in 8 goes through the chains, the others point away from
    them and end at the top tree."""
    from test_gpu_instanced import DeviceScene
    bound = 0 + 1 + DEPTH                                      # (a single-leaf top tree has depth 0)
    per, n = sizes(4, bound=bound)
    scene, rays, cap = qs.chain_scene(dlls["instanced"], restatement, DEPTH, n, stacked=any_hit, dtype=dtype)
    assert scene.dtype == dtype and scene.top_depth() == 0 and cap == qs.deep_cap(bound)
    away = np.arange(n) % 8 != 3
    rays[away, 3:6] = -rays[away, 3:6]
    dev = DeviceScene(scene)
    drays = _cuda(rays)
    mode = ANY_HIT if any_hit else ROBUST
    for flags in (mode, mode | ORIGINAL_IDS):
        want, want_inst, want_cnt = sc.host_walk(scene, rays, any_hit, not any_hit, bool(flags & ORIGINAL_IDS), deep_cap=cap, threads=HOST_THREADS)
        hits, inst, cnt, made = instanced_device(dev, drays, flags)
        assert made == 4, (flags, made)
        assert sc.same_records(hits, want) and (inst == want_inst).all() and (cnt == want_cnt).all(), (flags, cnt, want_cnt)
        parts = []
        for first, m in qs.slices(n, per):
            parts.append(instanced_device(dev, drays[first:first + m], flags))
            assert parts[-1][3] == 1, (flags, first)
        assert np.concatenate([p[0] for p in parts]).tobytes() == hits.tobytes() and (np.concatenate([p[1] for p in parts]) == inst).all(), flags
        assert (np.sum([p[2] for p in parts], axis=0) == cnt).all(), flags
    report(f"intersect_rays_instanced {'any-hit' if any_hit else 'closest-hit robust'} {np.dtype(dtype).name}", n, per, made)
    deepest = hits["prim"] == scene.geoms[0].ids32[DEPTH]
    assert deepest[-37:].any() and deepest.sum() > n // 64


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_instanced_chain_top(dlls, restatement, dtype):
    """instanced_adversarial.chain_top_scene (query_slices.chain_top_scene: the same in either scalar type): a chain-shaped top tree of depth 70 over instances of a chain of depth 1500, so the
    marker of the two-level stack sits at height 70, the spill begins inside the first instance's walk and the bound is
    70 + 1 + 1500. Closest-hit robust; one ray in 8 goes through the middle of the triangles (a ray that passed beside them would walk
    all 71 instances to the bottom), the others point away."""
    from test_gpu_instanced import DeviceScene
    top_depth, geom_depth = 70, 1500
    bound = top_depth + 1 + geom_depth
    per, n = sizes(4, bound=bound)
    scene, rays, cap = qs.chain_top_scene(dlls["instanced"], restatement, top_depth, geom_depth, n, dtype=dtype)
    assert scene.dtype == dtype and cap == qs.deep_cap(bound)
    away = np.arange(n) % 8 != 3
    rays[away, 3:6] = -rays[away, 3:6]
    rng = np.random.default_rng(n)
    rays[~away, 1], rays[~away, 2] = rng.uniform(-0.2, 0.2, int((~away).sum())), rng.uniform(-0.5, 0.0, int((~away).sum()))
    dev = DeviceScene(scene)
    drays = _cuda(rays)
    want, want_inst, want_cnt = sc.host_walk(scene, rays, False, True, False, deep_cap=cap, threads=HOST_THREADS)
    hits, inst, cnt, made = instanced_device(dev, drays, ROBUST)
    assert made == 4, made
    assert sc.same_records(hits, want) and (inst == want_inst).all() and (cnt == want_cnt).all(), (cnt, want_cnt)
    parts = []
    for first, m in qs.slices(n, per):
        parts.append(instanced_device(dev, drays[first:first + m], ROBUST))
        assert parts[-1][3] == 1, first
    assert np.concatenate([p[0] for p in parts]).tobytes() == hits.tobytes() and (np.concatenate([p[1] for p in parts]) == inst).all()
    assert (np.sum([p[2] for p in parts], axis=0) == cnt).all()
    report(f"intersect_rays_instanced chain top tree, closest-hit robust {np.dtype(dtype).name}", n, per, made)
    hit = hits["prim"] != INVALID
    assert (hit == ~away).all() and hit[-37:].any()
    assert (inst[hit] == top_depth).all() and (hits["prim"][hit] == geom_depth).all()     # the deepest instance, its deepest triangle


# ---- streams and threads ----------------------------------------------------------------------------------------------------------

def _point_rounds(bvh, dprims, dq, sort):
    """closest, radius count, radius fill and knn through the Python layer (the current torch stream), counters on. Every call is one
    launch, by the accessor of the calling thread."""
    import bvh_amd
    made = []
    hits, c0 = bvh_amd.closest_points(bvh, dprims, dq, counters=True, sort_queries=sort)
    made.append(launches())
    counts, c1 = bvh_amd.radius_count(bvh, dprims, dq, counters=True, sort_queries=sort)
    made.append(launches())
    off, ids, dist, c2 = bvh_amd.radius_search(bvh, dprims, dq, counters=True, sort_queries=sort)
    made.append(launches())
    ki, kd, kc, c3 = bvh_amd.knn(bvh, dprims, dq, 5, counters=True, sort_queries=sort)
    made.append(launches())
    assert made == [1, 1, 1, 1], made
    return hits, c0, counts, c1, off, ids, dist, c2, ki, kd, kc, c3


def _point_expected(dlls, bvh, prims, q, cap):
    nodes = bvh.nodes
    tree = Tree(nodes["bounds"], nodes["index"], prims, 0)
    hits, c0 = closest_host.host_walk(dlls["closest"], nodes["bounds"], nodes["index"], prims, q, 0, deep_cap=cap, threads=HOST_THREADS)
    off, ids, dist, counts, c1 = radius_host.host_radius(dlls["radius"], tree, q, deep_cap=cap, threads=HOST_THREADS)
    ki, kd, kc, c3 = knn_host.host_knn(dlls["knn"], tree, q, 5, deep_cap=cap, threads=HOST_THREADS)
    return hits, c0, counts, c1, off, ids, dist, c1, ki, kd, kc, c3     # (c1 twice: the count pass and the fill pass count the same)


def _equals_expected(out, want):
    import bvh_amd
    hits, c0, counts, c1, off, ids, dist, c2, ki, kd, kc, c3 = out
    got = (bvh_amd.hits_to_numpy(hits), c0, counts, c1, off, ids, dist, c2, ki.reshape(-1), kd.reshape(-1), kc, c3)
    for j, (g, w) in enumerate(zip(got, want)):
        g = g if isinstance(g, np.ndarray) else g.cpu().numpy()
        assert g.tobytes() == np.ascontiguousarray(w).reshape(-1).tobytes(), j


def _two_threads(bvh, dprims, dq):
    """Two host threads, each on a stream of its own: four rounds of every point query under SORTED and under default flags (thread 0
    begins with SORTED, thread 1 with the default). -> the results of each thread's last round under either."""
    import torch
    out, errors = [], []

    def work(k):
        try:
            stream = torch.cuda.Stream()
            mine = {}
            with torch.cuda.stream(stream):
                for _ in range(4):
                    for sort in ((True, None) if k == 0 else (None, True)):
                        mine[sort] = _point_rounds(bvh, dprims, dq, sort)
            stream.synchronize()
            out.extend(mine.values())
        except BaseException as exc:                          # noqa: BLE001 (reported by the asserting thread)
            errors.append(exc)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert len(out) == 4
    return out


def test_two_threads_two_streams_fresh_tree(dlls):
    """closest / radius / knn from two host threads on one FRESH tree: their first calls meet in tree_depth (the lazily computed depth,
    under its mutex), each has its stream's scratch and the sort scratch of query_order."""
    import bvh_amd
    import torch
    from bvh_amd import synth
    tris = synth.soup(20000)
    bb, cc = bvh_amd.tri_bounds(tris)
    bvh = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.Medium))
    dprims = bvh_amd.precompute_tris(tris, bvh.device_prim_ids())
    lo, hi = synth.scene_bounds(tris)
    q = np.zeros((4096 + 37, 4), dtype=np.float32)
    q[:, :3] = synth.points_uniform(len(q), lo, hi, seed=5)
    q[:, 3] = 0.05 * float(np.linalg.norm(hi - lo))
    q[::9, 3] = np.inf
    want = _point_expected(dlls, bvh, dprims.cpu().numpy(), q, 0)    # (reads the nodes back; no query has asked for the depth yet)
    dq = torch.from_numpy(q).cuda()
    torch.cuda.synchronize()
    for out in _two_threads(bvh, dprims, dq):
        _equals_expected(out, want)


def test_two_threads_two_streams_deep_chain(dlls, chains):
    """The same on the chain of depth 3000 with a batch of one launch per call (_point_rounds asserts it in each thread, where the
    accessor is that thread's own): each stream uses a spill of its own. The thread that asserts here has made another call last."""
    import torch
    bvh, nodes, prims, ids, dprims = chains(np.float32, False)
    n = 4096 + 37
    assert n <= qs.per_launch(DEPTH, 8)
    q = qs.mixed_queries(DEPTH, n, np.float32, lists=True)
    want = _point_expected(dlls, bvh, prims, q, qs.deep_cap(DEPTH))
    dq = torch.from_numpy(q).cuda()
    torch.cuda.synchronize()
    sliced = device(bvh, dprims, qs.mixed_queries(DEPTH, 2 * qs.per_launch(DEPTH, 8) + 37, np.float32))
    sliced.closest(0)
    assert sliced.lib.launches == [3]                          # this thread's latest query: the workers' calls do not show here
    for out in _two_threads(bvh, dprims, dq):
        _equals_expected(out, want)
    assert launches() == 3


def test_refit_then_sorted_query_on_a_side_stream(dlls):
    """refit_tris and a SORTED closest query issued back to back on a side stream (the sort keys are scaled by the root box the refit
    has just rewritten) equal the query on a fresh upload of the refitted tree."""
    import bvh_amd
    import torch
    from bvh_amd import synth
    tris = synth.soup(20000)
    moved = (tris * np.float32(1.5) + np.float32(0.25)).astype(np.float32)
    bb, cc = bvh_amd.tri_bounds(tris)
    bvh = bvh_amd.DefaultBuilder.build(bb, cc)
    twin = bvh_amd.Bvh.deserialize(bvh.serialize())
    lo, hi = synth.scene_bounds(moved)
    q = np.zeros((4096 + 37, 4), dtype=np.float32)
    q[:, :3] = synth.points_uniform(len(q), lo, hi, seed=6)
    q[:, 3] = np.inf
    dq, dmoved = torch.from_numpy(q).cuda(), torch.from_numpy(moved).cuda()
    # the expected tree: the twin refitted on the default stream, read back, uploaded afresh
    twin_prims = twin.refit_tris(dmoved)
    torch.cuda.synchronize()
    nodes, ids = twin.nodes, twin.prim_ids
    fresh = bvh_amd.Bvh.from_nodes(nodes, ids)
    want = bvh_amd.hits_to_numpy(bvh_amd.closest_points(fresh, twin_prims, dq, sort_queries=False))
    host, _ = closest_host.host_walk(dlls["closest"], nodes["bounds"], nodes["index"], twin_prims.cpu().numpy(), q, 0, threads=HOST_THREADS)
    assert want.tobytes() == host.tobytes()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dprims = bvh.refit_tris(dmoved)
        hits = bvh_amd.closest_points(bvh, dprims, dq, sort_queries=True)
    stream.synchronize()
    assert bvh_amd.hits_to_numpy(hits).tobytes() == want.tobytes()
    assert (want["prim"] != INVALID).all()


# ---- the mesh queries: sphere_cast, tri_distance, region ------------------------------------------------------------------------------
# Their spill is indexed by the lane of the launch like that of the point queries. Expected: byte equality with the device's own
# results for the same queries submitted one launch per call, counters summed; byte equality with the host harness on every 15th
# query (the harness walks one query at a time: a sixteenth of 3 * per_launch queries over 3000 levels is about what a test can
# afford, and 15 shares no factor with the periods of the batches below, so every kind of query is among those compared).
SAMPLE = 15

MESH_FLAGS = {"sphere_cast": (0, SORTED | ROBUST, ORIGINAL_IDS), "tri_distance": (0, SORTED, ORIGINAL_IDS), "region": (0, 64, ORIGINAL_IDS)}


def mesh_device(bvh, dtype):
    """test_gpu_mesh_query_fuzz.Device (the C entry points, every output between guard zones) that notes the launches of its calls."""
    from test_gpu_mesh_query_fuzz import Device as MeshDevice
    dev = MeshDevice(bvh, dtype)
    dev.lib = Counting(dev.lib)
    return dev


@pytest.fixture(scope="module")
def mesh_dlls(tmp_path_factory):
    import region_ref
    import test_sphere_cast_host as cast_host
    import test_tri_distance_host as dist_host
    d = tmp_path_factory.mktemp("mesh_query_slices_gpu")
    return {"cast": cast_host.compile_harness(d), "distance": dist_host.compile_harness(d), "region": region_ref.compile_harness(d)}


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_sphere_cast(mesh_dlls, chains, dtype):
    import test_sphere_cast_host as cast_host
    bvh, nodes, prims, ids, dprims = chains(dtype, False)
    per, n = sizes(qs.mesh_entry("sphere_cast", np.dtype(dtype).itemsize))
    cap = qs.deep_cap(DEPTH)
    rays, radii = qs.cast_rays(DEPTH, n, dtype)
    for flags in MESH_FLAGS["sphere_cast"]:
        dev = mesh_device(bvh, dtype)
        hits, cnt = dev.cast(dprims, 0, rays, radii, flags)
        assert dev.lib.launches == [4], (flags, dev.lib.launches)
        parts = []
        for first, m in qs.slices(n, per):                     # the same rays, one launch per call
            part = mesh_device(bvh, dtype)
            parts.append(part.cast(dprims, 0, rays[first:first + m], radii[first:first + m], flags))
            assert part.lib.launches == [1], (flags, first, part.lib.launches)
        assert np.concatenate([p[0] for p in parts]).tobytes() == hits.tobytes(), flags
        assert (np.sum([p[1] for p in parts], axis=0) == cnt).all(), flags
        want, _ = cast_host.host_walk(mesh_dlls["cast"], nodes["bounds"], nodes["index"], prims, rays[::SAMPLE], radii[::SAMPLE], 0, robust=bool(flags & ROBUST),
                                      prim_ids=ids if flags & ORIGINAL_IDS else None, deep_cap=cap, threads=HOST_THREADS)
        assert hits[::SAMPLE].tobytes() == want.tobytes(), flags
        if flags == 0:
            i = np.arange(n)
            through = (i % 7 != 0) & (i % 11 != 0)
            ball = through & (radii > 0)                       # (a bare ray at |y| = 0.5, z = 0.5 passes beside every triangle)
            assert (hits["prim"][ball] == DEPTH).all() and (hits["prim"][~through] == INVALID).all()         # the deepest triangle is the first one met
            assert np.isin(hits["prim"], (DEPTH, INVALID)).all() and ball[-37:].sum() >= 8
    report(f"sphere_cast {np.dtype(dtype).name}", n, per, dev.lib.launches[-1])


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_tri_distance(mesh_dlls, dtype):
    import test_tri_distance_host as dist_host
    import tri_intersect_ref as TR
    from test_gpu_tri_distance import device_tree
    tree = TR.chain_tree(DEPTH, dtype, stacked=True, ids=qs.prim_ids(DEPTH + 1))
    bvh = device_tree(tree)
    dtris = _cuda(tree.tris)
    per, n = sizes(qs.mesh_entry("tri_distance", np.dtype(dtype).itemsize))
    cap = qs.deep_cap(DEPTH)
    q = dist_host.chain_queries(DEPTH, n).astype(dtype)
    lim = np.where(np.arange(n) % 3 == 0, 2.0, np.inf).astype(dtype)
    for flags in MESH_FLAGS["tri_distance"]:
        dev = mesh_device(bvh, dtype)
        hits, uv, cnt = dev.distance(dtris, q, lim, flags)
        assert dev.lib.launches == [4], (flags, dev.lib.launches)
        parts = []
        for first, m in qs.slices(n, per):
            part = mesh_device(bvh, dtype)
            parts.append(part.distance(dtris, q[first:first + m], lim[first:first + m], flags))
            assert part.lib.launches == [1], (flags, first, part.lib.launches)
        assert np.concatenate([p[0] for p in parts]).tobytes() == hits.tobytes() and np.concatenate([p[1] for p in parts]).tobytes() == uv.tobytes(), flags
        assert (np.sum([p[2] for p in parts], axis=0) == cnt).all(), flags
        want, want_uv, _ = dist_host.host_walk(mesh_dlls["distance"], tree, q[::SAMPLE], lim[::SAMPLE], original_ids=bool(flags & ORIGINAL_IDS), deep_cap=cap,
                                               threads=HOST_THREADS)
        assert hits[::SAMPLE].tobytes() == want.tobytes() and uv[::SAMPLE].tobytes() == want_uv.tobytes(), flags
        if flags == 0:
            assert (hits["t"][::4] == 0).all() and (hits["prim"][::4] == 0).all()        # the sliver crosses every level: the lowest index wins
            assert (hits["t"][-37:] > 0).sum() >= 8
    report(f"tri_distance {np.dtype(dtype).name}", n, per, dev.lib.launches[-1])


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_region(mesh_dlls, dtype):
    """The count pass and the fill pass (lists and inside bytes between guard zones: test_gpu_mesh_query_fuzz.Device.region)."""
    import region_ref
    import tri_intersect_ref as TR
    from test_gpu_region import device_tree
    t = TR.chain_tree(DEPTH, dtype, stacked=True, ids=qs.prim_ids(DEPTH + 1))
    tree = region_ref.PrimTree(t.bounds, t.index, t.tris, t.ids)
    bvh = device_tree(tree)
    dprims = _cuda(tree.prims)
    per, n = sizes(qs.mesh_entry("region", np.dtype(dtype).itemsize))
    cap = qs.deep_cap(DEPTH)
    planes = qs.region_planes(DEPTH, n, dtype)
    for flags in MESH_FLAGS["region"]:
        dev = mesh_device(bvh, dtype)
        offsets, lst, ins, counts, cnt = dev.region(dprims, 0, planes, flags)
        assert dev.lib.launches == [4, 4], (flags, dev.lib.launches)                     # the count pass and the fill pass
        parts = []
        for first, m in qs.slices(n, per):
            part = mesh_device(bvh, dtype)
            parts.append(part.region(dprims, 0, planes[first:first + m], flags))
            assert part.lib.launches == [1, 1], (flags, first, part.lib.launches)
        for j, whole in ((1, lst), (2, ins), (3, counts)):
            assert np.concatenate([p[j] for p in parts]).tobytes() == whole.tobytes(), (flags, j)
        assert (np.sum([p[4] for p in parts], axis=0) == cnt).all(), flags
        h_off, h_lst, h_ins, h_counts, _ = region_ref.host_region(mesh_dlls["region"], tree, planes[::SAMPLE], exact=bool(flags & 64),
                                                                  original_ids=bool(flags & ORIGINAL_IDS), deep_cap=cap, threads=HOST_THREADS)
        assert (counts[::SAMPLE] == h_counts).all(), flags
        pick = np.concatenate([np.arange(int(offsets[k]), int(offsets[k + 1])) for k in range(0, n, SAMPLE)]).astype(np.int64)
        assert lst[pick].tobytes() == h_lst.tobytes() and ins[pick].tobytes() == h_ins.tobytes(), flags
        if flags == 0:
            i = np.arange(n)
            everything, nothing = i % 64 == 3, (i % 5 == 0) & (i % 64 != 3)
            assert (counts[everything] == DEPTH + 1).all() and (counts[nothing] == 0).all() and np.flatnonzero(everything)[-1] >= n - 37
            assert 0 < counts[~everything & ~nothing].min() and counts[~everything].max() < 16
    report(f"region {np.dtype(dtype).name}", n, per, dev.lib.launches[-1])
