"""Shared by tests/test_query_slices_host.py (CPU) and tests/test_gpu_query_slices.py (-m gpu): the launches that point_query_run
(bvh_amd/csrc/point_query.h) and the instanced driver (instanced.hip) cut a batch into when the tree is deeper than 64 levels.

Here: the mirror of the drivers' launch size, chain-shaped trees of any depth in float and double, the batches the sliced tests walk,
and the harnesses' slice entries (tests/cpp/*_body_host.cpp: *_host_walk_slice) driven slice after slice over one set of output
buffers, as the device does. A slice entry emulates ONE launch of slots [first, first + n): slot = first + lane, the spill indexed by
lane and sized for the launch, between guard zones."""
import ctypes as C

import numpy as np

import instanced_scenes as sc
import oracle
import test_overlap_host as overlap_host
import test_radius_search_host as radius_host
from test_kernel_body_host import _aligned, pair_records
from test_radius_search_host import GUARD, SENT_DIST, SENT_PRIM

# point_query.h / point_walk.inc / trace_device.h: the spill's budget, the stack entries kept on the chip, the block, the launch cap
DEEP_BYTES, POINT_SMALL, BLOCK, MAX_LAUNCH = 256 << 20, 64, 256, 1 << 30
KNN_LDS = 8                                                    # knn_body.inc: kKnnLds
_P, _Z, _I, _U, _LL = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_longlong


def deep_cap(bound):
    """HBM stack entries per lane for a stack bound (a tree's depth; for the instanced walk depth(top) + 1 + the deepest geometry)."""
    assert bound > POINT_SMALL
    return bound - POINT_SMALL + 1


def per_launch(bound, entry, lanes=BLOCK, n=None):
    """Queries per launch as the drivers compute it: `entry` bytes per stack entry (4 for radius, overlap and the instanced walk,
    4 + sizeof(T) for closest and knn), blocks of `lanes`."""
    per = max(lanes, DEEP_BYTES // (deep_cap(bound) * entry) // lanes * lanes)
    if n is not None:
        per = min(per, (min(n, MAX_LAUNCH) + lanes - 1) // lanes * lanes)
    return per


def knn_block_lanes(k, scalar_bytes):
    """knn.hip, knn_block_lanes ("k-nearest queries", has the table): of 256 / 128 / 64 lanes the block that keeps the most
    lanes resident on a CU, ties to the larger."""
    best, best_resident = 64, 0
    for lanes in (256, 128, 64):
        nbytes = (k + KNN_LDS) * lanes * (scalar_bytes + 4)
        if nbytes > (64 << 10):
            continue
        resident = min((160 << 10) // nbytes * lanes, 8 * 4 * 64)
        if resident > best_resident:
            best, best_resident = lanes, resident
    return best


def slices(n, per):
    return [(first, min(per, n - first)) for first in range(0, n, per)]


def mesh_entry(query, scalar_bytes):
    """Bytes per spilled stack entry of the mesh queries, as their drivers hand it to point_query_run: sphere_cast.hip and
    tri_distance.hip keep the key beside the node (sizeof(uint32_t) + sizeof(T): nearest_walk.inc), region.hip the node alone."""
    return {"sphere_cast": 4 + scalar_bytes, "tri_distance": 4 + scalar_bytes, "region": 4}[query]


# ---- scenes -----------------------------------------------------------------------------------------------------------------------

def chain_base(depth):
    """x of the first triangle: test_closest_point_host.chain_tree's 4000, shifted for deeper chains so that the far end (x = base -
    depth >= 1000) stays behind the queries (x < 100)."""
    return max(4000, depth + 1000)


def chain(depth, dtype=np.float32, stacked=False):
    """test_closest_point_host.chain_tree in either scalar type and at any depth: depth + 1 triangles at x = base - k, node 2k + 1 the
    leaf of triangle k, node 2k + 2 the rest of the chain; a query in front walks to the deepest leaf first and stacks one entry per
    level. stacked: every inner child on the left (test_overlap_host.chain), so that the left-first list walks stack one leaf per
    level too. -> (tris (n, 9), nodes, boxes {min.xyz, max.xyz} of the triangles)."""
    n = depth + 1
    tris = np.zeros((n, 9), dtype=dtype)
    x = (chain_base(depth) - np.arange(n)).astype(dtype)
    tris[:, 0] = tris[:, 3] = tris[:, 6] = x
    tris[:, 1], tris[:, 2], tris[:, 4], tris[:, 5], tris[:, 7], tris[:, 8] = -1, -1, 1, -1, 0, 1
    bb = overlap_host.prim_boxes(tris)
    return tris, chain_nodes(bb, stacked), bb


def chain_nodes(bb, stacked=False):
    """The chain-shaped tree over the boxes bb ((n, 6) {min.xyz, max.xyz}, n >= 2) in their order, in bb's scalar type: node 2k + 1 the
    leaf of box k, node 2k + 2 the rest of the chain (stacked: the other way round), every box the union of what is below it."""
    n = len(bb)
    suffix = bb.copy()
    suffix[:, :3] = np.minimum.accumulate(bb[::-1, :3])[::-1]
    suffix[:, 3:] = np.maximum.accumulate(bb[::-1, 3:])[::-1]
    box = lambda b: np.stack([b[:, 0], b[:, 3], b[:, 1], b[:, 4], b[:, 2], b[:, 5]], axis=1)
    nodes = np.zeros(2 * n - 1, dtype=oracle.NODED if bb.dtype == np.float64 else oracle.NODEF)
    k = np.arange(n - 1)
    nodes["bounds"][0], nodes["index"][0] = box(suffix[:1])[0], 1 << 4
    nodes["bounds"][2 * k + 1], nodes["index"][2 * k + 1] = box(bb[:n - 1]), (k << 4) | 1
    nodes["bounds"][2 * k + 2], nodes["index"][2 * k + 2] = box(suffix[1:]), (2 * k + 3) << 4
    nodes["index"][2 * n - 2] = ((n - 1) << 4) | 1             # (suffix[n - 1] is the last box itself)
    if stacked:
        nodes[1::2], nodes[2::2] = nodes[2::2].copy(), nodes[1::2].copy()
    return nodes


def prim_ids(n, seed=7):
    """BVH-order index -> original id: a permutation that is not the identity, so that ORIGINAL_IDS shows."""
    return np.random.default_rng(seed).permutation(n).astype(np.uint32)


def point_queries(depth, n, dtype, finite, radius):
    """test_closest_point_host.chain_queries ({x in [0, 100), |y|, |z| < 0.75, +inf}) with a finite radius, `radius` beyond the far end of
    the chain, on the queries of the mask `finite`. Within base - depth + 2.5 lie the last 3 triangles (the y, z offset adds less than
    0.01 at a distance of 900 or more), within + 10.5 the last 11."""
    rng = np.random.default_rng(depth)
    q = np.zeros((n, 4), dtype=dtype)
    q[:, 0] = rng.random(n) * 100
    q[:, 1:3] = (rng.random((n, 2)) - 0.5) * 1.5
    q[:, 3] = np.inf
    q[finite, 3] = (chain_base(depth) - depth + radius) - q[finite, 0]
    return q


def nearest_queries(depth, n, dtype):
    """For closest and knn: every 5th query with the radius that reaches 3 triangles (it stacks next to nothing), the others +inf (one
    entry per level)."""
    return point_queries(depth, n, dtype, np.arange(n) % 5 == 2, 2.5)


def radius_queries(depth, n, dtype):
    """For radius: +inf on every 8th query (the whole chain in depth-first order, one stacked leaf per level on the stacked chain), the
    radius that reaches the last 11 triangles on the others."""
    return point_queries(depth, n, dtype, np.arange(n) % 8 != 3, 10.5)


def box_queries(depth, n, dtype):
    """test_overlap_host.chain_boxes on the shifted chain: every 4th box covers every level, the others the far end only."""
    rng = np.random.default_rng(depth)
    far = chain_base(depth) - depth
    q = np.zeros((n, 6), dtype=dtype)
    q[:, 0] = far - 1 - rng.random(n)
    q[:, 3] = far + 10 * rng.random(n)
    q[::4, 3] = chain_base(depth) + 1
    q[:, 1:3] = -1.5 * rng.random((n, 2))
    q[:, 4:6] = 1.5 * rng.random((n, 2))
    return q


def mixed_queries(depth, n, dtype, lists=False):
    """The point batch of the device tests, where n * depth is what a test costs. Of every 8 queries: one in front of the chain with
    r = +inf (index 3 mod 8: the whole chain, one stack entry per level for closest and knn and, on the stacked chain, for radius),
    one in front with the radius that reaches the last 3 triangles (6 mod 8: the whole chain walked, next to nothing stacked), six
    just beyond the NEAR end with a radius that reaches triangle 0 alone (they are done after one record).
    lists: +inf only at 3 mod 64 (such a list has depth + 1 entries), the other 3 mod 8 reach the last 11 triangles."""
    q = point_queries(depth, n, dtype, np.arange(n) % 8 == 6, 2.5)
    i = np.arange(n)
    if lists:
        some = (i % 8 == 3) & (i % 64 != 3)
        q[some, 3] = (chain_base(depth) - depth + 10.5) - q[some, 0]
    near = ~np.isin(i % 8, (3, 6))
    rng = np.random.default_rng(depth + 1)
    q[near, 0] = chain_base(depth) + 1 + 4 * rng.random(int(near.sum()))
    q[near, 3] = (q[near, 0] - chain_base(depth)) + 0.75        # triangle 0 is within x - base + 0.6, triangle 1 a whole unit farther
    return q


def mixed_boxes(depth, n, dtype):
    """The box batch of the device tests: box_queries with the boxes that cover every level at 3 mod 64 only, the far end alone at
    the other 3 mod 8 and at 6 mod 8 (the whole chain walked, nothing stacked), and everywhere else a box at the near end that
    overlaps triangle 0 alone."""
    q = box_queries(depth, n, dtype)
    i = np.arange(n)
    far = chain_base(depth) - depth
    rng = np.random.default_rng(depth + 2)
    q[:, 3] = far + 10 * rng.random(n)
    q[i % 64 == 3, 3] = chain_base(depth) + 1
    near = ~np.isin(i % 8, (3, 6))
    q[near, 0], q[near, 3] = chain_base(depth) - 0.25, chain_base(depth) + 1
    return q


def cast_rays(depth, n, dtype):
    """For sphere_cast over `chain`: balls flying along +x from x in [0, 100) towards the far end of the chain (they enter the rest of
    the chain before each level's leaf and stack one entry per level; the deepest triangle is the first one met), radius 0.25 or 0;
    every 7th passes 5 units beside the chain (it fails the root's boxes), every 11th ends at tmax = 10, far short of it.
    -> (rays (n, 8), radii (n,))."""
    rng = np.random.default_rng(depth + 3)
    r = np.zeros((n, 8), dtype=dtype)
    r[:, 0] = rng.integers(0, 100, n)
    r[:, 1:3] = rng.integers(-2, 3, (n, 2)) / 4.0
    r[:, 3], r[:, 7] = 1.0, np.inf
    r[::7, 1] = 5.0
    r[::11, 7] = 10.0
    radii = np.where(np.arange(n) % 3 == 0, 0.0, 0.25).astype(dtype)
    return r, radii


def region_planes(depth, n, dtype):
    """For the region queries over tri_intersect_ref.chain_tree (stacked): z <= -0.5 cuts every triangle of the chain; a second plane
    x <= the far end + a little keeps a few levels, and every 64th region has none: every level (a list of depth + 1 entries, one
    stacked leaf per level). Every other 5th region is x <= 1: nothing. -> (n, 2, 4)."""
    rng = np.random.default_rng(depth + 4)
    planes = np.zeros((n, 2, 4), dtype=dtype)
    planes[:, 0] = [0, 0, 1, 0.5]
    planes[:, 1, 0] = 1
    planes[:, 1, 3] = -(chain_base(depth) - depth + 10 * rng.random(n))
    planes[::5, 1, 3] = -1.0
    planes[3::64, 1] = [0, 0, 0, 0]
    return planes


def box_chain(depth, dtype, ids):
    """The stacked chain as test_overlap_host.Tree over the triangles' boxes (test_overlap_host.chain), its boxes stored by the
    original ids `ids`. -> (Tree, nodes)."""
    _, nodes, bb = chain(depth, dtype, stacked=True)
    by_id = np.zeros_like(bb)
    by_id[ids.astype(np.int64)] = bb
    return overlap_host.Tree(nodes["bounds"], nodes["index"], by_id, ids), nodes


def fat_chain(depth, dtype, ids, reach=2.5, every=64, whole=True):
    """The stacked chain as an overlap Tree whose boxes (and the nodes' with them) are fattened by `reach` in x, so that box k overlaps
    the 2 * reach neighbours on either side, and every `every`-th by the whole chain's length: such a box overlaps every level, and in self
    mode its lane stacks one leaf per level. whole=False: the long boxes reach from their own place to the far end only, so that the
    box of the rest of the chain below level j ends where triangle j's does: lane k then leaves the chain after k + 2 * reach levels
    instead of walking all of it, and a long box k still stacks one leaf per level from its own level on.
    Refitted bottom-up, so the tree fits the boxes. -> (Tree, nodes)."""
    _, _, bb = chain(depth, dtype, stacked=True)
    bb = bb.copy()
    bb[:, 0] -= reach
    bb[:, 3] += reach
    bb[::every, 0] = chain_base(depth) - depth - 1
    if whole:
        bb[::every, 3] = chain_base(depth) + 1
    nodes = chain_nodes(bb, stacked=True)
    by_id = np.zeros_like(bb)
    by_id[ids.astype(np.int64)] = bb                           # the harness and the C ABI take the boxes by ORIGINAL id
    return overlap_host.Tree(nodes["bounds"], nodes["index"], by_id, ids), nodes


def chain_scene(dll, orc, depth, n_rays, stacked=False, dtype=np.float32):
    """instanced_scenes.chain_scene in either scalar type (in float it is that scene, array for array): three instances of the chain
    under a single-leaf top tree, rays from in front of the triangles, ray k starting in the object space of instance k % 3.
    stacked: the geometry with every inner child on the left, which is where a walk that never reorders (any-hit) stacks one leaf per
    level. -> (scene, rays, deep_cap as instanced.hip derives it: depth(top) + 1 + depth(geometry) - 64 + 1)."""
    tris, nodes, _ = chain(depth, dtype, stacked)
    rng = np.random.default_rng(depth)
    geom = sc.Geometry(orc, tris, nodes, np.arange(depth + 1, dtype=np.uint64))
    m = np.array([np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).reshape(12), sc.affine(rng, (0.0, 30.0, 0.0), (0.9, 1.1)),
                  sc.affine(rng, (0.0, -40.0, 10.0), (0.9, 1.1))])
    scene = sc.Scene(dll, [geom], m.astype(dtype), None).single_leaf_top()
    q = point_queries(depth, n_rays, np.float32, np.zeros(n_rays, dtype=bool), 0).astype(np.float64)        # (chain_queries' own draw)
    dirs = np.stack([np.full(n_rays, 1.0), rng.uniform(-1e-4, 1e-4, n_rays) + 2e-4, rng.uniform(-1e-4, 1e-4, n_rays) - 2e-4], axis=1)
    rays = np.zeros((n_rays, 8), dtype=dtype)
    for j in range(3):                                         # ray k starts in the object space of instance k % 3
        a = m[j].reshape(3, 4)
        rays[j::3, 0:3], rays[j::3, 3:6] = q[j::3, :3] @ a[:, :3].T + a[:, 3], dirs[j::3] @ a[:, :3].T
    rays[:, 7] = np.inf
    assert not (rays[:, 3:6] == 0).any()
    return scene, rays, deep_cap(scene.top_depth() + 1 + depth)


def chain_top_scene(dll, orc, top_depth, geom_depth, n_rays, dtype=np.float32):
    """instanced_adversarial.chain_top_scene in either scalar type: the chain as the geometry (depth geom_depth, its triangles shifted
    to x in [0, geom_depth]) and as the top tree over top_depth + 1 instances, instance k at x = X - k with the geometry squeezed into
    half a unit of x; rays from x < 0 going +x, so closest-hit stacks top_depth top leaves, the marker, then geom_depth entries.
    -> (scene, rays, deep_cap)."""
    tris, _, _ = chain(geom_depth, dtype)
    tris[:, 0::3] -= dtype(chain_base(geom_depth) - geom_depth)    # (integers: exact)
    geom = sc.Geometry(orc, tris, chain_nodes(overlap_host.prim_boxes(tris)), np.arange(geom_depth + 1, dtype=np.uint64))
    n = top_depth + 1
    m = np.zeros((n, 3, 4))
    m[:, 0, 0], m[:, 1, 1], m[:, 2, 2] = 0.5 / geom_depth, 1.0, 1.0
    m[:, 0, 3] = (n + 4) - np.arange(n)
    scene = sc.Scene(dll, [geom], m.reshape(n, 12).astype(dtype), None)
    scene.top_nodes, scene.top_ids = chain_nodes(scene.bboxes), np.arange(n, dtype=np.uint64)
    assert scene.top_depth() == top_depth
    rng = np.random.default_rng(1000 * top_depth + geom_depth)
    rays = np.zeros((n_rays, 8), dtype=dtype)
    rays[:, 0] = -1.0 - 99.0 * rng.random(n_rays)
    rays[:, 1:3] = (rng.random((n_rays, 2)) - 0.5) * 1.2
    rays[:, 3], rays[:, 4], rays[:, 5] = 1.0, 2e-4 + rng.uniform(-1e-4, 1e-4, n_rays), -2e-4 + rng.uniform(-1e-4, 1e-4, n_rays)
    rays[:, 7] = np.inf
    return scene, rays, deep_cap(top_depth + 1 + geom_depth)


# ---- the harnesses' slice entries -----------------------------------------------------------------------------------------------------

def bind(dlls):
    """argtypes of the *_host_walk_slice entries of the harnesses in `dlls` ({"closest" / "radius" / "knn" / "overlap" / "instanced": CDLL})."""
    sigs = {"closest": [_I, _I, _P, _U, _P, _P, _Z, _Z, _Z, _P, _P, _U, _P, _P],
            "radius": [_I, _I, _P, _U, _P, _P, _Z, _Z, _Z, _P, _P, _U, _P, _P, _P, _P, _P],
            "knn": [_I, _I, _P, _U, _P, _P, _Z, _Z, _Z, _U, _U, _P, _P, _U, _P, _P, _P, _P],
            "overlap": [_I, _P, _U, _P, _P, _P, _Z, _Z, _Z, _P, _I, _U, _P, _P, _P, _P],
            "instanced": [_I, _P, _U, _P, _U, _P, _P, _P, _P, _P, _P, _P, _Z, _Z, _Z, _I, _I, _I, _U, _P, _P, _P]}
    for kind, dll in dlls.items():
        f = getattr(dll, f"{kind}_host_walk_slice")
        f.restype, f.argtypes = _LL, sigs[kind]
    return dlls


def _p(a):
    return None if a is None else a.ctypes.data_as(_P)


def _u32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.uint32)


class Sliced:
    """What a sliced run leaves beside its outputs: per slice the spill entries it overwrote (negative: the harness saw a guard zone
    written to) and its counters."""

    def __init__(self):
        self.spill, self.counters = [], []

    def add(self, rc, cnt):
        self.spill.append(int(rc))
        self.counters.append(cnt.copy())

    def total(self):
        return np.sum(self.counters, axis=0).astype(np.uint64)

    def check(self, n_slices):
        """The guard zones stayed intact and every slice used its spill."""
        assert len(self.spill) == n_slices >= 3, self.spill
        assert min(self.spill) > 0, self.spill


def closest_sliced(dll, tree, queries, per, cap, order=None, ids=None, lanes=None):
    """closest_points over the slices of `per` slots: (hit records, Sliced). tree: a test_radius_search_host.Tree."""
    from test_closest_point_host import HITD, HITF
    q = _aligned(np.ascontiguousarray(queries, dtype=tree.dtype))
    hits = np.zeros(len(q), dtype=HITD if tree.double else HITF)
    order, ids, run = _u32(order), _u32(ids), Sliced()
    for first, n in slices(len(q), per):
        cnt = np.zeros(3, dtype=np.uint64)
        run.add(dll.closest_host_walk_slice(int(tree.double), tree.leaf, _p(tree.pairs), tree.root, _p(tree.prims), _p(q), first, n, lanes or per,
                                            _p(order), _p(ids), cap, _p(hits), _p(cnt)), cnt)
    return hits, run


def _radius_pass(dll, tree, q, per, cap, order, ids, counts, offsets, lp, ld, lanes):
    run = Sliced()
    for first, n in slices(len(q), per):
        cnt = np.zeros(3, dtype=np.uint64)
        run.add(dll.radius_host_walk_slice(int(tree.double), tree.leaf, _p(tree.pairs), tree.root, _p(tree.prims), _p(q), first, n, lanes or per,
                                           _p(order), _p(ids), cap, _p(counts), _p(offsets), None if lp is None else lp[GUARD:].ctypes.data_as(_P),
                                           None if ld is None else ld[GUARD:].ctypes.data_as(_P), _p(cnt)), cnt)
    return run


def radius_sliced(dll, tree, queries, per, cap, order=None, ids=None, lanes=None):
    """Count pass, offsets, fill pass, each over the slices of `per` slots and one set of buffers: what
    test_radius_search_host.host_radius returns, then the Sliced of the count pass and of the fill pass."""
    q = _aligned(np.ascontiguousarray(queries, dtype=tree.dtype))
    order, ids = _u32(order), _u32(ids)
    counts = np.full(len(q), 0xABABABAB, dtype=np.uint32)
    count_run = _radius_pass(dll, tree, q, per, cap, order, ids, counts, None, None, None, lanes)
    offsets = np.concatenate([[0], np.cumsum(counts.astype(np.uint64))]).astype(np.uint64)
    total = int(offsets[-1])
    c2 = np.full(len(q), 0xABABABAB, dtype=np.uint32)
    lp, ld = np.full(total + 2 * GUARD, SENT_PRIM, dtype=np.uint32), np.full(total + 2 * GUARD, SENT_DIST, dtype=tree.dtype)
    fill_run = _radius_pass(dll, tree, q, per, cap, order, ids, c2, offsets, lp, ld, lanes)
    assert (c2 == counts).all() and radius_host.guards_intact(lp, total, ld)
    return (offsets, lp[GUARD:GUARD + total], ld[GUARD:GUARD + total], counts, fill_run.total()), count_run, fill_run


def knn_sliced(dll, tree, queries, k, per, cap, stride=BLOCK, order=None, ids=None, lanes=None):
    """knn over the slices of `per` slots: (what test_knn_host.host_knn returns, Sliced)."""
    q = _aligned(np.ascontiguousarray(queries, dtype=tree.dtype))
    n_all = len(q)
    order, ids, run = _u32(order), _u32(ids), Sliced()
    counts = np.full(n_all, 0xABABABAB, dtype=np.uint32)
    op, od = np.full(n_all * k + 2 * GUARD, SENT_PRIM, dtype=np.uint32), np.full(n_all * k + 2 * GUARD, SENT_DIST, dtype=tree.dtype)
    for first, n in slices(n_all, per):
        cnt = np.zeros(3, dtype=np.uint64)
        run.add(dll.knn_host_walk_slice(int(tree.double), tree.leaf, _p(tree.pairs), tree.root, _p(tree.prims), _p(q), first, n, lanes or per, k, stride,
                                        _p(order), _p(ids), cap, op[GUARD:].ctypes.data_as(_P), od[GUARD:].ctypes.data_as(_P), _p(counts), _p(cnt)), cnt)
    assert radius_host.guards_intact(op, n_all * k, od)
    return (op[GUARD:GUARD + n_all * k].reshape(n_all, k), od[GUARD:GUARD + n_all * k].reshape(n_all, k), counts, run.total()), run


def _overlap_pass(dll, tree, q, n_all, per, cap, order, original_ids, counts, offsets, lp, lanes):
    run = Sliced()
    for first, n in slices(n_all, per):
        cnt = np.zeros(3, dtype=np.uint64)
        run.add(dll.overlap_host_walk_slice(int(tree.double), _p(tree.pairs), tree.root, _p(tree.bboxes), _p(tree.ids), _p(q), first, n, lanes or per,
                                            _p(order), int(original_ids), cap, _p(counts), _p(offsets),
                                            None if lp is None else lp[GUARD:].ctypes.data_as(_P), _p(cnt)), cnt)
    return run


def overlap_sliced(dll, tree, queries, per, cap, order=None, original_ids=False, lanes=None):
    """overlap_boxes (queries None: overlap_self) as count pass, offsets, fill pass over the slices of `per` slots: what
    test_overlap_host.host_overlap returns, then the Sliced of the count pass and of the fill pass."""
    q = None if queries is None else _aligned(np.ascontiguousarray(queries, dtype=tree.dtype))
    n_all = tree.n if q is None else len(q)
    order = _u32(order)
    counts = np.full(n_all, 0xABABABAB, dtype=np.uint32)
    count_run = _overlap_pass(dll, tree, q, n_all, per, cap, order, original_ids, counts, None, None, lanes)
    offsets = np.concatenate([[0], np.cumsum(counts.astype(np.uint64))]).astype(np.uint64)
    total = int(offsets[-1])
    c2 = np.full(n_all, 0xABABABAB, dtype=np.uint32)
    lp = np.full(total + 2 * GUARD, SENT_PRIM, dtype=np.uint32)
    fill_run = _overlap_pass(dll, tree, q, n_all, per, cap, order, original_ids, c2, offsets, lp, lanes)
    assert (c2 == counts).all() and radius_host.guards_intact(lp, total)
    return (offsets, lp[GUARD:GUARD + total], counts, fill_run.total()), count_run, fill_run


def instanced_sliced(scene, rays, any_hit, robust, per, cap, original_ids=False, lanes=None):
    """The two-level walk over the slices of `per` rays: (hit records, instance per ray, Sliced); instanced_scenes.host_walk's outputs."""
    g = scene.geoms
    rays = _aligned(np.ascontiguousarray(rays, dtype=scene.dtype))
    top_pairs = _aligned(pair_records(scene.top_nodes["bounds"], scene.top_nodes["index"]))
    top_ids = scene.top_ids.astype(np.uint32)
    hits = _aligned(np.zeros(len(rays), dtype=oracle.HITD if scene.double else oracle.HITF))
    inst = np.zeros(len(rays), dtype=np.uint32)
    roots = np.array([x.root_index for x in g], dtype=np.uint32)
    tables = [sc._ptr_array([getattr(x, name) for x in g]) for name in ("pairs", "tris12", "ids32")]
    run = Sliced()
    for first, n in slices(len(rays), per):
        cnt = np.zeros(3, dtype=np.uint64)
        run.add(scene.dll.instanced_host_walk_slice(int(scene.double), _p(top_pairs), int(scene.top_nodes["index"][0]) & 0xFFFFFFFF, _p(top_ids), len(g),
                                                    tables[0], tables[1], tables[2], _p(roots), _p(scene.world2obj), _p(scene.gids), _p(rays), first, n,
                                                    lanes or per, int(any_hit), int(robust), int(original_ids), cap, _p(hits), _p(inst), _p(cnt)), cnt)
    return hits, inst, run
