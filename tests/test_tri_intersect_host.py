"""CPU: the TEXT of the triangle-intersection kernel (bvh_amd/csrc/tri_intersect_body.inc + overlap_body.inc + list_walk.inc +
point_walk.inc + trace_device.h) compiled for the host by tests/cpp/tri_intersect_body_host.cpp. The pair test against an exact
integer reference on a lattice where its arithmetic is exact, and on constructed pairs; the walk over a lattice tree and the golden
trees against the brute force of the pair test (listed in the tree's left-first depth-first order): EXACT equality, nothing excluded.
The shapes of the output (count pass, exact offsets, fixed segments, padding, guard zones); self mode and its pair totals; the
shared-vertex filter; trees deeper than 64 levels and their sliced launches; the exported symbols. The device's counts, lists and
counters must equal this harness's byte for byte (tests/test_gpu_tri_intersect.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import query_slices as qs
import tri_intersect_ref as R
from conftest import ROOT
from tri_intersect_ref import GUARD, INVALID, SENT_PRIM, TREES, TRI_SCENES, _p, guards_intact

# unordered intersecting pairs of the scenes' own triangles, by the pair test (closed sets: a mesh's neighbours touch), and those of
# them without a common vertex; the lattice totals are those of the integer reference. (binned, parallel_high): where neighbours
# merely touch and the coordinates make the determinants round, the answer for a pair can depend on which of the two is the query,
# and that is the one that comes first in BVH order.
SELF_PAIRS = {"cornell": (144, 143), "soup2k": (64, 64), "terrain2k": (11749, 11753), "soup2k_f64": (64, 64), "lattice": 1453}
SELF_PAIRS_UNSHARED = {"cornell": (20, 20), "soup2k": (64, 64), "terrain2k": (0, 0), "soup2k_f64": (64, 64), "lattice": 1260}


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return R.compile_harness(tmp_path_factory.mktemp("tri_intersect"))


@pytest.fixture(scope="module")
def lattice():
    """The lattice triangles and their exact intersection matrix (computed once, never changed)."""
    t = R.lattice_tris()
    ref = R.sat_matrix(t, t)
    ref.setflags(write=False)
    t.setflags(write=False)
    return t, ref


def test_reference_matrix_is_the_python_int_reference(lattice):
    t, ref = lattice
    rng = np.random.default_rng(3)
    picks = [tuple(rng.integers(0, len(t), 2)) for _ in range(1500)] + [tuple(p) for p in np.argwhere(ref)[::3]]
    for i, j in picks:
        assert R.sat_intersects(t[i], t[j]) == ref[i, j]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pair_test_is_exact_on_the_lattice(dll, lattice, dtype):
    """Integer coordinates in [-8, 8], cast to the scalar type. The kernel's expressions: a coordinate difference is an integer of
    magnitude <= 16; a 2 x 2 determinant of differences (a normal's component, an orientation in the projection) a difference of two
    products <= 256, so <= 512; a 3 x 3 one ((v - o) . n, and (a - d) . ((b - d) x (c - d))) a sum of three products <= 16 * 512, so
    <= 24576 < 2^15, and so is every partial sum. All are integers far below 2^24: float32 and float64 compute them without rounding,
    and the answer must be the exact one on every pair, nothing excluded (each triangle with itself and both orders included)."""
    t, ref = lattice
    n = len(t)
    tf = t.astype(dtype)
    m = R.pair_matrix(dll, tf, tf)
    assert (m == ref).all(), np.argwhere(m != ref)[:5]
    # the scene has every class of pair
    iu = np.triu_indices(n, 1)
    normal = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    no_area = (normal == 0).all(axis=1)
    coplanar = np.stack([(np.einsum("jvk,k->jv", t - t[i, 0], normal[i]) == 0).all(axis=1) for i in range(n)]) & ~no_area[:, None] & ~no_area[None, :]
    shared = R.shares_vertex_matrix(t, t)
    classes = {"intersecting": int(ref[iu].sum()), "coplanar and intersecting": int((ref & coplanar)[iu].sum()),
               "coplanar and apart": int((~ref & coplanar)[iu].sum()), "sharing a vertex": int(shared[iu].sum()), "no area": int(no_area.sum())}
    print(classes)
    assert len(iu[0]) == 79800 and all(v > 20 for v in classes.values()), classes
    assert classes["intersecting"] == SELF_PAIRS["lattice"] and int((ref & ~shared)[iu].sum()) == SELF_PAIRS_UNSHARED["lattice"]
    # symmetric in its arguments; unchanged by rotating or reversing either triangle's vertices
    assert (m == m.T).all()
    for perm in ([1, 2, 0], [2, 0, 1], [0, 2, 1], [2, 1, 0], [1, 0, 2]):
        tp = np.ascontiguousarray(tf[:, perm])
        assert (R.pair_matrix(dll, tp, tf) == ref).all() and (R.pair_matrix(dll, tf, tp) == ref).all()
    # the shared-vertex filter removes exactly the pairs with a common vertex
    assert (R.pair_matrix(dll, tf, tf, skip_shared=True) == (ref & ~shared)).all()


A = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]
CONSTRUCTED = [
    ("a shared vertex only", A, [(0, 0, 0), (-2, 0, 1), (0, -2, 1)], True),
    ("a shared edge", A, [(0, 0, 0), (4, 0, 0), (0, -1, 3)], True),
    ("an edge piercing the interior", A, [(1, 1, -1), (1, 1, 1), (5, 5, 0)], True),
    ("an edge passing beside", A, [(3, 3, -1), (3, 3, 1), (5, 5, 0)], False),
    ("a vertex resting on the interior", A, [(1, 1, 0), (1, 1, 3), (2, 2, 3)], True),
    ("a vertex just above the interior", A, [(1, 1, 1), (1, 1, 3), (2, 2, 3)], False),
    ("a vertex on an edge", A, [(2, 0, 0), (2, -1, 2), (3, -1, 2)], True),
    ("coplanar, disjoint", A, [(5, 5, 0), (7, 5, 0), (5, 7, 0)], False),
    ("coplanar, disjoint though the boxes overlap", A, [(3, 3, 0), (5, 3, 0), (3, 5, 0)], False),
    ("coplanar, touching at a vertex", A, [(4, 0, 0), (6, 0, 0), (4, -2, 0)], True),
    ("coplanar, touching along an edge", A, [(0, 0, 0), (4, 0, 0), (2, -2, 0)], True),
    ("coplanar, touching vertex on edge", A, [(2, 2, 0), (4, 4, 0), (4, 2, 0)], True),
    ("coplanar, overlapping", A, [(1, 1, 0), (5, 1, 0), (1, 5, 0)], True),
    ("coplanar, contained", A, [(1, 1, 0), (2, 1, 0), (1, 2, 0)], True),
    ("coplanar, wound the other way", A, [(1, 1, 0), (1, 2, 0), (2, 1, 0)], True),
    ("parallel planes", A, [(0, 0, 1), (4, 0, 1), (0, 4, 1)], False),
    ("a zero-area triangle through the other", A, [(0, 0, 0), (1, 1, 0), (2, 2, 0)], False),
    ("a point-sized triangle on the other", A, [(1, 1, 0), (1, 1, 0), (1, 1, 0)], False),
]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_constructed_pairs(dll, dtype):
    for name, a, b, want in CONSTRUCTED:
        assert R.sat_intersects(a, b) == want, name            # (the table agrees with the exact reference)
        for x, y in ((a, b), (b, a)):
            assert R.pair_test(dll, x, y, dtype) == want, name
            shared = bool(set(map(tuple, x)) & set(map(tuple, y)))
            assert R.pair_test(dll, x, y, dtype, skip_shared=True) == (want and not shared), name
    through = [(1, 1, -1), (1, 1, 1), (5, 5, 0)]
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(9):
            b = np.array(through, dtype=dtype).reshape(9)
            assert R.pair_test(dll, A, b, dtype) and R.pair_test(dll, b, A, dtype)
            b[k] = bad
            assert not R.pair_test(dll, A, b, dtype) and not R.pair_test(dll, b, A, dtype), (bad, k)
    # -0 equals +0: as a coordinate of the test, and as a shared vertex
    neg = np.array([(-0.0, -0.0, 0.0), (-2, 0, 1), (0, -2, 1)], dtype=dtype)
    assert R.pair_test(dll, A, neg, dtype) and R.pair_test(dll, neg, A, dtype)
    assert not R.pair_test(dll, A, neg, dtype, skip_shared=True) and not R.pair_test(dll, neg, A, dtype, skip_shared=True)
    # a NaN equals nothing: two triangles that "share" a NaN vertex are not skipped for it, they intersect nothing anyway
    nan_a, nan_b = np.array(A, dtype=dtype), np.array(through, dtype=dtype)
    nan_a[0], nan_b[0] = np.nan, np.nan
    assert not R.pair_test(dll, nan_a, nan_b, dtype) and not R.pair_test(dll, nan_a, nan_b, dtype, skip_shared=True)


def check_walk(dll, tree, q, within, threads=4, **kw):
    """The count / offsets / fill walk of `q` equals the brute-force matrix `within` ([query, BVH-order primitive])."""
    offsets, ids, counts, cnt = R.host_intersect(dll, tree, q, threads=threads, **kw)
    want_counts, want_ids = R.expected_lists(within, tree.dfs)
    assert (counts == want_counts).all() and ids.tobytes() == want_ids.tobytes()
    return offsets, ids, counts, cnt


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_lattice_walk_equals_the_integer_reference(dll, orc, lattice, dtype):
    t, ref = lattice
    tree = R.built_tree(orc, t.astype(dtype), dtype)
    assert len(tree.dfs) == tree.n == len(t)
    order = tree.ids.astype(np.int64)
    # mesh against mesh: the lattice's own triangles as queries, then another lattice
    within = ref[:, order]
    assert (R.pair_matrix(dll, t.astype(dtype), tree.ordered_tris()) == within).all()
    _, _, counts, cnt = check_walk(dll, tree, t.astype(dtype), within)
    assert cnt[0] > 0 and cnt[1] > 0 and cnt[2] > 0 and (counts == 0).any() and counts.max() > 8
    other = R.lattice_tris(256, seed=77)
    check_walk(dll, tree, other.astype(dtype), R.sat_matrix(other, t)[:, order])
    # self mode: every pair once, no (q, q)
    self_within = ref[np.ix_(order, order)] & R.self_mask(tree.n)
    offsets, ids, counts, _ = check_walk(dll, tree, None, self_within)
    assert int(offsets[-1]) == SELF_PAIRS["lattice"] and (ids > np.repeat(np.arange(tree.n), counts)).all()
    shared = R.shares_vertex_matrix(t, t)[np.ix_(order, order)]
    offsets, _, _, _ = check_walk(dll, tree, None, self_within & ~shared, skip_shared=True)
    assert int(offsets[-1]) == SELF_PAIRS_UNSHARED["lattice"]


@pytest.mark.parametrize("scene", TRI_SCENES)
@pytest.mark.parametrize("mode", TREES)
def test_walk_equals_brute_force(dll, scene, mode):
    tree = R.golden_tree(scene, mode)
    assert len(tree.dfs) == tree.n and len(set(tree.dfs.tolist())) == tree.n
    pt = tree.ordered_tris()
    for name, q in (("moved", R.query_tris(tree.tris, 1024, 11)), ("own", tree.tris)):
        within = R.pair_matrix(dll, q, pt)
        offsets, ids, counts, cnt = check_walk(dll, tree, q, within)
        print(f"{scene} {mode} {name}: {len(ids)} listed triangles (mean list {len(ids) / len(q):.2f})")
        assert cnt[0] > 0 and cnt[1] > 0 and cnt[2] > 0 and len(ids) >= len(q) // 16
        if name == "moved":
            assert (counts[5::64] == 0).all() and (counts[::16] > 0).all()
            # original ids map values only; reading the batch through a permuted order changes nothing
            oo, oi, oc, _ = R.host_intersect(dll, tree, q, original_ids=True)
            assert (oo == offsets).all() and (oi == tree.ids[ids.astype(np.int64)]).all() and (oc == counts).all()
            perm = np.random.default_rng(5).permutation(len(q)).astype(np.uint32)
            po, pi, pc, pcnt = R.host_intersect(dll, tree, q, order=perm)
            assert (po == offsets).all() and pi.tobytes() == ids.tobytes() and (pcnt == cnt).all()
            # the shared-vertex filter, against numpy's ==
            shared = R.shares_vertex_matrix(q, pt)
            assert (R.pair_matrix(dll, q, pt, skip_shared=True) == (within & ~shared)).all()
            _, _, sc, scnt = check_walk(dll, tree, q, within & ~shared, skip_shared=True)
            assert (scnt == cnt).all()                          # (the filter comes after the fetch: the counters do not change)
            assert (sc[::16] < counts[::16]).any()              # an unmoved query shares vertices with its own neighbours


@pytest.mark.parametrize("scene", TRI_SCENES)
@pytest.mark.parametrize("mode", TREES)
def test_self_mode(dll, scene, mode):
    tree = R.golden_tree(scene, mode)
    pt = tree.ordered_tris()
    full = R.pair_matrix(dll, pt, pt)
    within = full & R.self_mask(tree.n)
    offsets, ids, counts, cnt = check_walk(dll, tree, None, within)
    assert int(offsets[-1]) == SELF_PAIRS[scene][TREES.index(mode)]
    assert (ids > np.repeat(np.arange(tree.n), counts)).all()    # i > q: no triangle with itself, every pair once
    assert cnt[1] < tree.n * tree.n // 4                         # triangles fetched: after the i > q filter
    oo, oi, _, _ = R.host_intersect(dll, tree, None, original_ids=True)
    assert (oo == offsets).all() and (oi == tree.ids[ids.astype(np.int64)]).all()
    shared = R.shares_vertex_matrix(pt, pt)
    so, _, _, scnt = check_walk(dll, tree, None, within & ~shared, skip_shared=True)
    assert int(so[-1]) == SELF_PAIRS_UNSHARED[scene][TREES.index(mode)] and (scnt == cnt).all()


def test_output_shapes(dll):
    tree = R.golden_tree("terrain2k", "parallel_high")
    q = R.query_tris(tree.tris, 300, 5)
    n = len(q)
    offsets, ids, counts, _ = R.host_intersect(dll, tree, q)       # count pass == list lengths, no padding, guards: checked inside
    assert counts.max() > 3 and (counts == 0).any() and (counts > 0).any()
    _, lp, _ = R.host_walk(dll, tree, q, offsets=offsets, total=len(ids), counts=False)        # without the optional counts: same lists
    assert (lp[GUARD:GUARD + len(ids)] == ids).all() and guards_intact(lp, len(ids))
    # k = 3 slots per query, the buffer starting at a non-zero offset: prefix in walk order, padding, untruncated counts, guards
    k, base = 3, 7
    fixed = (base + k * np.arange(n + 1)).astype(np.uint64)
    total = base + k * n + 5                                   # entries before offsets[0] and after offsets[n] belong to nobody
    c3, lp, _ = R.host_walk(dll, tree, q, offsets=fixed, total=total)
    assert (c3 == counts).all()
    assert (lp[GUARD:GUARD + base] == SENT_PRIM).all() and (lp[GUARD + base + k * n:] == SENT_PRIM).all() and guards_intact(lp, total)
    seg = lp[GUARD + base:GUARD + base + k * n].reshape(n, k)
    for i in range(n):
        m = min(int(counts[i]), k)
        assert (seg[i, :m] == ids[int(offsets[i]):int(offsets[i]) + m]).all() and (seg[i, m:] == INVALID).all()
    # stale offsets: a segment that ends before it begins is empty, the others (here all [0, 9)) are kept to; counts are still reported
    stale = np.zeros(n + 1, dtype=np.uint64)
    stale[::2] = 9
    c5, lp, _ = R.host_walk(dll, tree, q, offsets=stale, total=16)
    assert (c5 == counts).all()
    assert not (lp[GUARD + 9:GUARD + 16] != SENT_PRIM).any() and guards_intact(lp, 16)
    # self mode, fixed slots
    so, si, sc, _ = R.host_intersect(dll, tree, None)
    fixed = (2 * np.arange(tree.n + 1)).astype(np.uint64)
    c6, lp, _ = R.host_walk(dll, tree, None, offsets=fixed, total=2 * tree.n)
    seg = lp[GUARD:GUARD + 2 * tree.n].reshape(tree.n, 2)
    assert (c6 == sc).all() and sc.max() > 2 and guards_intact(lp, 2 * tree.n)
    for i in range(tree.n):
        m = min(int(sc[i]), 2)
        assert (seg[i, :m] == si[int(so[i]):int(so[i]) + m]).all() and (seg[i, m:] == INVALID).all()


def test_invalid_triangles(dll):
    """No area, a NaN, an infinity: as a query an empty list (a segment is padded), as a primitive never listed."""
    tree = R.golden_tree("cornell", "binned")
    dt = tree.dtype
    pt = tree.ordered_tris()
    q = np.ascontiguousarray(pt[:8].copy())
    q[1, 4] = np.nan
    q[2, 0] = np.inf
    q[3, 3:6] = q[3, 0:3]                                      # two equal vertices
    q[4] = np.array([0, 0, 0, 1, 1, 1, 3, 3, 3], dtype=dt)     # three points in a line
    within = R.pair_matrix(dll, q, pt)
    assert not within[1:5].any() and within[0].any() and within[5:].any(axis=1).all()
    check_walk(dll, tree, q, within)
    fixed = (2 * np.arange(len(q) + 1)).astype(np.uint64)
    _, lp, _ = R.host_walk(dll, tree, q, offsets=fixed, total=2 * len(q))
    assert (lp[GUARD:-GUARD].reshape(-1, 2)[1:5] == INVALID).all()
    # primitives made invalid (the tree is not refitted: the walk still reaches every other primitive)
    bad = tree.tris.copy()
    j, other = 3, 9
    bad[tree.ids[j], 7] = np.nan
    bad[tree.ids[other], 3:6] = bad[tree.ids[other], 0:3]
    t2 = tree.with_tris(bad)
    w2 = R.pair_matrix(dll, pt, t2.ordered_tris())
    assert not w2[:, j].any() and not w2[:, other].any()
    check_walk(dll, t2, pt, w2)
    so, si, sc, _ = R.host_intersect(dll, t2, None)
    assert sc[j] == 0 and sc[other] == 0 and j not in si and other not in si


@pytest.mark.parametrize("depth", [70, 300])
@pytest.mark.parametrize("stacked", [False, True])
def test_deep_chain(dll, depth, stacked):
    """Stacked, 70 levels cross LDS -> scratch (entry 16), scratch -> HBM (entry 64) and end on the last of the 6 HBM entries given;
    300 levels fill 236."""
    tree = R.chain_tree(depth, stacked=stacked)
    assert (tree.dfs == (np.arange(depth, -1, -1) if stacked else np.arange(depth + 1))).all()
    q = R.chain_queries(depth, 48)
    within = R.pair_matrix(dll, q, tree.ordered_tris())
    _, _, counts, _ = check_walk(dll, tree, q, within, deep_cap=depth - 64 if stacked else depth - 64 + 1)
    assert (counts[::4] == depth + 1).all() and 0 < counts[1::4].min() and counts[1::4].max() < 16
    # self mode: every triangle crosses its neighbours and is parallel to the ones after them
    pt = tree.ordered_tris()
    so, _, _, _ = check_walk(dll, tree, None, R.pair_matrix(dll, pt, pt) & R.self_mask(tree.n), deep_cap=depth - 64 + 1)
    assert int(so[-1]) == depth


@pytest.mark.parametrize("self_mode", [False, True])
def test_sliced_launches_of_a_deep_chain(dll, self_mode):
    """The launches point_query_run cuts a batch into over a deep tree (walk_slice: a.first, lane-indexed spill shared by the launch's
    lanes, one LDS stand-in per block): together they give what the whole batch gives, and no launch writes outside its spill."""
    depth, per = 300, 256
    cap = qs.deep_cap(depth)
    ids = qs.prim_ids(depth + 1)
    tree = R.chain_tree(depth, stacked=True, ids=ids)
    q = None if self_mode else R.chain_queries(depth, 600)
    n_all = tree.n if self_mode else len(q)
    qa = None if q is None else R._aligned(np.ascontiguousarray(q, dtype=tree.dtype))
    offsets, ids_want, counts_want, cnt_want = R.host_intersect(dll, tree, q, deep_cap=cap, original_ids=True)
    counts = np.full(n_all, 0xABABABAB, dtype=np.uint32)
    lp = np.full(len(ids_want) + 2 * GUARD, SENT_PRIM, dtype=np.uint32)
    total_cnt = np.zeros(3, dtype=np.uint64)
    launches = qs.slices(n_all, per)
    assert len(launches) > 1 and launches[-1][1] < per
    for first, n in launches:
        cnt = np.zeros(3, dtype=np.uint64)
        wrote = dll.tri_intersect_host_walk_slice(int(tree.double), _p(tree.pairs), tree.root, _p(tree.tris), _p(tree.ids), _p(qa), first, n, per, None, 1, 0,
                                                  cap, _p(counts), _p(offsets), lp[GUARD:].ctypes.data_as(C.c_void_p), _p(cnt))
        assert wrote >= 0, wrote                               # (-1: a guard zone of the spill was written to)
        total_cnt += cnt
    assert (counts == counts_want).all() and (lp[GUARD:GUARD + len(ids_want)] == ids_want).all() and guards_intact(lp, len(ids_want))
    assert (total_cnt == cnt_want).all()
    assert dll.tri_intersect_host_walk_slice(int(tree.double), _p(tree.pairs), tree.root, _p(tree.tris), _p(tree.ids), _p(qa), 0, per + 1, per, None, 0, 0, cap,
                                             _p(counts), None, None, _p(total_cnt)) == -2


def test_tri_intersect_symbols_are_declared_and_exported():
    from bvh_amd import _lib, build
    build.build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "bvh_amd.h")).read()
    declared = set(re.findall(r"BVH_AMD_API[^;]*?\b(bvh\w+)\s*\(", header))
    want = {f"bvh{s}_intersect_tris{kind}" for s in ("3f", "3d") for kind in ("", "_self")}
    assert {n for n in declared if "intersect_tris" in n} == want
    assert want <= set(_lib.exported_symbols())
    for name in sorted(want):
        assert hasattr(lib, name), name
    for s in ("2f", "2d"):
        for kind in ("", "_self"):
            assert not hasattr(lib, f"bvh{s}_intersect_tris{kind}")
            assert f"bvh{s}_intersect_tris{kind}" not in _lib.exported_symbols()
    assert re.search(r"BVH_AMD_TRI_SKIP_SHARED\s*=\s*32u", header)
    import bvh_amd
    for name in ("tri_intersect_count", "tri_intersect_search", "self_intersections"):
        assert callable(getattr(bvh_amd, name))
