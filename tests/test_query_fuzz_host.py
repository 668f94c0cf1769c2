"""CPU: the host harnesses of the four query bodies (closest_body.inc, radius_body.inc, knn_body.inc, overlap_body.inc, compiled by g++
from the kernels' own text) on adversarial scenes and on the tree shapes the golden scenes never have: a root that is a leaf, two to
five primitives, max_leaf_size 1, leaves of 9 to 15 primitives; trees from the restatement's builders (tests/adversarial_queries.py).

Exact tier (lattice points, quarter-lattice queries, lattice radii): every record, list, row, count and distance equals the numpy
brute force, nothing excluded, no tolerance. This is what pins the inclusive edges (d2 <= r2, box_dist2 <= r2, d2 <= worst on pop) and
the (d2, index) tie-break. Rounded tier (lattice triangles, duplicates, flat, mixed magnitudes, uniform, lattice spheres with zero
radii): the property checks of the host tests, unchanged. Overlap: walk == numpy brute force exactly on duplicated and collapsed boxes.

One test pins what the walk does NOT promise: on coincident zero-radius spheres in leaves of one, the primitive returned is one of
those at the minimum distance, not always the one of lowest index (docs/HISTORY.md, "Open: tie-break of the point queries")."""
import functools

import numpy as np
import pytest

import adversarial_queries as adv
import test_closest_point_host as closest_host
import test_knn_host as knn_host
import test_overlap_host as overlap_host
import test_radius_search_host as radius_host
from test_radius_search_host import GUARD, INVALID, SENT_PRIM, Tree, dfs_prim_order, host_radius

KS = (1, 5, 64)
EXACT_CASES = adv.cases(1, adv.EXACT_KINDS, 10)
ROUNDED_CASES = adv.cases(2, adv.ROUNDED_KINDS, 12)
OVERLAP_CASES = adv.cases(3, ("lattice", "dups", "flat", "scales", "uniform", "points_lattice", "spheres"), 8)


@pytest.fixture(scope="module")
def dlls(tmp_path_factory):
    d = tmp_path_factory.mktemp("query_fuzz")
    return {"closest": closest_host.compile_harness(d), "radius": radius_host.compile_harness(d), "knn": knn_host.compile_harness(d),
            "overlap": overlap_host.compile_harness(d)}


def build_tree(orc, raw, lim, bq):
    """The restatement's tree over the scene with the drawn shape: (nodes, prim_ids, BVH-order prims, leaf)."""
    sphere = raw.shape[1] == 4
    bb, cc = orc.sphere_bboxes(raw) if sphere else orc.prep_tris(raw)
    t = orc.build(bb, cc, builder=bq[0], quality=bq[1], min_leaf=lim[0], max_leaf=lim[1])
    nodes, ids = t.nodes(), t.prim_ids()
    prims = raw[ids.astype(np.int64)] if sphere else orc.precompute_tris(raw, ids)
    return nodes, ids, np.ascontiguousarray(prims), 1 if sphere else 0


def check_shape(nodes, n, lim):
    """The tree has the shape the case asks for: every primitive in exactly one leaf, no leaf above the limit; n == 1: the root is it."""
    dfs = dfs_prim_order(nodes["index"])
    assert len(dfs) == n and len(set(dfs.tolist())) == n
    counts = nodes["index"].astype(np.uint64) & np.uint64(15)
    assert counts.max() <= lim[1]
    if n == 1:
        assert len(nodes) == 1 and int(nodes["index"][0]) == 1                # a leaf word: first 0, count 1; no pair records
    return dfs, counts


# ---- exact tier -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _exact_scene(case):
    kind, n, lim, bq, dtype, seed = case
    rng = np.random.default_rng(seed)
    raw = adv.scene(rng, n, kind, dtype)
    return raw, adv.lattice_queries(rng, raw, dtype)


def run_exact(dlls, nodes, ids, prims, q, lim, what):
    """Every exact comparison on one tree with BVH-order primitives `prims` ((n, 12) points as triangles). -> the witnesses."""
    n = len(prims)
    dfs, _ = check_shape(nodes, n, lim)
    tree = Tree(nodes["bounds"], nodes["index"], prims, 0)
    d2 = adv.exact_d2(prims[:, :3], q)
    # closest: prim, t == sqrt(d2) bit for bit, u == v == 0
    hits, ccnt = closest_host.host_walk(dlls["closest"], nodes["bounds"], nodes["index"], prims, q, 0, threads=4)
    prim, t, hit = adv.expect_closest(d2, q)
    assert (hits["prim"] == prim).all(), (what, int((hits["prim"] != prim).sum()))
    assert hits["t"].tobytes() == t.tobytes(), what
    assert (hits["u"] == 0).all() and (hits["v"] == 0).all(), what
    ho, _ = closest_host.host_walk(dlls["closest"], nodes["bounds"], nodes["index"], prims, q, 0, prim_ids=ids.astype(np.uint32))
    assert (ho["prim"][hit] == ids[prim[hit].astype(np.int64)]).all() and (ho["prim"][~hit] == INVALID).all() and ho["t"].tobytes() == t.tobytes(), what
    # radius: counts, lists, distances
    offsets, lst, dist, counts, _ = host_radius(dlls["radius"], tree, q, threads=4)
    e_off, e_ids, e_dist, e_counts = adv.expect_radius(d2, q, dfs)
    assert (counts == e_counts).all(), (what, int((counts != e_counts).sum()))
    assert (offsets == e_off).all() and lst.tobytes() == e_ids.tobytes() and dist.tobytes() == e_dist.tobytes(), what
    # knn: ids, distances, counts, padding; k = 64 exceeds n in the small trees
    for k in KS:
        ki, kd, kc, kcnt = knn_host.host_knn(dlls["knn"], tree, q, k, threads=4)
        e_ki, e_kd, e_kc = adv.expect_knn(d2, q, k)
        assert (kc == e_kc).all(), (what, k)
        assert ki.tobytes() == e_ki.tobytes(), (what, k, int((ki != e_ki).any(axis=1).sum()))
        assert kd.tobytes() == e_kd.tobytes(), (what, k)
        if k == 1:                                             # k = 1 is closest_points, byte for byte, counters included
            assert ki[:, 0].tobytes() == np.ascontiguousarray(hits["prim"]).tobytes() and kd[:, 0].tobytes() == np.ascontiguousarray(hits["t"]).tobytes()
            assert kcnt.tobytes() == ccnt.tobytes(), (what, kcnt, ccnt)
    return adv.exact_witnesses(d2, q, adv.leaf_of_prims(nodes["index"], n))


@pytest.mark.parametrize("case", EXACT_CASES, ids=adv.case_id)
def test_exact_tier(dlls, orc, case):
    kind, n, lim, bq, dtype, seed = case
    raw, q = _exact_scene(case)
    nodes, ids, prims, leaf = build_tree(orc, raw, lim, bq)
    on_boundary, cross_leaf_ties, zero_radius = run_exact(dlls, nodes, ids, prims, q, lim, adv.case_id(case))
    print(f"{adv.case_id(case)}: {on_boundary} queries at distance exactly r, {cross_leaf_ties} rows with equal-d2 neighbours in different leaves, "
          f"{zero_radius} with r = 0 on a primitive")
    if kind == "points_lattice" and n >= 17:                   # (one point, or a tree of a leaf or two, need not offer all three)
        assert on_boundary > 0 and zero_radius > 0 and cross_leaf_ties > 0


def test_exact_tier_is_not_vacuous(orc):
    """Over the module's cases: queries at distance exactly r, ties across leaves, r = 0 on a primitive; and the fixed shapes are there."""
    total = np.zeros(3, dtype=np.int64)
    for case in EXACT_CASES:
        kind, n, lim, bq, dtype, seed = case
        raw, q = _exact_scene(case)
        nodes, ids, prims, _ = build_tree(orc, raw, lim, bq)
        total += adv.exact_witnesses(adv.exact_d2(prims[:, :3], q), q, adv.leaf_of_prims(nodes["index"], n))
    assert (total >= 100).all(), total
    for cases in (EXACT_CASES, ROUNDED_CASES, OVERLAP_CASES):
        assert any(c[1] == 1 for c in cases) and any(c[1] == 2 and c[2] == (1, 1) for c in cases) and any(c[1] >= 200 and c[2] == (9, 15) for c in cases)


# ---- rounded tier -----------------------------------------------------------------------------------------------------------------

def run_rounded(dlls, nodes, prims, leaf, raw, q, lim, what):
    """The host tests' property checks on one tree, per radius of the batch. -> adv.check_rounded's figures."""
    n = len(prims)
    dt = prims.dtype
    dfs, _ = check_shape(nodes, n, lim)
    tree = Tree(nodes["bounds"], nodes["index"], prims, leaf)
    tol = adv.host_tol(raw, dt)
    d2 = radius_host.host_brute(dlls["radius"], tree, q)
    hits, ccnt = closest_host.host_walk(dlls["closest"], nodes["bounds"], nodes["index"], prims, q, leaf, threads=4)
    offsets, lst, dist, counts, _ = host_radius(dlls["radius"], tree, q, threads=4)
    rows = {k: knn_host.host_knn(dlls["knn"], tree, q, k, threads=4) for k in KS}
    assert rows[1][0][:, 0].tobytes() == np.ascontiguousarray(hits["prim"]).tobytes() and rows[1][1][:, 0].tobytes() == np.ascontiguousarray(hits["t"]).tobytes()
    assert rows[1][3].tobytes() == ccnt.tobytes()
    return adv.check_rounded(hits, (offsets, lst, dist, counts), {k: v[:3] for k, v in rows.items()}, d2, q, dfs, tol, what)


@pytest.mark.parametrize("case", ROUNDED_CASES, ids=adv.case_id)
def test_rounded_tier(dlls, orc, case):
    kind, n, lim, bq, dtype, seed = case
    rng = np.random.default_rng(seed)
    raw = adv.scene(rng, n, kind, dtype)
    q = adv.rounded_queries(rng, raw, dtype)
    nodes, ids, prims, leaf = build_tree(orc, raw, lim, bq)
    run_rounded(dlls, nodes, prims, leaf, raw, q, lim, adv.case_id(case))


def test_coincident_zero_radius_spheres_keep_the_distance_not_the_index(dlls, orc):
    """Pins the open finding (docs/HISTORY.md): sphere_dist2 squares fl(sqrt(s)) - r, which can round below the exactly computed
    box_dist2 = s of a leaf that holds a coincident sphere, so that leaf is skipped although it holds an equal distance with a lower
    index. What holds, and is asserted: the distance returned is bit-equal to the brute-force minimum, and the primitive returned is
    one of those at that distance. When the arithmetic is made consistent, tighten this to `== the lowest index`."""
    differing = 0
    for dtype in (np.float32, np.float64):
        rng = np.random.default_rng(7)
        ctr = rng.integers(0, 5, size=(600, 3)).astype(dtype)                 # 125 lattice points: every centre several times
        raw = np.ascontiguousarray(np.concatenate([ctr, np.zeros((600, 1), dtype=dtype)], axis=1))
        nodes, ids, prims, leaf = build_tree(orc, raw, (1, 1), (0, 2))
        check_shape(nodes, 600, (1, 1))
        tree = Tree(nodes["bounds"], nodes["index"], prims, 1)
        q = np.zeros((256, 4), dtype=dtype)
        q[:, :3] = rng.integers(-4, 25, size=(256, 3)) * 0.25
        q[:, 3] = np.inf
        d2 = radius_host.host_brute(dlls["radius"], tree, q)
        hits, _ = closest_host.host_walk(dlls["closest"], nodes["bounds"], nodes["index"], prims, q, 1)
        assert (hits["prim"] != INVALID).all()
        assert hits["t"].tobytes() == np.sqrt(d2.min(axis=1)).tobytes()                       # the distance: the brute-force minimum, bit for bit
        assert (d2[np.arange(len(q)), hits["prim"]] == d2.min(axis=1)).all()                  # the primitive: among those at that distance
        differing += int((hits["prim"] != d2.argmin(axis=1)).sum())
    print(f"coincident zero-radius spheres: {differing} of 512 queries return a primitive at the minimum distance that is not the lowest index")


# ---- overlap ----------------------------------------------------------------------------------------------------------------------

def box_tree(orc, boxes, centres, lim, bq):
    t = orc.build(boxes, centres, builder=bq[0], quality=bq[1], min_leaf=lim[0], max_leaf=lim[1])
    nodes = t.nodes()
    return overlap_host.Tree(nodes["bounds"], nodes["index"], boxes, t.prim_ids()), nodes


def run_overlap(dll, tree, q, what):
    """Walk == numpy brute force, exactly: query boxes in both id modes and in fixed segments, then self mode. -> self pairs."""
    pb = tree.ordered_boxes()
    offsets, ids, counts, _ = overlap_host.host_overlap(dll, tree, q, threads=4)
    want_counts, want_ids = overlap_host.expected_lists(overlap_host.brute(pb, q), tree.dfs)
    assert (counts == want_counts).all(), (what, int((counts != want_counts).sum()))
    assert ids.tobytes() == want_ids.tobytes(), what
    oo, oi, oc, _ = overlap_host.host_overlap(dll, tree, q, original_ids=True)
    assert (oo == offsets).all() and (oi == tree.ids[ids.astype(np.int64)]).all() and (oc == counts).all(), what
    n, k, base = len(q), 3, 7                                  # k slots per query behind a non-zero base
    fixed = (base + k * np.arange(n + 1)).astype(np.uint64)
    total = base + k * n + 5
    c3, lp, _ = overlap_host.host_walk(dll, tree, q, offsets=fixed, total=total)
    assert (c3 == counts).all() and overlap_host.guards_intact(lp, total), what
    assert (lp[GUARD:GUARD + base] == SENT_PRIM).all() and (lp[GUARD + base + k * n:] == SENT_PRIM).all(), what
    seg = lp[GUARD + base:GUARD + base + k * n].reshape(n, k)
    want = np.full((n, k), INVALID, dtype=np.uint32)
    for i in range(n):
        m = min(int(counts[i]), k)
        want[i, :m] = want_ids[int(offsets[i]):int(offsets[i]) + m]
    assert (seg == want).all(), what
    within, (self_counts, self_ids) = overlap_host.self_expected(tree)
    so, si, sc, _ = overlap_host.host_overlap(dll, tree, None, threads=4)
    assert (sc == self_counts).all() and si.tobytes() == self_ids.tobytes(), what
    oso, osi, _, _ = overlap_host.host_overlap(dll, tree, None, original_ids=True)
    assert (oso == so).all() and (osi == tree.ids[si.astype(np.int64)]).all(), what
    return int(so[-1])


@pytest.mark.parametrize("case", OVERLAP_CASES, ids=adv.case_id)
def test_overlap_on_adversarial_boxes(dlls, orc, case):
    kind, n, lim, bq, dtype, seed = case
    rng = np.random.default_rng(seed)
    boxes, centres = adv.adversarial_boxes(rng, adv.scene(rng, n, kind, dtype))
    tree, nodes = box_tree(orc, boxes, centres, lim, bq)
    check_shape(nodes, n, lim)
    pairs = run_overlap(dlls["overlap"], tree, adv.box_queries(rng, boxes), adv.case_id(case))
    print(f"{adv.case_id(case)}: {pairs} self pairs")
    assert n > 1 or pairs == 0                                 # one primitive: nothing to pair it with


@pytest.mark.parametrize("n,lim,bq", [(2, (1, 1), (0, 2)), (65, (1, 1), (2, 0)), (200, (9, 15), (1, 2)), (200, (1, 8), (3, 0))])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_self_overlap_of_coincident_boxes(dlls, orc, n, lim, bq, dtype):
    """n copies of one box (with extent, and collapsed to a point): every pair overlaps, n (n - 1) / 2 of them, each once."""
    for box in ([1, 2, 3, 2, 4, 3.5], [1, 2, 3, 1, 2, 3]):
        boxes = np.ascontiguousarray(np.tile(np.asarray(box, dtype=dtype), (n, 1)))
        tree, nodes = box_tree(orc, boxes, np.ascontiguousarray((boxes[:, :3] + boxes[:, 3:]) * dtype(0.5)), lim, bq)
        check_shape(nodes, n, lim)
        q = np.ascontiguousarray(np.concatenate([boxes[:3], boxes[:3] + dtype(10)]))
        assert run_overlap(dlls["overlap"], tree, q, (n, lim, box)) == n * (n - 1) // 2
