"""Shared by tests/test_query_fuzz_host.py (CPU) and tests/test_gpu_query_fuzz.py (-m gpu): the adversarial scenes, queries and tree
shapes of the point and box queries, their exact expectations in numpy, and the project's property checks as functions.

Scenes: the triangle kinds of test_gpu_fuzz._scene3 (its seeds are not touched: every generator here is handed its own rng), zero-area
triangles on integer lattice points, one lattice point repeated, spheres on lattice centres with about 30 % zero radii, and for the
overlap queries the scene's boxes with about 10 % duplicated and about 10 % collapsed to zero extent on one to three axes.

The exact tier: primitives that are points of the integer lattice 0..4, queries on the quarter lattice -1..6, radii of LATTICE_RADII.
Every operation of tri_dist2 and box_dist2 is then exact in float and in double (det == 0, ee == 0, w == 0, d2 = |q - p|^2 a multiple
of 1/16 below 2^11), so the float64 numpy below IS the kernel's arithmetic and the comparison needs no tolerance and excludes nothing."""
import numpy as np

from test_gpu_fuzz import _scene3
from test_overlap_host import prim_boxes

INVALID = 0xFFFFFFFF
N_QUERIES = 1021                                               # not a multiple of 64 or 256
SIZES = (1, 2, 5, 17, 64, 65, 200, 1500, 4000)
LEAF_LIMITS = ((1, 8), (1, 1), (2, 4), (3, 15), (9, 15))
BUILDERS = ((2, 0), (3, 0), (0, 2), (1, 2), (1, 1))            # (builder, quality): binned, sweep, serial high, parallel high / medium
LATTICE_RADII = (0.0, 0.5, 1.0, 1.5, 2.5, 3.0, np.inf)
ROUNDED_KINDS = ("lattice", "dups", "flat", "scales", "uniform", "spheres")
EXACT_KINDS = ("points_lattice", "one_point")
# The shapes every module's parametrisation contains whatever the draw gives: a root that is a leaf, two leaves of one primitive, and
# leaves of 9 to 15 primitives in a tree of some depth.
FIXED_SHAPES = ((1, (1, 8), (2, 0)), (2, (1, 1), (0, 2)), (200, (9, 15), (1, 2)), (1500, (9, 15), (3, 0)))


def shapes(seed, drawn):
    """FIXED_SHAPES and `drawn` more (n, leaf limits, (builder, quality)) from the seed."""
    rng = np.random.default_rng(seed)
    out = list(FIXED_SHAPES)
    for _ in range(drawn):
        out.append((int(rng.choice(SIZES)), LEAF_LIMITS[int(rng.integers(0, len(LEAF_LIMITS)))], BUILDERS[int(rng.integers(0, len(BUILDERS)))]))
    return out


def cases(seed, kinds, drawn):
    """[(kind, n, leaf limits, (builder, quality), dtype, case seed)]: the shapes of `seed`, the kinds and both scalar types dealt
    round robin (shifted, so that a fixed shape does not always meet the same kind)."""
    out = []
    for j, (n, lim, bq) in enumerate(shapes(seed, drawn)):
        out.append((kinds[(j + seed) % len(kinds)], n, lim, bq, (np.float32, np.float64)[(j + j // 2) % 2], 100 * seed + j))
    return out


def case_id(c):
    kind, n, lim, bq, dtype, seed = c
    return f"{kind}-n{n}-leaf{lim[0]}_{lim[1]}-b{bq[0]}q{bq[1]}-{np.dtype(dtype).name}"


def scene(rng, n, kind, dtype):
    """(n, 9) triangles, or (n, 4) spheres for kind "spheres"."""
    if kind == "points_lattice":                               # zero-area triangles on the integer lattice 0..4, many coincident
        return _scene3(rng, n, "points", dtype)
    if kind == "one_point":                                    # all of them the same lattice point: a root box of zero extent
        return np.ascontiguousarray(np.tile(rng.integers(0, 5, size=3).astype(dtype), (n, 3)))
    if kind == "spheres":                                      # lattice centres (coincident ones included), about 30 % of radius exactly 0
        ctr = rng.integers(0, 5, size=(n, 3)).astype(dtype)
        rad = (rng.random((n, 1)) * 0.75).astype(dtype)
        rad[rng.random(n) < 0.3] = 0
        return np.ascontiguousarray(np.concatenate([ctr, rad], axis=1))
    return _scene3(rng, n, kind, dtype)


def sites(raw):
    """The vertices of triangles, the centres of spheres: (m, 3)."""
    return raw[:, :3] if raw.shape[1] == 4 else raw.reshape(-1, 3)


def scene_extent(raw):
    """(lo, hi, diagonal) in float64."""
    if raw.shape[1] == 4:
        c, r = raw[:, :3].astype(np.float64), raw[:, 3:4].astype(np.float64)
        lo, hi = (c - r).min(axis=0), (c + r).max(axis=0)
    else:
        p = raw.reshape(-1, 3).astype(np.float64)
        lo, hi = p.min(axis=0), p.max(axis=0)
    return lo, hi, float(np.linalg.norm(hi - lo))


def host_tol(raw, dtype):
    """The tolerance of the host tests' walk-against-brute-force checks, unchanged: 8 eps (1 + max |raw| + diag)."""
    return 8 * np.finfo(dtype).eps * (1.0 + float(np.abs(raw).max()) + scene_extent(raw)[2])


def rounded_queries(rng, raw, dtype, n=N_QUERIES):
    """(n, 4) {x, y, z, radius}: a third uniform in 1.3 times the scene box, a third exactly on vertices / centres, a third a small
    normal offset from one; the radius of each query one of 0, 5 % and 25 % of the diagonal and +inf."""
    lo, hi, diag = scene_extent(raw)
    s = sites(raw).astype(np.float64)
    a = b = n // 3
    c = n - a - b
    ctr, half = 0.5 * (lo + hi), 0.5 * (hi - lo) * 1.3
    pts = np.concatenate([ctr + (2.0 * rng.random((a, 3)) - 1.0) * half, s[rng.integers(0, len(s), size=b)],
                          s[rng.integers(0, len(s), size=c)] + rng.standard_normal((c, 3)) * 0.01 * (diag if diag > 0 else 1.0)])
    q = np.zeros((n, 4), dtype=dtype)
    q[:, :3] = pts[rng.permutation(n)]
    q[:, 3] = np.asarray([0.0, 0.05 * diag, 0.25 * diag, np.inf], dtype=dtype)[rng.integers(0, 4, size=n)]
    return q


def lattice_queries(rng, raw, dtype, n=N_QUERIES):
    """(n, 4) for the exact tier: two thirds anywhere on the quarter lattice -1..6, a third on primitives; radii of LATTICE_RADII."""
    a = n - n // 3
    s = sites(raw).astype(np.float64)
    pts = np.concatenate([rng.integers(-4, 25, size=(a, 3)) * 0.25, s[rng.integers(0, len(s), size=n - a)]])
    q = np.zeros((n, 4), dtype=dtype)
    q[:, :3] = pts[rng.permutation(n)]
    q[:, 3] = np.asarray(LATTICE_RADII, dtype=dtype)[rng.integers(0, len(LATTICE_RADII), size=n)]
    return q


def adversarial_boxes(rng, raw):
    """The scene's boxes by original id, about 10 % of them a copy of another and about 10 % collapsed to zero extent on one, two or
    three axes; and their centres, for the builders."""
    b = prim_boxes(raw).copy()
    n = len(b)
    dup = np.flatnonzero(rng.random(n) < 0.1)
    b[dup] = b[rng.integers(0, n, size=len(dup))]
    for i in np.flatnonzero(rng.random(n) < 0.1):
        axes = rng.permutation(3)[:int(rng.integers(1, 4))]
        b[i, 3 + axes] = b[i, axes]
    half = np.asarray(0.5, dtype=b.dtype)
    return np.ascontiguousarray(b), np.ascontiguousarray((b[:, :3] + b[:, 3:]) * half)


def box_queries(rng, boxes, n=N_QUERIES):
    """(n, 6): a third the primitives' own boxes, a third corners of them (zero extent: they touch), a third cubes around uniform points
    of 1.3 times the scene box; every 97th covers the scene, every 89th lies outside it."""
    dt = boxes.dtype
    lo, hi = boxes[:, :3].min(axis=0).astype(np.float64), boxes[:, 3:].max(axis=0).astype(np.float64)
    diag = float(np.linalg.norm(hi - lo))
    a = b = n // 3
    c = n - a - b
    own = boxes[rng.integers(0, len(boxes), size=a)]
    pick = boxes[rng.integers(0, len(boxes), size=b)]
    corner = np.where(rng.random((b, 3)) < 0.5, pick[:, :3], pick[:, 3:])
    ctr = 0.5 * (lo + hi) + (2.0 * rng.random((c, 3)) - 1.0) * 0.65 * (hi - lo)
    half = 0.1 * (diag if diag > 0 else 1.0) * rng.random((c, 1))
    q = np.concatenate([own, np.concatenate([corner, corner], axis=1), np.concatenate([ctr - half, ctr + half], axis=1).astype(dt)]).astype(dt)
    q = q[rng.permutation(n)]
    q[7::97, :3], q[7::97, 3:] = (lo - 1).astype(dt), (hi + 1).astype(dt)
    q[5::89] = np.concatenate([hi + 2, hi + 3]).astype(dt)
    return np.ascontiguousarray(q)


def leaf_of_prims(index, n):
    """leaf[i]: the node that holds BVH-order primitive i."""
    leaf = np.full(n, -1, dtype=np.int64)
    for k, w in enumerate(np.asarray(index).astype(np.uint64)):
        first, count = int(w) >> 4, int(w) & 15
        if count:
            leaf[first:first + count] = k
    assert (leaf >= 0).all()
    return leaf


# ---- exact expectations (float64 on dyadic data) --------------------------------------------------------------------------------------

def exact_d2(points, q):
    """d2[k, i] = |q_k - p_i|^2 in float64: exact for lattice points and quarter-lattice queries."""
    d = np.asarray(q, np.float64)[:, None, :3] - np.asarray(points, np.float64)[None, :, :]
    return (d * d).sum(axis=2)


def _within(d2, q):
    r = np.asarray(q, np.float64)[:, 3:4]
    with np.errstate(invalid="ignore"):
        return d2 <= r * r


def expect_closest(d2, q):
    """(prim uint32, t in q's dtype): the argmin by (d2, index) among the primitives within the radius; INVALID and the radius where
    there is none."""
    masked = np.where(_within(d2, q), d2, np.inf)
    best = masked.argmin(axis=1)                               # (the first minimum: the lowest index)
    bd2 = masked[np.arange(len(q)), best]
    hit = np.isfinite(bd2)
    t = np.where(hit, np.sqrt(np.where(hit, bd2, 0).astype(q.dtype)), q[:, 3]).astype(q.dtype)
    return np.where(hit, best, INVALID).astype(np.uint32), t, hit


def expect_knn(d2, q, k):
    """(ids (n, k) uint32, dist (n, k), counts uint32): the k smallest (d2, index) within the radius by a stable argsort, the rest of a
    row INVALID / the radius."""
    within = _within(d2, q)
    masked = np.where(within, d2, np.inf)
    order = np.argsort(masked, axis=1, kind="stable")[:, :k]
    if order.shape[1] < k:
        order = np.concatenate([order, np.zeros((len(order), k - order.shape[1]), dtype=order.dtype)], axis=1)
    counts = np.minimum(within.sum(axis=1), k)
    valid = np.arange(k)[None, :] < counts[:, None]
    dist = np.sqrt(np.where(valid, np.take_along_axis(masked, order, axis=1), 0).astype(q.dtype))
    return (np.where(valid, order, INVALID).astype(np.uint32), np.where(valid, dist, q[:, 3:4]).astype(q.dtype), counts.astype(np.uint32))


def expect_radius(d2, q, dfs):
    """(offsets uint64, ids uint32, dist, counts uint32): every primitive within the radius, in the tree's depth-first order."""
    w = _within(d2, q)[:, dfs]
    rows, cols = np.nonzero(w)
    counts = w.sum(axis=1)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    ids = dfs[cols]
    return offsets, ids.astype(np.uint32), np.sqrt(d2[rows, ids].astype(q.dtype)), counts.astype(np.uint32)


def exact_witnesses(d2, q, leaf, k=5):
    """What keeps the exact tier from being vacuous: (queries at distance exactly r > 0 of a primitive, rows of the k nearest with two
    neighbours of equal d2 in different leaves, queries of radius 0 on a primitive)."""
    r = np.asarray(q, np.float64)[:, 3:4]
    on_boundary = int(((d2 == r * r) & (r > 0) & np.isfinite(r)).any(axis=1).sum())
    zero = int(((d2 == 0) & (r == 0)).any(axis=1).sum())
    ids, _, counts = expect_knn(d2, q, k)
    valid = (np.arange(k)[None, 1:] < counts[:, None])
    gi = np.where(ids == INVALID, 0, ids).astype(np.int64)
    gd2 = np.take_along_axis(d2, gi, axis=1)
    cross = valid & (gd2[:, :-1] == gd2[:, 1:]) & (leaf[gi[:, :-1]] != leaf[gi[:, 1:]])
    return on_boundary, int(cross.any(axis=1).sum()), zero


# ---- the rounded tier's property checks, as the host tests state them -----------------------------------------------------------------

def check_radius_lists(offsets, ids, dist, d2, dfs, r, tol):
    """The checks of test_radius_search_host.test_walk_equals_brute_force for one radius r (a scalar of the tree's type) against the
    brute-force matrix d2 of the harness: (1) every list in the tree's order and within the brute force's set, its distances the
    square roots of the matrix entries; (2) only pairs within tol of the boundary may be lacking. -> (expected pairs, lacking pairs);
    the caller applies the cap (3)."""
    pos = np.empty(len(dfs), dtype=np.int64)
    pos[dfs] = np.arange(len(dfs))
    within = d2 <= r * r                                       # (r * r rounded in the scalar type, as the kernel does)
    lacking = 0
    for k in range(len(d2)):
        a, b = int(offsets[k]), int(offsets[k + 1])
        got = ids[a:b].astype(np.int64)
        p = pos[got]
        assert (np.diff(p) > 0).all(), k
        assert within[k, got].all(), k
        assert (dist[a:b] == np.sqrt(d2[k, got])).all(), k
        missed = within[k].copy()
        missed[got] = False
        if missed.any():
            dm = np.sqrt(d2[k, missed].astype(np.float64))
            assert (np.abs(dm - float(r)) <= tol).all(), (k, dm, float(r))
            lacking += int(missed.sum())
    return int(within.sum()), lacking


def check_closest(hits, walk_d2, brute_d2, r, tol):
    """The checks of test_closest_point_host.test_walk_equals_brute_force for one radius r: the walk's d2 is never below the brute
    force's and within tol of it, t = sqrt(d2), hit / miss agree away from the boundary, a miss reports the radius."""
    hit = hits["prim"] != INVALID
    bd = np.sqrt(brute_d2.astype(np.float64))
    if np.isfinite(r):
        clear = np.abs(bd - float(r)) > tol
        assert (hit[clear] == (bd <= float(r))[clear]).all()
    else:
        assert hit.all()
    assert (walk_d2[hit] >= brute_d2[hit]).all()
    assert (np.sqrt(walk_d2[hit].astype(np.float64)) - bd[hit] <= tol).all()
    assert (hits["t"][hit] == np.sqrt(walk_d2[hit])).all()
    assert (hits["t"][~hit] == r).all() and (hits["u"][~hit] == 0).all() and (hits["v"][~hit] == 0).all()
    return int(hit.sum())


def check_rounded(hits, radius, knn_rows, d2, q, dfs, tol, what):
    """The rounded tier on one tree, per radius of the batch: check_closest, check_radius_lists with the host test's cap, and
    test_knn_host.check_rows. hits: closest records; radius: (offsets, ids, dist, counts); knn_rows: {k: (ids, dist, counts)};
    d2: the harness's brute-force matrix (n x prims). -> (expected pairs, lacking pairs, knn rows that differ from the brute force's)."""
    from test_knn_host import brute_order, check_rows
    offsets, lst, dist, counts = radius
    brute_d2 = d2.min(axis=1)
    walk_d2 = d2[np.arange(len(q)), np.where(hits["prim"] == INVALID, 0, hits["prim"]).astype(np.int64)]
    expected = lacking = differing = 0
    for r in np.unique(q[:, 3]):
        sel = np.flatnonzero(q[:, 3] == r)
        check_closest(hits[sel], walk_d2[sel], brute_d2[sel], r, tol)
        sub_off = np.concatenate([[0], np.cumsum(counts[sel].astype(np.uint64))]).astype(np.uint64)
        sub_ids = np.concatenate([lst[int(offsets[j]):int(offsets[j + 1])] for j in sel])
        sub_dist = np.concatenate([dist[int(offsets[j]):int(offsets[j + 1])] for j in sel])
        e, l = check_radius_lists(sub_off, sub_ids, sub_dist, d2[sel], dfs, r, tol)
        expected += e
        lacking += l
        brute = brute_order(d2[sel], r * r)
        for k, (ki, kd, kc) in knn_rows.items():
            differing += check_rows(ki[sel], kd[sel], kc[sel], d2[sel], r, k, tol, brute)[0]
    print(f"{what}: radius lists lack {lacking} of {expected} expected pairs; {differing} knn rows differ from the brute force's")
    assert lacking <= 0.001 * expected, (what, lacking, expected)             # the host test's cap, not a tolerance
    everything = int(np.isinf(q[:, 3]).sum())
    assert everything > 0 and expected >= everything * d2.shape[1]             # (the queries with r = inf list every primitive)
    return expected, lacking, differing
