"""CPU: the host harnesses of sphere_cast, tri_distance, region_* and winding_* (the kernels' own text compiled by g++) on the
adversarial scenes and tree shapes of tests/adversarial_queries.py, with the batches of tests/adversarial_mesh_queries.py: a root that
is a leaf, two leaves of one primitive, leaves of 9 to 15, every builder of the restatement, coincident and collapsed primitives, root
boxes without extent, axis-parallel rays, -0.0, tmin < 0, segments and points as query triangles, exact copies of duplicated
triangles, planes through lattice vertices, query points in the plane of every triangle.

Trees: the restatement's, through test_query_fuzz_host.build_tree with the drawn shape; check_shape is asserted on every one.

tri_distance. Exact tier (point queries {p, p, p} on lattice points, the radius as max_distance): prim and the bytes of t equal the
numpy argmin by (d2, index), uv = 0, and the walk equals the harness's brute force byte for byte: this pins the inclusive
`key <= limit` pop, the `(d2 == best && i < best_prim)` tie rule and the start at max_distance^2 with no harness in between.
Rounded kinds: the checks of test_tri_distance_host.test_walk_against_brute_force with one max_distance per query.
sphere_cast. ROBUST on the rays with tmin >= 0: no contact of the brute force is missed, t >= the brute force's, residuals within
TOL, differing records capped; the fast box test the same on rays without a zero direction component, and only t >= brute and the
residuals on the others; on the marked tmin = -1 rays only that a reported hit is a contact (see the last test of this file).
region. test_region_host.test_walk_equals_brute_force's assertions, CULL and EXACT, plus regions of integer planes through lattice
vertices (plane values of exactly 0). winding. Moments finite and byte-stable under shuffled and 8-thread climbs; beta = inf against
winding_ref64 (det == 0 -> 0); w == 0 exactly on scenes without area at every beta; on a root that is a leaf the finite betas equal
the exact sum within beta radii of the root's own centre.

Measured on the CPU (this file prints the figures):
  tri_distance: records differing from the brute force: 0 of 1021 in every rounded case; largest |t - t64| / scale 1.6e-7 (float),
    1.3e-15 (double); TOL (1.01e-5, 8.5e-14) unchanged. Witnesses per points_lattice case with n >= 17: 62 .. 122 queries at distance
    exactly max_distance, 184 .. 338 with equal d2 in different leaves, 43 .. 68 with max_distance 0 on a primitive.
  sphere_cast: largest residual / scale 3.7e-7 (float), 4.9e-16 (double), against TOL 1.07e-6 / 1.9e-15, measured in extended
    precision (adversarial_mesh_queries.cast_residuals: in float64 the ruler itself is off by 1.6e-15 on a triangle of `dups`, which
    made two of 16,000 records of the double kernel read 2.3e-15). Records differing from the brute force: 0 everywhere but `flat`:
    16 of 1021 (ROBUST) and 15 (fast, of the 580 rays it is held to) on flat-n1500, 1 on flat-n5; no contact missed. Sent from afar
    through `flat` (origins a diagonal off the plane, so that bare rays cross the whole stack of coplanar triangles within an ulp of
    one t) 26 of 1021 differ, all within 64 sqrt(eps): the (t, index) argmin is promised for exact arithmetic only
    (sphere_cast_body.inc), so that batch is held to everything but the 2 % cap.
  region: CULL and EXACT lists and inside flags equal the brute force in every case, m = 1, 6, 8 and the lattice planes (m = 1, 3, 8);
    1,651 .. 576,000 plane values of exactly 0 at a vertex per lattice case.
  winding, beta = inf: dyadic tier within 16 eps n on every query (largest 7.9e-7 against 2.9e-3 in float32 at n = 1500, 5.6e-16
    against 7.1e-13 in float64; up to 58 % of all (query, triangle) pairs have a determinant of exactly 0). Rounded tier: see
    ROUNDED_MEASURED below; at most 1.1 % of the queries lie within 1e-4 diagonals of the surface and are left out.

Mutants, each made once by hand on a copy of the tree and run against this file (none is committed); every one fails it:
  | mutant                                                                    | fails                                               |
  | nearest_walk.inc: an entry popped on `key < limit`                          | 5 exact + 9 rounded tri_distance, 11 sphere_cast     |
  | tri_distance: accept on `d2 < best` alone (no index tie rule)               | 14 exact + 16 rounded tri_distance cases             |
  | tri_distance: best starts one ulp below max_distance^2                      | 7 exact tri_distance cases (distance == max_distance) |
  | sphere_cast: child boxes grown by 0 instead of r                            | 14 sphere_cast cases (contacts missed)               |
  | region: `d0 <= 0` made `d0 < 0` in the triangle test                        | 14 region cases                                      |
  | region: `<= 0` made `< 0` in node_in_region                                 | 14 region cases (spheres included)                   |
  | winding: a one-leaf root reads row 0 of the moments instead of row 1        | the 4 winding cases whose root is a leaf with area   |
The last one needed a case of its own: with beta = inf a row of zeros changes nothing, and finite values alone are no check; hence
the comparison of the finite betas with the exact sum on one-leaf roots."""
import functools
import math

import numpy as np
import pytest

import adversarial_mesh_queries as amq
import adversarial_queries as adv
import region_ref as R
import test_sphere_cast_host as cast_host
import test_tri_distance_host as dist_host
import test_winding_host as wind_host
import tri_intersect_ref as TR
from test_query_fuzz_host import build_tree, check_shape

INVALID = adv.INVALID


@pytest.fixture(scope="module")
def dlls(tmp_path_factory):
    d = tmp_path_factory.mktemp("mesh_query_fuzz")
    return {"cast": cast_host.compile_harness(d), "distance": dist_host.compile_harness(d), "region": R.compile_harness(d),
            "winding": wind_host.compile_harness(d)}


@functools.lru_cache(maxsize=None)
def _scene(case):
    kind, n, lim, bq, dtype, seed = case
    raw = adv.scene(np.random.default_rng(seed), n, kind, dtype)
    raw.setflags(write=False)
    return raw


def _rng(case, salt):
    return np.random.default_rng([case[5], salt])


# ---- sphere_cast ----------------------------------------------------------------------------------------------------------------------------

def run_cast(dll, nodes, ids, prims, leaf, raw, rays, radii, marks, what, cap=0.02):
    """ROBUST and the fast box test against the brute force. -> per box test (hits, differing records, largest residual / scale)."""
    dt = prims.dtype.type
    brute, _ = cast_host.host_brute(dll, prims, rays, radii, leaf)
    out = []
    for robust in (True, False):
        hits, cnt = cast_host.host_walk(dll, nodes["bounds"], nodes["index"], prims, rays, radii, leaf, robust=robust, threads=4)
        # ROBUST promises every contact at t >= 0; the fast test on top of that wants a direction without a zero component
        complete = ~marks["negative"] & (True if robust else ~marks["zero"])
        out.append(amq.check_cast(raw, ids, rays, radii, marks, hits, brute, leaf == 1, complete, cast_host.TOL[dt], (what, robust), cap=cap))
        perm = np.random.default_rng(9).permutation(len(rays)).astype(np.uint32)
        hp, cp = cast_host.host_walk(dll, nodes["bounds"], nodes["index"], prims, rays, radii, leaf, robust=robust, order=perm)
        assert hp.tobytes() == hits.tobytes() and (cp == cnt).all(), what
        ho, _ = cast_host.host_walk(dll, nodes["bounds"], nodes["index"], prims, rays, radii, leaf, robust=robust, prim_ids=ids.astype(np.uint32))
        hit = hits["prim"] != INVALID
        assert (ho["prim"][hit] == ids[hits["prim"][hit]]).all() and (ho["prim"][~hit] == INVALID).all(), what
        for f in ("t", "u", "v"):
            assert ho[f].tobytes() == hits[f].tobytes(), what
    return out


@pytest.mark.parametrize("case", amq.CAST_CASES, ids=adv.case_id)
def test_sphere_cast(dlls, orc, case):
    kind, n, lim, bq, dtype, seed = case
    raw = _scene(case)
    nodes, ids, prims, leaf = build_tree(orc, raw, lim, bq)
    check_shape(nodes, n, lim)
    rays, radii, marks = amq.rays(_rng(case, 1), raw, dtype)
    assert marks["negative"].sum() > 50 and 250 < marks["zero"].sum() < 450 and (radii == 0).sum() > 100
    (hr, dr, rr), (hf, df, rf) = run_cast(dlls["cast"], nodes, ids, prims, leaf, raw, rays, radii, marks, adv.case_id(case))
    print(f"{adv.case_id(case)}: ROBUST {hr} hits, {dr} records differ from the brute force, residual/scale {rr:.3e}; fast {hf} hits, {df} differ, {rf:.3e}")
    assert hr > 0
    lo, hi, diag = adv.scene_extent(raw)
    if (hi == lo).any():                                       # a scene without extent on some axis: also from afar (amq.rays, floor)
        rays, radii, marks = amq.rays(_rng(case, 6), raw, dtype, floor=diag if diag > 0 else 1.0)
        (hr, dr, rr), (hf, df, rf) = run_cast(dlls["cast"], nodes, ids, prims, leaf, raw, rays, radii, marks, adv.case_id(case), cap=None)
        print(f"{adv.case_id(case)}, from afar: ROBUST {hr} hits, {dr} records differ, residual/scale {rr:.3e}; fast {hf} hits, {df} differ, {rf:.3e}")
        assert hr > 0


# ---- tri_distance ---------------------------------------------------------------------------------------------------------------------------

def run_distance_exact(dll, tree, q4, what):
    """Point queries {p, p, p} on lattice points with the radius as max_distance: prim and the bytes of t equal the numpy argmin by
    (d2, index), uv = 0; and the walk equals the harness's brute force byte for byte. -> adv.exact_witnesses."""
    pts = tree.ordered_tris()[:, :3]
    d2 = adv.exact_d2(pts, q4)
    prim, t, hit = adv.expect_closest(d2, q4)
    queries, lim = np.ascontiguousarray(np.tile(q4[:, :3], (1, 3))), np.ascontiguousarray(q4[:, 3])
    hits, uv, cnt = dist_host.host_walk(dll, tree, queries, lim)
    assert (hits["prim"] == prim).all(), (what, int((hits["prim"] != prim).sum()))
    assert hits["t"].tobytes() == t.tobytes() and (hits["u"] == 0).all() and (hits["v"] == 0).all() and (uv == 0).all(), what
    brute, buv, _ = dist_host.host_brute(dll, tree, queries, lim)
    assert hits.tobytes() == brute.tobytes() and uv.tobytes() == buv.tobytes(), what
    ho, uo, _ = dist_host.host_walk(dll, tree, queries, lim, original_ids=True)
    assert (ho["prim"][hit] == tree.ids[prim[hit].astype(np.int64)]).all() and (ho["prim"][~hit] == INVALID).all() and ho["t"].tobytes() == t.tobytes(), what
    return adv.exact_witnesses(d2, q4, adv.leaf_of_prims(tree.index, tree.n))


@pytest.mark.parametrize("case", amq.DISTANCE_EXACT_CASES, ids=adv.case_id)
def test_tri_distance_exact_tier(dlls, orc, case):
    kind, n, lim, bq, dtype, seed = case
    raw = _scene(case)
    nodes, ids, prims, leaf = build_tree(orc, raw, lim, bq)
    check_shape(nodes, n, lim)
    tree = TR.TriTree(nodes["bounds"], nodes["index"], raw, ids)
    q4 = adv.lattice_queries(_rng(case, 2), raw, dtype)
    witnesses = run_distance_exact(dlls["distance"], tree, q4, adv.case_id(case))
    print(f"{adv.case_id(case)}: witnesses (distance exactly max_distance, equal d2 in different leaves, max_distance 0 on a primitive) {witnesses}")
    if kind == "points_lattice" and n >= 17:
        assert min(witnesses) > 0, witnesses


def run_distance(dll, tree, q, lim, what):
    """The rounded kinds: amq.check_distance on the walk, then order and ORIGINAL_IDS invariance."""
    dt = tree.dtype.type
    hits, uv, cnt = dist_host.host_walk(dll, tree, q, lim)
    brute, buv, second = dist_host.host_brute(dll, tree, q, lim)
    out = amq.check_distance(q, lim, tree.ordered_tris(), hits, uv, brute, second, dist_host.TOL[dt], what)
    perm = np.random.default_rng(9).permutation(len(q)).astype(np.uint32)
    hp, up, cp = dist_host.host_walk(dll, tree, q, lim, order=perm)
    assert hp.tobytes() == hits.tobytes() and up.tobytes() == uv.tobytes() and (cp == cnt).all(), what
    ho, uo, _ = dist_host.host_walk(dll, tree, q, lim, original_ids=True)
    hit = hits["prim"] != INVALID
    assert (ho["prim"][hit] == tree.ids[hits["prim"][hit]]).all() and (ho["prim"][~hit] == INVALID).all() and uo.tobytes() == uv.tobytes(), what
    for f in ("t", "u", "v"):
        assert ho[f].tobytes() == hits[f].tobytes(), what
    return out + (int((hits["t"][hit] == 0).sum()),)


@pytest.mark.parametrize("case", amq.DISTANCE_CASES, ids=adv.case_id)
def test_tri_distance_rounded_tier(dlls, orc, case):
    kind, n, lim, bq, dtype, seed = case
    raw = _scene(case)
    nodes, ids, prims, leaf = build_tree(orc, raw, lim, bq)
    check_shape(nodes, n, lim)
    tree = TR.TriTree(nodes["bounds"], nodes["index"], raw, ids)
    q, limits, _ = amq.query_tris(_rng(case, 3), raw, dtype)
    found, differ, err, zeros = run_distance(dlls["distance"], tree, q, limits, adv.case_id(case))
    print(f"{adv.case_id(case)}: {found} hits, {zeros} at distance 0, {differ} records differ from the brute force's (excused), max |t - t64|/scale {err:.3e}")
    assert zeros > 100                                         # (the copies, at least)


# ---- region ---------------------------------------------------------------------------------------------------------------------------------

def run_region(dll, tree, planes, what, original=False):
    """CULL, and EXACT for triangles, against the brute force. -> listed by CULL."""
    pairs_exact = lambda pr, pl: R.host_pairs(dll, pr, pl, tree.dtype)[1]
    listed = 0
    for exact in ((False, True) if tree.leaf == 0 else (False,)):
        offsets, ids, ins, counts, cnt = R.host_region(dll, tree, planes, exact=exact, threads=4)
        got, _ = amq.check_region(tree, planes, (offsets, ids, ins, counts), exact, pairs_exact, (what, exact))
        listed = listed or got
        if original:
            oo, oi, oins, oc, _ = R.host_region(dll, tree, planes, exact=exact, original_ids=True)
            assert (oo == offsets).all() and (oi == tree.ids[ids.astype(np.int64)]).all() and (oc == counts).all() and oins.tobytes() == ins.tobytes(), what
    return listed


@pytest.mark.parametrize("case", amq.REGION_CASES, ids=adv.case_id)
def test_region(dlls, orc, case):
    kind, n, lim, bq, dtype, seed = case
    raw = _scene(case)
    nodes, ids, prims, leaf = build_tree(orc, raw, lim, bq)
    check_shape(nodes, n, lim)
    tree = R.PrimTree(nodes["bounds"], nodes["index"], raw, ids)
    listed = 0
    for m in (1, 6, 8):
        planes = R.make_regions(raw, 192, m, dtype, seed + m)
        listed += run_region(dlls["region"], tree, planes, (adv.case_id(case), m), original=m == 6)
        kinds = 6 if m >= 6 else 3
        counts = R.host_walk(dlls["region"], tree, planes)[0]
        assert (counts[np.arange(192) % kinds == kinds - 2] == 0).all() and (counts[np.arange(192) % kinds == kinds - 1] == n).all()
    assert listed > 0
    if kind in amq.LATTICE_KINDS or kind == "spheres":
        through = 0
        for m in (1, 3, 8):
            planes = amq.lattice_regions(_rng(case, 4 + m), raw, dtype, 192, m)
            through += amq.planes_through_vertices(raw, planes)
            listed += run_region(dlls["region"], tree, planes, (adv.case_id(case), "lattice", m))
        print(f"{adv.case_id(case)}: {through} plane values of exactly 0 at a vertex")
        assert through > 0


# ---- winding --------------------------------------------------------------------------------------------------------------------------------

CLEARANCE = 1e-4                                               # of the diagonal: what the rounded tier keeps away from the surface
# The rounded tier (dups, scales, uniform) at beta = inf, on the queries clear of the surface: 16 eps n holds wherever n >= 5 (the
# largest figure measured is 741 eps, dups, n = 1500, float64, against 24000 eps) and does not for n = 1 and n = 2, where ONE solid
# angle seen from 1e-4 diagonals off its triangle's edge is already tens of eps off: largest |w - winding_ref64| measured over the
# cases with n <= 2: 25.6 eps in float32 (scales, n = 1), 86.0 eps in float64 (dups, n = 2). Asserted: the larger of 16 eps n and 4 x that.
ROUNDED_MEASURED = {np.float32: 3.05e-6, np.float64: 1.91e-14}


def run_winding(dll, nodes, prims, raw_ordered, kind, pts, what):
    """Moments (finite, the same bytes whatever the climb's order), then the walk. -> (largest |w - w64| at beta = inf, the bound,
    fraction of queries dropped for being within CLEARANCE of the surface)."""
    dt = prims.dtype.type
    eps = float(np.finfo(dt).eps)
    n, nn = len(prims), len(nodes)
    b, ix = nodes["bounds"], nodes["index"]
    mom = wind_host.host_prepare(dll, b, ix, prims)
    assert mom.shape == (nn + 1, 8) and np.isfinite(mom).all() and (mom[0] == 0).all(), what
    shuffled = np.random.default_rng(nn).permutation(nn)
    assert wind_host.host_prepare(dll, b, ix, prims, lanes=shuffled).tobytes() == mom.tobytes(), what
    assert wind_host.host_prepare(dll, b, ix, prims, threads=8).tobytes() == mom.tobytes(), what
    assert wind_host.host_prepare(dll, b, ix, prims, lanes=shuffled, threads=8).tobytes() == mom.tobytes(), what
    q = wind_host.queries4(pts, dt)
    worst = dropped = 0.0
    w_inf = None
    for beta in wind_host.BETAS[::-1]:                         # (+inf first: the exact sums the finite betas are held against)
        w, cnt = wind_host.host_walk(dll, b, ix, prims, mom, q, beta=beta)
        assert np.isfinite(w).all(), (what, beta)
        if kind in amq.AREALESS_KINDS:
            assert (w == 0).all(), (what, beta)
        elif nn == 1 and not math.isinf(beta):
            # a root that is a leaf: within beta radii of ITS centre (row 1 of the moments) the sum is the exact one, byte for byte
            d2 = ((q[:, :3].astype(np.float64) - mom[1, :3].astype(np.float64)) ** 2).sum(axis=1)
            near = d2 < beta * beta * float(mom[1, 3]) * (1 - 1e-5)
            assert near.sum() > 20 and w[near].tobytes() == w_inf[near].tobytes() and (w[near] != 0).any(), (what, beta, int(near.sum()))
        if math.isinf(beta):
            w_inf = w
            assert cnt[2] == 0 and cnt[1] == len(q) * n, (what, cnt)
            ref = amq.winding_ref64(raw_ordered, q)
            keep = np.ones(len(q), dtype=bool) if kind in amq.DYADIC_WINDING else amq.clear_of_surface(raw_ordered, q, CLEARANCE)
            dropped = 1.0 - keep.mean()
            assert dropped <= 0.05, (what, dropped)
            err = np.abs(w.astype(np.float64) - ref)[keep]
            worst = float(err.max())
            bound = 16 * eps * n if kind in amq.DYADIC_WINDING else max(16 * eps * n, 4 * ROUNDED_MEASURED[dt])
            assert worst <= bound, (what, worst, bound, int(np.argmax(err)))
    return worst, bound, dropped


@pytest.mark.parametrize("case", amq.WINDING_CASES + [c for pair in amq.MOVING_CASES.values() for c in pair], ids=adv.case_id)
def test_winding(dlls, orc, case):
    kind, n, lim, bq, dtype, seed = case
    raw = _scene(case)
    nodes, ids, prims, leaf = build_tree(orc, raw, lim, bq)
    check_shape(nodes, n, lim)
    pts = amq.winding_points(_rng(case, 5), raw, kind, dtype)
    worst, bound, dropped = run_winding(dlls["winding"], nodes, prims, raw[ids.astype(np.int64)], kind, pts, adv.case_id(case))
    print(f"{adv.case_id(case)}: beta = inf, largest |w - w64| {worst:.3e} against {bound:.3e}; {dropped:.1%} of the queries within "
          f"{CLEARANCE} diagonals of the surface left out")


def test_winding_in_plane_queries_see_zero_determinants(orc):
    """The dyadic tier is not vacuous: on `lattice` and `flat` a good part of all (query, triangle) pairs has a determinant of exactly
    0, and the reference with and without the det == 0 rule differ there."""
    import winding_scenes as ws
    for kind in ("lattice", "flat"):
        rng = np.random.default_rng(77)
        raw = adv.scene(rng, 200, kind, np.float32)
        pts = amq.winding_points(rng, raw, kind, np.float32)
        plain = ws.solid_angles64(raw, pts.astype(np.float64)).sum(axis=1) / (4 * np.pi)
        ruled = amq.winding_ref64(raw, pts)
        zero = amq.zero_determinants(raw, pts)
        print(f"{kind}: {zero.mean():.1%} of the (query, triangle) pairs have a determinant of exactly 0; the rule moves {int((plain != ruled).sum())} sums")
        assert zero.mean() > 0.05 and (np.abs(plain - ruled) >= 0.25).any(), kind


# ---- the shapes, and the negative-t finding ---------------------------------------------------------------------------------------------------

def test_cases_hold_the_fixed_shapes():
    for cases in (amq.CAST_CASES, amq.DISTANCE_EXACT_CASES, amq.DISTANCE_CASES, amq.REGION_CASES, amq.WINDING_CASES):
        assert any(c[1] == 1 for c in cases) and any(c[1] == 2 and c[2] == (1, 1) for c in cases) and any(c[1] >= 200 and c[2] == (9, 15) for c in cases)
        assert len(cases) >= 14


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_robust_finds_behind_the_origin_only_what_it_finds_in_front(dlls, orc, dtype):
    """Pins what ROBUST does NOT promise (include/bvh_amd.h, sphere_cast; DESIGN.md, "Sphere casts"): a contact at NEGATIVE t with a
    box thinner than the padding of the inverse direction. trace_device.h computes a slab's far plane as (far - org) * bump2(inv):
    the padded inverse moves the exit outward, which for t < 0 is towards more negative t, below the entry of a box of no thickness.
    Two triangles in the plane z = 0 (one leaf each: every box has zero extent in z), a ray straight down through one of them with
    tmin = -1 from just above the plane: the contact at t = -height is the brute force's and may be skipped by the walk. The same
    ray moved back along its direction, so that the same contact lies at t > 0, finds it, to the same point."""
    tris = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0], [2, 2, 0, 3, 2, 0, 2, 3, 0]], dtype=dtype)
    nodes, ids, prims, leaf = build_tree(orc, tris, (1, 1), (0, 2))
    assert len(nodes) == 3
    heights = np.array([7e-4, 6e-5, 2.0 ** -10, 0.25], dtype=dtype)
    rays = np.zeros((len(heights), 8), dtype=dtype)
    rays[:, 0], rays[:, 1], rays[:, 2] = 0.25, 0.25, heights
    rays[:, 5], rays[:, 6], rays[:, 7] = 1.0, -1.0, np.inf     # going UP: the plane is behind the origin, at t = -height
    brute, _ = cast_host.host_brute(dlls["cast"], prims, rays, 0.0, 0)
    assert (brute["prim"] != INVALID).all() and (np.abs(brute["t"] + heights) <= 2 * np.finfo(dtype).eps).all()       # (t = tmin + tau: rounded at 1)
    behind, _ = cast_host.host_walk(dlls["cast"], nodes["bounds"], nodes["index"], prims, rays, 0.0, 0, robust=True)
    found = behind["prim"] != INVALID
    assert behind[found].tobytes() == brute[found].tobytes()   # what is reported is the contact; nothing is claimed about the others
    print(f"{np.dtype(dtype).name}: contacts at t = -{heights.tolist()} found behind the origin: {found.tolist()}")
    # the cause is the box without thickness, not the sign of t: the same two triangles tilted (boxes half a unit thick in z) are
    # found behind the origin, like the brute force
    tilted = tris.copy()
    tilted[:, 2], tilted[:, 5], tilted[:, 8] = -0.25, 0.25, 0.0
    tn, tids, tprims, _ = build_tree(orc, tilted, (1, 1), (0, 2))
    up = rays.copy()
    up[:, 2] = 0.5                                              # above both boxes
    tb, _ = cast_host.host_brute(dlls["cast"], tprims, up, 0.0, 0)
    tw, _ = cast_host.host_walk(dlls["cast"], tn["bounds"], tn["index"], tprims, up, 0.0, 0, robust=True)
    assert (tb["prim"] != INVALID).all() and (tb["t"] < 0).all() and tw.tobytes() == tb.tobytes()
    moved = rays.copy()
    moved[:, 2] -= 1.0                                          # the origin moved back by one unit of t: the contact at t = 1 - height > 0
    moved[:, 6] = 0.0
    front, _ = cast_host.host_walk(dlls["cast"], nodes["bounds"], nodes["index"], prims, moved, 0.0, 0, robust=True)
    fb, _ = cast_host.host_brute(dlls["cast"], prims, moved, 0.0, 0)
    assert (front["prim"] != INVALID).all() and front.tobytes() == fb.tobytes()
    assert (front["prim"] == brute["prim"]).all() and np.allclose(front["t"], 1.0 - heights.astype(np.float64), atol=4 * np.finfo(dtype).eps)
