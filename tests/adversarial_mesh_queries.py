"""Shared by tests/test_mesh_query_fuzz_host.py (CPU) and tests/test_gpu_mesh_query_fuzz.py (-m gpu): the adversarial batches of the
sphere-cast, triangle-distance, convex-region and winding-number queries over the scenes and tree shapes of tests/adversarial_queries.py
(its `cases`, `scene`, `lattice_queries`, `expect_closest`, ... are used as they are), the float64 references those need, and the
property checks of the four host test files as functions, so that the CPU tier and the device tier assert the same thing.

Every generator is handed its own rng and the case lists below carry their own seeds: nothing here draws from, or shifts, the streams
of the other fuzz modules. Not a test module."""
import numpy as np

import adversarial_queries as adv
import region_ref
import winding_scenes as ws
from test_sphere_cast_host import dist64

INVALID = adv.INVALID
N_QUERIES = adv.N_QUERIES                                      # 1021: not a multiple of 64 or 256
TRI_KINDS = ("lattice", "dups", "flat", "scales", "uniform")
LATTICE_KINDS = ("lattice", "points_lattice", "one_point")     # every coordinate a small multiple of 1/2
AREALESS_KINDS = adv.EXACT_KINDS                               # points_lattice, one_point: no triangle has area
DYADIC_WINDING = ("lattice", "flat") + AREALESS_KINDS          # the winding tier in which every query is checked
RADIUS_FRACTIONS = (0.0, 0.001, 0.01, 0.05, 0.25)

# (kind, n, leaf limits, (builder, quality), dtype, seed) as adversarial_queries.cases deals them: FIXED_SHAPES and 12 drawn each.
CAST_CASES = adv.cases(7, TRI_KINDS + ("spheres",) + AREALESS_KINDS, 12)
DISTANCE_EXACT_CASES = adv.cases(1, adv.EXACT_KINDS, 10)
DISTANCE_CASES = adv.cases(8, TRI_KINDS, 12)
REGION_CASES = adv.cases(9, TRI_KINDS + ("spheres",) + AREALESS_KINDS, 12)
WINDING_CASES = adv.cases(10, TRI_KINDS + AREALESS_KINDS, 12)
# the degenerate root boxes with more than one primitive, whatever the deal gives (as test_gpu_query_fuzz.POINT_CASES adds them)
DEGENERATE_ROOTS = [("flat", 200, (1, 8), (2, 0), np.float32, 1051), ("flat", 65, (1, 1), (0, 2), np.float64, 1052),
                    ("one_point", 65, (1, 8), (3, 0), np.float32, 1053), ("one_point", 200, (9, 15), (1, 2), np.float64, 1054)]
# the geometry the moving-geometry test of the device tier refits a `uniform` tree to, per (leaf limits, scalar type): lattice points,
# then duplicates. The host tier walks the same scenes (under their own trees), so what it measures covers them.
MOVING_CASES = {(lim, np.dtype(dt).name): tuple((kind, 1500, lim, (0, 2), dt, 1100 + 10 * j + k) for k, kind in enumerate(("points_lattice", "dups")))
                for j, (lim, dt) in enumerate(((l, d) for l in ((3, 15), (1, 1)) for d in (np.float32, np.float64)))}


def _unit_diag(diag):
    return diag if diag > 0 else 1.0


# ---- rays for sphere_cast ----------------------------------------------------------------------------------------------------------------

def rays(rng, raw, dtype, n=N_QUERIES, floor=1e-3):
    """(rays (n, 8), radii (n,), marks). A third of the directions along an axis (both signs), about 5 % of the others with one
    component of -0.0, the rest without a zero component; origins in 1.4 times the scene box (an extent below `floor` counts as
    `floor`, as in test_gpu_fuzz._rays3: over a flat scene the default keeps the origins within 0.0007 of its plane, so that a ball
    with a radius starts in contact; floor = the diagonal sends them well off the plane, through the whole stack of coplanar
    triangles), a fifth snapped onto a plane of the box; tmax finite for a fifth; tmin 0 but for a tenth with tmin = -1;
    one radius per ray out of RADIUS_FRACTIONS of the diagonal (1 where that is 0). Rays 3, 4 and 5 are invalid: NaN tmin, NaN
    radius, negative radius. marks: {"negative": tmin < 0, "zero": a direction component is 0, "invalid": the three}."""
    lo, hi, diag = adv.scene_extent(raw)
    d1 = _unit_diag(diag)
    half = 0.7 * np.maximum(hi - lo, floor)
    mid = 0.5 * (lo + hi)
    org = mid + (2.0 * rng.random((n, 3)) - 1.0) * half
    snap = np.flatnonzero(rng.random(n) < 0.2)
    axis = rng.integers(0, 3, size=len(snap))
    org[snap, axis] = np.where(rng.random(len(snap)) < 0.5, lo[axis], hi[axis])
    d = rng.standard_normal((n, 3))
    d[d == 0] = 0.5                                            # (never drawn in practice; "no zero component" is then a fact)
    which = rng.integers(0, 9, size=n)                         # 0, 1, 2: along x, y, z
    for a in range(3):
        sel = np.flatnonzero(which == a)
        d[sel] = 0.0
        d[sel, a] = np.where(rng.random(len(sel)) < 0.5, 1.0, -1.0)
    minus = np.flatnonzero((which >= 3) & (rng.random(n) < 0.05))
    d[minus, rng.integers(0, 3, size=len(minus))] = -0.0
    r = np.zeros((n, 8), dtype=dtype)
    r[:, 0:3], r[:, 3:6] = org, d
    r[:, 6] = np.where(rng.random(n) < 0.1, -1.0, 0.0)
    r[:, 7] = np.where(rng.random(n) < 0.2, rng.random(n) * 1.5 * d1, np.inf)
    radii = (np.asarray(RADIUS_FRACTIONS)[rng.integers(0, len(RADIUS_FRACTIONS), size=n)] * d1).astype(dtype)
    r[3, 6], radii[4], radii[5] = np.nan, np.nan, -radii[5] - dtype(0.125)
    invalid = np.zeros(n, dtype=bool)
    invalid[3:6] = True
    marks = {"negative": (r[:, 6] < 0) & ~invalid, "zero": (r[:, 3:6] == 0).any(axis=1), "invalid": invalid}
    return np.ascontiguousarray(r), np.ascontiguousarray(radii), marks


# ---- query triangles for tri_distance -----------------------------------------------------------------------------------------------------

def query_tris(rng, raw, dtype, n=N_QUERIES):
    """(queries (n, 9), max_distance (n,), the kind of each query). Each query is made from a triangle of the scene: kind 0 an exact
    copy (distance 0, and a tie wherever the scene holds duplicates), 1 moved by about 2 % of the diagonal, 2 shrunk to 30 % and
    lifted by up to 5 %, 3 put anywhere in 1.3 times the box; every 10th a segment, every 50th a point. max_distance is one of
    {inf, the median distance from a query's first vertex to the scene's nearest vertex, 0}; queries 5 and 11 carry NaN and -1."""
    t = np.asarray(raw).reshape(-1, 3, 3)
    lo, hi, diag = adv.scene_extent(raw)
    d1 = _unit_diag(diag)
    src = t[rng.integers(0, len(t), size=n)].astype(np.float64)
    kind = rng.integers(0, 4, size=n)
    q = src.copy()
    m = kind == 1
    q[m] += 0.02 * d1 * rng.standard_normal((int(m.sum()), 1, 3))
    m = kind == 2
    c = q[m].mean(axis=1, keepdims=True)
    q[m] = c + 0.3 * (q[m] - c) + 0.05 * d1 * (2.0 * rng.random((int(m.sum()), 1, 3)) - 1.0)
    m = kind == 3
    c = q[m].mean(axis=1, keepdims=True)
    q[m] = q[m] - c + (0.5 * (lo + hi) + (2.0 * rng.random((int(m.sum()), 1, 3)) - 1.0) * 0.65 * np.where(hi > lo, hi - lo, d1))
    q[::10, 2] = q[::10, 1]
    q[::50, 1], q[::50, 2] = q[::50, 0], q[::50, 0]
    q = np.ascontiguousarray(q.reshape(n, 9).astype(dtype))
    verts = t.reshape(-1, 3).astype(np.float64)
    first = q[:, :3].astype(np.float64)
    nearest = np.sqrt(np.min(((first[:, None, :] - verts[None, ::max(1, len(verts) // 2000), :]) ** 2).sum(axis=2), axis=1))
    lim = np.asarray([np.inf, np.median(nearest), 0.0], dtype=dtype)[rng.integers(0, 3, size=n)]
    lim[5], lim[11] = np.nan, -1.0
    return q, np.ascontiguousarray(lim), kind


# ---- regions --------------------------------------------------------------------------------------------------------------------------------

LATTICE_NORMALS = np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1], [1, 1, 0], [1, -1, 0], [0, 1, 1], [-1, 0, 1], [1, 1, 1], [1, -1, 1], [2, 1, 0],
                            [-1, 2, 0], [1, 2, -2], [2, -1, 2], [-2, -2, 1], [3, 4, 0], [0, -3, 4], [2, 3, 6]], dtype=np.float64)


def lattice_regions(rng, raw, dtype, n, m):
    """(n, m, 4) regions for the lattice kinds: min(m, 1 + k % 3) planes with an integer normal of LATTICE_NORMALS (either sign)
    through a vertex (or centre) of the scene, padded with planes that hold everywhere. Every product of the stated plane expression
    is then exact (multiples of 1/2 below 2^7), so the value at that vertex is exactly 0: the inclusive edge of the leaf test."""
    sites = adv.sites(raw).astype(np.float64)
    out = np.zeros((n, m, 4), dtype=np.float64)
    for k in range(n):
        planes = []
        for _ in range(min(m, 1 + k % 3)):
            nrm = LATTICE_NORMALS[rng.integers(0, len(LATTICE_NORMALS))] * (1.0 if rng.random() < 0.5 else -1.0)
            p = sites[rng.integers(0, len(sites))]
            planes.append([nrm[0], nrm[1], nrm[2], -float(nrm @ p)])
        out[k] = region_ref.pad_planes(planes, m, k)
    return np.ascontiguousarray(out.astype(dtype))


def planes_through_vertices(raw, planes):
    """The witness of lattice_regions: how many (region, plane with a normal, vertex or centre) triples have a plane value of exactly
    0, by the stated expression in the scene's scalar type."""
    pts = np.ascontiguousarray(adv.sites(raw))
    real = (np.asarray(planes)[:, :, :3] != 0).any(axis=2)
    return int(((region_ref.plane_values(planes, pts) == 0) & real[:, :, None]).sum())


# ---- winding points -------------------------------------------------------------------------------------------------------------------------

def winding_points(rng, raw, kind, dtype, n=N_QUERIES):
    """(n, 3) query points. Dyadic tier (DYADIC_WINDING): two thirds on the quarter lattice -1 .. 6, a third exactly on vertices; for
    `flat` a further third replaced by points IN the plane z = 0. Rounded tier: half uniform in 1.3 times the box, half a small
    offset (about 1 % of the diagonal) from a vertex, none ON a vertex (the winding number of a surface point is not defined)."""
    lo, hi, diag = adv.scene_extent(raw)
    d1 = _unit_diag(diag)
    verts = np.asarray(raw).reshape(-1, 3).astype(np.float64)
    if kind in DYADIC_WINDING:
        a = n - n // 3
        pts = np.concatenate([rng.integers(-4, 25, size=(a, 3)) * 0.25, verts[rng.integers(0, len(verts), size=n - a)]])
        if kind == "flat":
            inplane = rng.permutation(n)[:n // 3]
            pts[inplane, 2] = np.where(rng.random(len(inplane)) < 0.5, 0.0, -0.0)
            pts[inplane[::2], :2] = rng.random((len(inplane[::2]), 2)) * 1.5 - 0.25
        return np.ascontiguousarray(pts[rng.permutation(n)].astype(dtype))
    a = n // 2
    off = rng.standard_normal((n - a, 3))
    off = 0.01 * d1 * off / np.linalg.norm(off, axis=1, keepdims=True) * (0.25 + rng.random((n - a, 1)))
    pts = np.concatenate([0.5 * (lo + hi) + (2.0 * rng.random((a, 3)) - 1.0) * 0.65 * np.where(hi > lo, hi - lo, d1),
                          verts[rng.integers(0, len(verts), size=n - a)] + off])
    pts = np.ascontiguousarray(pts[rng.permutation(n)].astype(dtype))
    on_vertex = (pts[:, None, :] == np.asarray(raw).reshape(-1, 3)[None, :, :]).all(axis=2).any(axis=1)
    pts[on_vertex] += dtype(0.003 * d1)                        # (an offset rounded away: move it off again)
    return pts


def zero_determinants(tris9, q):
    """[query, triangle]: the float64 determinant a . (b x c) of the triangle's vertices seen from the query is exactly 0."""
    t = np.asarray(tris9, dtype=np.float64).reshape(-1, 3, 3)
    out = np.zeros((len(q), len(t)), dtype=bool)
    for k, p in enumerate(np.asarray(q, dtype=np.float64)[:, :3]):
        a, b, c = t[:, 0] - p, t[:, 1] - p, t[:, 2] - p
        out[k] = np.einsum("ij,ij->i", a, np.cross(b, c)) == 0
    return out


def winding_ref64(tris9, q):
    """float64 winding numbers over all triangles: winding_scenes.solid_angles64, with the solid angle of a triangle whose computed
    determinant is exactly 0 (its plane holds the query) taken as 0, which is what include/bvh_amd.h promises for such a triangle."""
    t = np.asarray(tris9, dtype=np.float64).reshape(-1, 3, 3)
    q = np.asarray(q, dtype=np.float64)[:, :3]
    om = ws.solid_angles64(t.reshape(-1, 9), q)
    om[zero_determinants(t, q)] = 0.0
    return om.sum(axis=1) / (4 * np.pi)


def clear_of_surface(tris9, q, frac):
    """Mask: the query is at least frac * diagonal (1 where that is 0) away from every triangle, by test_sphere_cast_host.dist64."""
    t = np.asarray(tris9, dtype=np.float64).reshape(-1, 9)
    q = np.asarray(q, dtype=np.float64)[:, :3]
    need = frac * _unit_diag(adv.scene_extent(np.asarray(tris9).reshape(-1, 9))[2])
    out = np.zeros(len(q), dtype=bool)
    for k, p in enumerate(q):
        out[k] = dist64(t, np.broadcast_to(p, (len(t), 3))).min() >= need
    return out


# ---- property checks, as the host tests state them ------------------------------------------------------------------------------------------

def _dist_ext(tri, q):
    """test_sphere_cast_host.dist64 in extended precision (numpy's longdouble: a 64-bit significand on x86). In float64 the foot
    ap - u ab - v ac of a point ON a triangle cancels to the rounding noise of u and v, about eps |ab| / sin^2 of the triangle's
    angle: 1.6e-15 on a triangle of `dups` with sin = 0.29, which is the whole of TOL[float64] = 1.9e-15. The double kernel's records
    must be measured with something finer than themselves."""
    from test_sphere_cast_host import _dot, _seg_dist, degenerate64
    L = np.longdouble
    tri, q = np.asarray(tri, dtype=L), np.asarray(q, dtype=L)
    a, b, c = tri[:, 0:3], tri[:, 3:6], tri[:, 6:9]
    best = np.minimum(np.minimum(_seg_dist(q, a, b), _seg_dist(q, a, c)), _seg_dist(q, b, c))
    ab, ac, ap = b - a, c - a, q - a
    abab, acac, abac, apab, apac = _dot(ab, ab), _dot(ac, ac), _dot(ab, ac), _dot(ap, ab), _dot(ap, ac)
    det = abab * acac - abac * abac
    ok = ~degenerate64(tri) & (det > 0)
    sdet = np.where(ok, det, L(1))
    u, v = (acac * apab - abac * apac) / sdet, (abab * apac - abac * apab) / sdet
    inside = ok & (u >= 0) & (v >= 0) & (u + v <= 1)
    foot = np.linalg.norm(ap - u[:, None] * ab - v[:, None] * ac, axis=1)
    return np.where(inside, np.minimum(best, foot), best)


def cast_residuals(raw, ids, rays_, radii, hits, sphere):
    """test_sphere_cast_host.prim_residuals (residual / scale of every record against ITS primitive, from the original vertices /
    spheres), evaluated in extended precision: the same quantity, a finer ruler."""
    L = np.longdouble
    hit = hits["prim"] != INVALID
    prim = np.where(hit, hits["prim"], 0).astype(np.int64)
    src = np.asarray(raw)[np.asarray(ids).astype(np.int64)][prim].astype(L)
    r64, r = rays_.astype(L), radii.astype(L)
    t = np.where(hit, hits["t"].astype(L), L(0))
    ct = r64[:, 0:3] + t[:, None] * r64[:, 3:6]
    if sphere:
        dist = np.maximum(np.linalg.norm(ct - src[:, :3], axis=1) - src[:, 3], L(0))
        scale = np.maximum(np.abs(src).max(axis=1), np.maximum(np.abs(r64[:, :3]).max(axis=1), np.abs(ct).max(axis=1)))
    else:
        dist = _dist_ext(src.reshape(-1, 9), ct)
        scale = np.maximum(np.maximum(np.abs(src).max(axis=1), np.abs(r64[:, :3]).max(axis=1)), np.abs(ct).max(axis=1))
    res = np.where(t == r64[:, 6], np.maximum(dist - r, L(0)), np.abs(dist - r)) / scale
    return np.where(hit, res, L(0)).astype(np.float64)


def check_cast(raw, ids, rays_, radii, marks, hits, brute, sphere, complete, tol, what, cap=0.02):
    """A sphere-cast walk against the brute force over the same sweep test (records by BVH-order prim). Everywhere: invalid rays give
    the miss record, a miss is the miss record, t >= the brute force's t, every hit is a real contact of ITS primitive (residual <=
    tol * scale, cast_residuals). On the rays of the mask `complete` (those for which the box test promises to lose nothing): no contact of the brute
    force is missed, and the records that differ there are at most `cap` = 2 % of the batch (test_walk_golden's differ.mean()), by at
    most 64 sqrt(eps) in t: the caps of test_sphere_cast_host.test_walk_golden. cap=None (the rays sent from afar through a scene without extent, where dozens of
    coincident or coplanar primitives are met within an ulp of one t and sphere_cast_body.inc promises the (t, index) argmin only for
    exact arithmetic): the share is returned, not capped; the gap and everything else still hold.
    -> (hits, differing records, largest residual / scale)."""
    dt = rays_.dtype.type
    hit, bhit = hits["prim"] != INVALID, brute["prim"] != INVALID
    bad = marks["invalid"]
    assert not hit[bad].any() and not bhit[bad].any(), what
    miss = ~hit
    assert hits["t"][miss].tobytes() == rays_[miss, 7].tobytes() and (hits["u"][miss] == 0).all() and (hits["v"][miss] == 0).all(), what
    ok = ~bad
    assert (hits["t"][ok] >= brute["t"][ok]).all(), what
    assert not (hit & ~bhit).any(), what                      # (the walk tests a subset of what the brute force tests)
    res = cast_residuals(raw, ids, rays_, radii, hits, sphere)
    assert (res <= tol).all(), (what, float(res.max()), int(np.argmax(res)))
    sel = complete & ok
    lost = sel & bhit & ~hit
    assert not lost.any(), (what, np.flatnonzero(lost)[:8])
    differ = sel & ((hits["prim"] != brute["prim"]) | (hits["t"] != brute["t"]))
    assert cap is None or differ.sum() <= cap * len(rays_), (what, int(differ.sum()), int(sel.sum()), len(rays_))
    both = differ & hit & bhit
    gap = np.abs(hits["t"][both].astype(np.float64) - brute["t"][both].astype(np.float64))
    assert (gap <= 64 * np.sqrt(np.finfo(dt).eps)).all(), (what, gap.max())
    return int(hit.sum()), int(differ.sum()), float(res.max())


def check_distance(q, lim, ordered_tris, hits, uv, brute, second, tol, what):
    """A tri_distance walk against the brute force over the same pair distance, with one max_distance per query: the checks of
    test_tri_distance_host.test_walk_against_brute_force. |t - t_brute| <= tol * scale; prim equal, or the runner-up no farther than
    the tolerance (either may then be reported), for at most 2 % of the queries; the record's t is the float64 distance of ITS pair
    within tol * scale; NaN and negative limits give the miss record with the limit's bits. (The golden test counts every query with
    a close runner-up; here exact copies of duplicated triangles tie on purpose, so the cap counts the queries that NEED the excuse.)
    -> (hits, queries that needed the excuse, largest |t - t64| / scale)."""
    from test_tri_distance_host import pair_scale, ref_dist64
    hit, bhit = hits["prim"] != INVALID, brute["prim"] != INVALID
    with np.errstate(invalid="ignore"):
        bad = ~(lim >= 0)
    assert not hit[bad].any() and hits["t"][bad].tobytes() == lim[bad].tobytes() and (uv[bad] == 0).all(), what
    assert not bhit[bad].any() and brute["t"][bad].tobytes() == lim[bad].tobytes(), what
    ok = ~bad
    tris = ordered_tris[np.where(hit, hits["prim"], 0).astype(np.int64)]
    btris = ordered_tris[np.where(bhit, brute["prim"], 0).astype(np.int64)]
    scale = np.maximum(pair_scale(q, tris), pair_scale(q, btris))
    gap = np.abs(hits["t"][ok].astype(np.float64) - brute["t"][ok].astype(np.float64))
    assert (gap <= tol * scale[ok]).all(), (what, float((gap / scale[ok]).max()))
    assert (hits["t"][ok & ~hit] == lim[ok & ~hit]).all() and (hits["u"][~hit] == 0).all() and (hits["v"][~hit] == 0).all() and (uv[~hit] == 0).all(), what
    both = ok & hit & bhit
    differ = ok & ((hit != bhit) | (both & (hits["prim"] != brute["prim"])))
    excused = second - brute["t"].astype(np.float64) <= tol * scale
    edge = np.abs(brute["t"].astype(np.float64) - lim.astype(np.float64)) <= tol * scale       # hit on one side, miss on the other: t is at the limit
    assert (~differ | np.where(hit == bhit, excused, edge)).all(), (what, np.flatnonzero(differ)[:8])
    assert differ.sum() <= 0.02 * len(q), (what, int(differ.sum()))
    err = np.abs(ref_dist64(q[hit], tris[hit]) - hits["t"][hit]) / scale[hit] if hit.any() else np.zeros(1)
    assert (err <= tol).all(), (what, float(err.max()))
    return int(hit.sum()), int(differ.sum()), float(err.max())


def check_region(tree, planes, got, exact, pairs_exact, what):
    """Count / fill results `got` = (offsets, ids, inside, counts) of a region walk against region_ref.brute_cull (and, for EXACT, the
    kernel's predicate on every pair CULL lets through, `pairs_exact(prims, planes) -> bool`): the assertions of
    test_region_host.test_walk_equals_brute_force, the sphere rule (a subset; what is lacking is within 16 u M of tangent) included.
    -> (listed, pairs in the brute force only)."""
    offsets, ids, ins, counts = got
    pr = tree.ordered()
    match, inside = region_ref.brute_cull(pr, planes)
    if exact:
        qi, pi = np.nonzero(match)
        match = match.copy()
        match[qi, pi] = pairs_exact(pr[pi], planes[qi])
        inside = inside & match
    only = 0
    if tree.leaf == 1:
        walk = np.zeros_like(match)
        walk[np.repeat(np.arange(len(planes)), counts), ids.astype(np.int64)] = True
        assert not (walk & ~match).any(), what
        qi, pi = np.nonzero(match & ~walk)
        only = len(qi)
        if only:
            p, p64 = pr.astype(np.float64)[pi], planes.astype(np.float64)[qi]
            s = np.einsum("kpc,kc->kp", p64[:, :, :3], p[:, :3]) + p64[:, :, 3]
            ln = np.linalg.norm(p64[:, :, :3], axis=2)
            big = (np.abs(p64[:, :, :3]) * (np.abs(p[:, None, :3]) + p[:, None, 3:4])).sum(axis=2) + np.abs(p64[:, :, 3])
            margin = p[:, 3:4] * ln - s
            assert ((margin <= 16 * np.finfo(tree.dtype).eps / 2 * big) & (ln > 0)).any(axis=1).all(), what
            match, inside = walk, inside & walk
    want_counts, want_ids = region_ref.expected_lists(match, tree.dfs)
    assert (counts == want_counts).all(), (what, int((counts != want_counts).sum()))
    assert ids.tobytes() == want_ids.tobytes(), what
    assert ins.tobytes() == region_ref.expected_inside(match, inside, tree.dfs).tobytes(), what
    assert (offsets == np.concatenate([[0], np.cumsum(want_counts.astype(np.uint64))])).all(), what
    return len(want_ids), only
