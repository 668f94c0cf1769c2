"""Shared by tests/test_instanced_fuzz_host.py (CPU) and tests/test_gpu_instanced_fuzz.py (-m gpu): the adversarial two-level scenes of the
instanced ray queries, their rays, and the expectations that do not come from the kernel's own text.

Instance classes (CLASSES): benign, mirrored, exact powers of two, squashed (kappa ~ 1e3), uniform 1e-4 / 1e4, far (+1e4 per axis),
coincident groups, and about 10 % dead instances (zero determinant, a NaN entry, an infinite translation, a geometry index outside the
table). Existing generators keep their seeds: every generator here is handed its own rng.

Three expectations, strongest first (the fourth and fifth, the order-free and the one-sided properties under a built top tree, are
order_free, which restates test_instanced_host.check_order_free for grazing rays, and one_sided below):
 * the composition of the checker's single-level query in slot order (test_instanced_host.expect_single_leaf), bit for bit;
 * the exact tier, with neither the harness nor the checker: pow2 instances of lattice triangles (vertices on the integer lattice
   0..4), rays with quarter-lattice origins and directions in {-2..2}^3. Every operation before the division is exact in float and
   in double, so numpy in T with the kernel's operation order (exact_pairs) gives the kernel's bits; nothing is excluded;
 * the float64 flattened truth (float64_truth): every enabled instance's triangles carried to world space in float64, Moeller-Trumbore
   in float64 on the rays as given, and the rays on which float rounding may decide marked unclear by the margin M_UNCLEAR."""
import numpy as np

import oracle
import instanced_scenes as sc
from instanced_scenes import INVALID

M_UNCLEAR = 1e-3
RAY_COUNTS = (1, 63, 64, 65, 257, 1021)
FULL_BATCH = 1021
TOP_SIZES = (2, 5, 17, 65, 200)
TOP_LIMITS = ((1, 1), (9, 15))
ROUNDED_CLASSES = ("benign", "mirror", "squash", "huge_small", "far", "coincident")
TRUTH_CLASSES = ("benign", "mirror", "far")


# ---- instance classes: (rng, n, dtype) -> (n, 12) object-to-world matrices in float64, to be rounded to dtype by the caller ----------

def _spread(n):
    """Half-width of the cube the translations are drawn from: a few instances overlap, most do not."""
    return 1.5 * n ** (1.0 / 3.0) + 1.0


def benign(rng, n, dtype):
    return np.array([sc.affine(rng, rng.uniform(-_spread(n), _spread(n), size=3)) for _ in range(n)]).reshape(n, 12)


def mirror(rng, n, dtype):
    """benign with one or three axes negated: a negative determinant."""
    m = benign(rng, n, dtype).reshape(n, 3, 4)
    for k in range(n):
        signs = -np.ones(3) if rng.random() < 0.5 else np.roll([-1.0, 1.0, 1.0], int(rng.integers(0, 3)))
        m[k, :, :3] = m[k, :, :3] * signs
        assert np.linalg.det(m[k, :, :3]) < 0
    return m.reshape(n, 12)


def pow2(rng, n, dtype):
    """Signed axis permutations times powers of two within 2^-3..2^3 (per axis, at most a factor 2 apart within one instance), integer
    translations: the matrix, its inverse and the image of every lattice point are exact in float and in double."""
    m = np.zeros((n, 3, 4))
    for k in range(n):
        perm, base = rng.permutation(3), int(rng.integers(-3, 3))
        for row in range(3):
            m[k, row, perm[row]] = (-1.0 if rng.random() < 0.5 else 1.0) * 2.0 ** (base + int(rng.integers(0, 2)))
        m[k, :, 3] = rng.integers(-6, 7, size=3)
    return m.reshape(n, 12)


def squash(rng, n, dtype):
    """One object axis times 1e-3: kappa about 1e3."""
    m = benign(rng, n, dtype).reshape(n, 3, 4)
    for k in range(n):
        m[k, :, :3] = m[k, :, :3] @ np.diag(np.roll([1e-3, 1.0, 1.0], int(rng.integers(0, 3))))
    return m.reshape(n, 12)


def huge_small(rng, n, dtype):
    """Uniform scale 1e-4 or 1e4."""
    m = benign(rng, n, dtype).reshape(n, 3, 4)
    for k in range(n):
        m[k, :, :3] *= 1e4 if rng.random() < 0.3 else 1e-4
    return m.reshape(n, 12)


def far(rng, n, dtype):
    """The translation offset by 1e4 on every axis."""
    m = benign(rng, n, dtype).reshape(n, 3, 4)
    m[:, :, 3] += 1e4
    return m.reshape(n, 12)


def coincident(rng, n, dtype):
    """Groups of 2 to 4 instances with identical matrices (assign_geometries gives a group one geometry): ties in t."""
    m = benign(rng, n, dtype)
    k = 0
    while k < n:
        g = int(rng.integers(2, 5))
        m[k:k + g] = m[k]
        k += g
    return m


CLASSES = {"benign": benign, "mirror": mirror, "pow2": pow2, "squash": squash, "huge_small": huge_small, "far": far, "coincident": coincident}


def assign_geometries(rng, m, n_geoms, use_all=True):
    """A geometry index per instance: every table entry used where there are instances enough (the last one by the last instance),
    identical matrices next to each other share theirs."""
    n = len(m)
    gids = rng.integers(0, n_geoms, size=n).astype(np.uint32)
    if use_all and n >= n_geoms:
        gids[rng.permutation(n)[:n_geoms]] = np.arange(n_geoms, dtype=np.uint32)
    if use_all:
        gids[n - 1] = n_geoms - 1
    for k in range(1, n):
        if (m[k] == m[k - 1]).all():
            gids[k] = gids[k - 1]
    return gids


def kill(rng, m, gids, n_geoms, share=0.1, which=None):
    """`dead`: about `share` of the instances (or exactly `which`) get a zero determinant, a NaN entry, an infinite translation or a
    geometry index outside the table, in turn. -> the indices killed."""
    n = len(m)
    which = np.flatnonzero(rng.random(n) < share) if which is None else np.asarray(which)
    for j, k in enumerate(which):
        how = j % 4
        if how == 0:
            m[k, 4:7] = 0.0                                    # a zero row: determinant exactly 0
        elif how == 1:
            m[k, int(rng.integers(0, 12))] = np.nan
        elif how == 2:
            m[k, 3 + 4 * int(rng.integers(0, 3))] = np.inf if rng.random() < 0.5 else -np.inf
        else:
            gids[k] = n_geoms + int(rng.integers(0, 3)) * 1000
    return which


def instances(rng, n, dtype, kinds, n_geoms, dead=0.1):
    """n instances dealt round robin from the classes `kinds` (a coincident group stays together), then `dead` of them killed.
    -> (matrices (n, 12) in dtype, geometry indices, the indices killed)."""
    per = {k: CLASSES[k](rng, n, dtype) for k in kinds}
    m = np.zeros((n, 12))
    for k in range(n):
        m[k] = per[kinds[(k // 4) % len(kinds)]][k]
    gids = assign_geometries(rng, m, n_geoms)
    dead_ids = kill(rng, m, gids, n_geoms, dead) if dead else np.zeros(0, dtype=np.int64)
    alive = np.setdiff1d(np.arange(n), dead_ids)
    if len(alive) >= 2 * n_geoms:                              # every table entry by an instance that is alive (the last entry too)
        for g in range(n_geoms):
            if not (gids[alive] == g).any():
                counts = np.bincount(gids[alive], minlength=n_geoms)
                gids[alive[np.argmax(counts[gids[alive]])]] = g
    if len(alive) and not (gids[alive] == n_geoms - 1).any():
        gids[alive[-1]] = n_geoms - 1
    return m.astype(dtype), gids, dead_ids


# ---- geometries -----------------------------------------------------------------------------------------------------------------------

def leaf_geometry(orc, tris9):
    """A geometry whose root is a leaf of len(tris9) <= 15 triangles: one node, no pair record, BVH order = the given order."""
    tris9 = np.ascontiguousarray(tris9)
    assert 1 <= len(tris9) <= 15
    p = tris9.reshape(-1, 3)
    nodes = np.zeros(1, dtype=oracle.NODED if tris9.dtype == np.float64 else oracle.NODEF)
    lo, hi = p.min(axis=0), p.max(axis=0)
    nodes[0]["bounds"] = [lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]]
    nodes[0]["index"] = len(tris9)
    return sc.Geometry(orc, tris9, nodes, np.arange(len(tris9), dtype=np.uint64))


def random_tris(rng, n, dtype):
    """n ordinary triangles in the cube [-1, 1]^3, edges of about 0.8."""
    c = rng.uniform(-0.7, 0.7, size=(n, 1, 3))
    return np.clip(c + rng.uniform(-0.4, 0.4, size=(n, 3, 3)), -1, 1).reshape(n, 9).astype(dtype)


def degenerate_tris(rng, dtype):
    """40 triangles: ordinary ones, zero-area ones (a point three times; three points on a line) and exact duplicates of ordinary ones."""
    t = random_tris(rng, 40, dtype).reshape(40, 3, 3)
    t[5::8, 1] = t[5::8, 0]
    t[5::8, 2] = t[5::8, 0]                                     # a point
    t[6::8, 2] = t[6::8, 0] + 2 * (t[6::8, 1] - t[6::8, 0]) * dtype(0.25)    # on the line p0 p1
    t[7::8] = t[3::8]                                           # duplicates
    return np.ascontiguousarray(t.reshape(40, 9))


def lattice_tris(rng, n, dtype):
    """n triangles with vertices on the integer lattice 0..4, none of zero area asked for: some are (collinear draws), some coincide."""
    return rng.integers(0, 5, size=(n, 9)).astype(dtype)


def soup300(dtype):
    from bvh_amd import synth
    return sc.centred(synth.soup(300, seed=21, jitter=0.08, dtype=np.float64)).astype(dtype)


def tiny_geometries(orc, rng, dtype, soup=None):
    """Roots that are leaves of 1, 2 and 15 triangles, the degenerate geometry (the checker's default builder), the 300-triangle soup
    (`soup`: its Geometry on a tree from elsewhere, a device builder's for instance)."""
    return [leaf_geometry(orc, random_tris(rng, 1, dtype)), leaf_geometry(orc, random_tris(rng, 2, dtype)), leaf_geometry(orc, random_tris(rng, 15, dtype)),
            sc.Geometry(orc, degenerate_tris(rng, dtype)), soup if soup is not None else sc.Geometry(orc, soup300(dtype))]


def truth_geometries(orc, rng, dtype):
    """For the float64 tier (no exact duplicates: a tie in t is unclear by definition): the soup and leaves of 1 and 15 triangles."""
    return [sc.Geometry(orc, soup300(dtype)), leaf_geometry(orc, random_tris(rng, 1, dtype)), leaf_geometry(orc, random_tris(rng, 15, dtype))]


def table_of(geoms, count):
    """Exactly `count` table entries: the given geometries over and over (16 and 17 sit on either side of kInstSmallGeoms)."""
    return [geoms[k % len(geoms)] for k in range(count)]


# ---- top trees ------------------------------------------------------------------------------------------------------------------------

def two_leaf_top(scene):
    """A root with two leaves of one instance each."""
    assert scene.n == 2
    nodes = np.zeros(3, dtype=oracle.NODED if scene.double else oracle.NODEF)
    b = scene.bboxes
    box = lambda lo, hi: [lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]]
    nodes[0]["bounds"], nodes[0]["index"] = box(b[:, :3].min(axis=0), b[:, 3:].max(axis=0)), 1 << 4
    for k in range(2):
        nodes[1 + k]["bounds"], nodes[1 + k]["index"] = box(b[k, :3], b[k, 3:]), (k << 4) | 1
    scene.top_nodes, scene.top_ids = nodes, np.arange(2, dtype=np.uint64)
    return scene


def built_top(scene, orc, lim, bq):
    """The checker's builder `bq` = (builder, quality) with leaf limits `lim` over the instance boxes."""
    cpu = orc.build(scene.bboxes, scene.centers, builder=bq[0], quality=bq[1], min_leaf=lim[0], max_leaf=lim[1])
    scene.top_nodes, scene.top_ids = cpu.nodes(), cpu.prim_ids()
    return scene


def top_walk_counters(orc, scene, rays, any_hit, robust):
    """{pair records fetched, 0, leaves visited} of the top tree's walk when no instance can be hit: the checker's single-level walk of
    the top tree over zero triangles, on the rays that are not NaN-flagged (the instanced walk ends those before their first fetch)."""
    cpu = orc.from_arrays(scene.top_nodes, scene.top_ids)
    live = np.ascontiguousarray(rays[~sc.nan_flagged(rays)])
    hits, cnt = cpu.intersect_tri(np.zeros((len(scene.top_ids), 12), dtype=scene.dtype), live, any_hit, robust, counters=True)
    assert (hits["prim"] == INVALID).all()
    return np.array([cnt[0], 0, cnt[2]], dtype=np.uint64)


def top_leaves(scene):
    return int(((scene.top_nodes["index"].astype(np.uint64) & np.uint64(15)) != 0).sum())


# ---- rays -----------------------------------------------------------------------------------------------------------------------------

def special_rays(scene, n, seed, first_pass=None):
    """FULL_BATCH rays, of which a seeded choice of n is returned: 400 of scene_rays and 200 of centroid_rays, and copies of such rays with one, two and three
    zero direction components (+0.0 and -0.0; three: a null direction), a NaN direction component, the origin exactly on a plane of an
    instance's box and of a top node's box, tmin > tmax, tmax = 0, and tmin = tmax = the t of a hit that `first_pass` (rays -> hit
    records) reports for the ray."""
    rng = np.random.default_rng(seed)
    base = sc.scene_rays(scene, 400, seed + 1)
    if any(scene.enabled(i) for i in range(scene.n)):
        base = np.concatenate([base, centroid_rays(scene, rng, 200)])
    else:
        base = np.concatenate([base, sc.scene_rays(scene, 200, seed + 2)])
    usable = np.flatnonzero(np.isfinite(base[:, :6]).all(axis=1))                          # (the copies start from finite rays)
    extra = base[usable[rng.integers(0, len(usable), size=FULL_BATCH - 600)]].copy()
    extra[:, 6], extra[:, 7] = 0, np.inf
    kind = np.arange(len(extra)) % 10
    zero = lambda: scene.dtype.type(-0.0 if rng.random() < 0.5 else 0.0)
    for k in range(len(extra)):
        if kind[k] in (0, 1, 2):                               # one, two, three zero components
            for axis in rng.permutation(3)[:kind[k] + 1]:
                extra[k, 3 + axis] = zero()
        elif kind[k] == 3:
            extra[k, 3 + int(rng.integers(0, 3))] = np.nan
        elif kind[k] == 4:                                     # on a plane of an instance's box
            i, axis = int(rng.integers(0, scene.n)), int(rng.integers(0, 3))
            extra[k, axis] = scene.bboxes[i, axis + 3 * int(rng.integers(0, 2))]
        elif kind[k] == 5:                                     # on a plane of a top node's box (the root's where there is no other)
            node, axis = int(rng.integers(0, len(scene.top_nodes))), int(rng.integers(0, 3))
            extra[k, axis] = scene.top_nodes["bounds"][node][2 * axis + int(rng.integers(0, 2))]
        elif kind[k] == 6:
            extra[k, 6], extra[k, 7] = 2.0, 1.0
        elif kind[k] == 7:
            extra[k, 7] = 0.0
        # 8, 9: pinned below
    if first_pass is not None:
        pin = np.flatnonzero(kind >= 8)
        h = first_pass(extra[pin])
        got = h["prim"] != INVALID
        extra[pin[got], 6] = extra[pin[got], 7] = h["t"][got]
    full = np.concatenate([base, extra])
    return np.ascontiguousarray(full[np.sort(rng.permutation(FULL_BATCH)[:n])])


def centroid_rays(scene, rng, n):
    """Rays from 5 to 30 units away at the world images of triangle centroids of enabled instances: t is 0.5 to 2 there, and every ray
    hits something however small or large the instance is."""
    live = [i for i in range(scene.n) if scene.enabled(i)]
    r = np.zeros((n, 8), dtype=scene.dtype)
    for k in range(n):
        i = live[int(rng.integers(0, len(live)))]
        g = scene.geoms[scene.gid(i)]
        mat = scene.obj2world[i].astype(np.float64).reshape(3, 4)
        at = mat[:, :3] @ g.tris9[int(rng.integers(0, len(g.tris9)))].astype(np.float64).reshape(3, 3).mean(axis=0) + mat[:, 3]
        d = rng.normal(size=3)
        org = at - d / np.linalg.norm(d) * rng.uniform(5, 30)
        r[k, 0:3], r[k, 3:6], r[k, 7] = org, (at - org) * rng.uniform(0.5, 2.0), np.inf
    return r


def face_vertices(geom):
    """The vertices of a geometry that lie on a face of its root box, in float64."""
    v = np.unique(geom.tris9.reshape(-1, 3), axis=0)
    lo, hi = geom.root_box[0::2], geom.root_box[1::2]
    return v[((v == lo) | (v == hi)).any(axis=1)].astype(np.float64)


def grazing_rays(scene, rng, per_instance, distances=(30.0, 3000.0)):
    """Rays aimed at the world images of the vertices on the faces of the geometries' root boxes, `per_instance` per enabled instance,
    from the given distances in random directions: t = 1 at the vertex."""
    out = []
    for i in range(scene.n):
        if not scene.enabled(i):
            continue
        v = face_vertices(scene.geoms[scene.gid(i)])
        m = scene.obj2world[i].astype(np.float64).reshape(3, 4)
        at = v[rng.integers(0, len(v), size=per_instance)] @ m[:, :3].T + m[:, 3]
        d = rng.normal(size=(per_instance, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        org = at - d * np.asarray(distances)[rng.integers(0, len(distances), size=per_instance), None]
        r = np.zeros((per_instance, 8), dtype=scene.dtype)
        r[:, 0:3], r[:, 3:6], r[:, 7] = org, at - org, np.inf
        out.append(r)
    return np.concatenate(out)


def axis_rays(scene, rng, n, distance=20.0):
    """World rays along +-x, +-y, +-z (two direction components exactly zero, of either sign) from `distance` outside the scene's box,
    aimed at the instances' boxes."""
    lo, hi = scene.bboxes[:, :3].min(axis=0).astype(np.float64), scene.bboxes[:, 3:].max(axis=0).astype(np.float64)
    r = np.zeros((n, 8), dtype=scene.dtype)
    for k in range(n):
        axis, back = int(rng.integers(0, 3)), rng.random() < 0.5
        i = int(rng.integers(0, scene.n))
        org = scene.centers[i].astype(np.float64) + rng.normal(scale=0.3, size=3)
        org[axis] = hi[axis] + distance if back else lo[axis] - distance
        d = np.array([0.0 if rng.random() < 0.5 else -0.0] * 3)
        d[axis] = -1.0 if back else 1.0
        r[k, 0:3], r[k, 3:6] = org, d
    r[:, 7] = np.inf
    return r


def lattice_rays(rng, n, dtype):
    """The exact tier's rays: origins on the quarter lattice -8..8, directions with components in {-2, -1, 0, 1, 2} (-0.0 among the zeros,
    the null direction among them), tmin 0 or a quarter, tmax inf or a quarter-lattice value: hits exactly at tmin and tmax occur."""
    r = np.zeros((n, 8), dtype=dtype)
    r[:, 0:3] = rng.integers(-32, 33, size=(n, 3)) * 0.25
    d = rng.integers(-2, 3, size=(n, 3)).astype(dtype)
    d[(d == 0) & (rng.random((n, 3)) < 0.5)] = -0.0
    r[:, 3:6] = d
    r[:, 6] = np.where(rng.random(n) < 0.2, rng.integers(0, 9, size=n) * 0.25, 0.0)
    r[:, 7] = np.where(rng.random(n) < 0.3, rng.integers(0, 33, size=n) * 0.25, np.inf)
    return r


# ---- the exact tier: numpy in T, the kernel's operation order ------------------------------------------------------------------------

def _dot3(a0, a1, a2, b0, b1, b2):
    """trace_device.h's dot3: ((0 + a0 b0) + a1 b1) + a2 b2, one rounding per operation."""
    zero = np.asarray(a0).dtype.type(0)
    return ((zero + a0 * b0) + a1 * b1) + a2 * b2


def exact_inverse(obj2world):
    """The inverse of pow2 matrices in float64 by solving the permutation: exact, and independent of the kernel's adjugate."""
    out = np.zeros_like(obj2world, dtype=np.float64)
    for k, row in enumerate(obj2world.astype(np.float64)):
        m = row.reshape(3, 4)
        inv = np.zeros((3, 3))
        for r in range(3):
            (c,) = np.flatnonzero(m[r, :3])
            inv[c, r] = 1.0 / m[r, c]                          # (a power of two)
        out[k] = np.concatenate([inv, -(inv @ m[:, 3]).reshape(3, 1)], axis=1).reshape(12)
    return out


def exact_pairs(world2obj, tris9_list, gids, order, rays, dtype):
    """t, u, v, accepted for every (slot, triangle, ray) in dtype, by the kernel's order of operations: transform (dot3, + w), c = p0 -
    org, r = dir x c, 1 / dot3(n, dir), * inv_det, the closed -eps barycentric test, tmin <= t <= tmax. `order`: the instances in slot
    order; tris9_list[g]: the triangles of geometry g in BVH order. -> a list per slot of (instance, t, u, v, ok, intermediates), the
    arrays (triangles, rays); intermediates = the four values before the division, for the exactness assertion."""
    T = np.dtype(dtype).type
    rays = rays.astype(dtype)
    eps = T(np.finfo(dtype).eps)
    out = []
    with np.errstate(all="ignore"):
        for i in order:
            w = world2obj[i].astype(dtype)
            local = sc.transform_rays(w, rays)
            tri = tris9_list[int(gids[i])].astype(dtype).reshape(-1, 3, 3)
            p0, e1, e2 = tri[:, 0], tri[:, 0] - tri[:, 1], tri[:, 2] - tri[:, 0]
            n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
            col = lambda a, k: a[:, k][:, None]                 # (triangles, 1)
            org, d = local[None, :, 0:3], local[None, :, 3:6]   # (1, rays, 3)
            c0, c1, c2 = col(p0, 0) - org[..., 0], col(p0, 1) - org[..., 1], col(p0, 2) - org[..., 2]
            d0, d1, d2 = d[..., 0], d[..., 1], d[..., 2]
            rx, ry, rz = d1 * c2 - d2 * c1, d2 * c0 - d0 * c2, d0 * c1 - d1 * c0
            det = _dot3(col(n, 0), col(n, 1), col(n, 2), d0, d1, d2)
            inv_det = T(1) / det
            du, dv = _dot3(rx, ry, rz, col(e2, 0), col(e2, 1), col(e2, 2)), _dot3(rx, ry, rz, col(e1, 0), col(e1, 1), col(e1, 2))
            dt = _dot3(col(n, 0), col(n, 1), col(n, 2), c0, c1, c2)
            u, v = du * inv_det, dv * inv_det
            wv = T(1) - u - v
            t = dt * inv_det
            ok = (u >= -eps) & (v >= -eps) & (wv >= -eps) & (t >= rays[None, :, 6]) & (t <= rays[None, :, 7])
            out.append((int(i), t, u, v, ok, (det, du, dv, dt)))
    return out


def exact_expect(pairs, rays, any_hit):
    """The walk's result on root-leaf geometries under a single-leaf top tree from exact_pairs' arrays: the slots in order, within a slot
    the triangles in BVH order; an accepted t <= the running tmax takes over (so of equal t the LAST one tested stays); any-hit ends
    after the first slot with a hit (a leaf is always finished). -> (prim, instance, t, u, v), and per ray whether two different
    (slot, triangle) pairs share the winning t."""
    n = len(rays)
    prim, inst = np.full(n, INVALID, dtype=np.uint32), np.full(n, INVALID, dtype=np.uint32)
    t, u, v = rays[:, 7].copy(), np.zeros(n, dtype=rays.dtype), np.zeros(n, dtype=rays.dtype)
    tied = np.zeros(n, dtype=bool)
    live = ~sc.nan_flagged(rays)
    for i, pt, pu, pv, ok, _ in pairs:
        for k in range(pt.shape[0]):
            take = live & ok[k] & (pt[k] <= t)
            tied |= take & (prim != INVALID) & (pt[k] == t)
            tied &= ~(take & (pt[k] < t))
            prim[take], inst[take], t[take], u[take], v[take] = k, i, pt[k][take], pu[k][take], pv[k][take]
        if any_hit:
            live = live & (prim == INVALID)
    return prim, inst, t, u, v, tied


def assert_intermediates_exact(pairs32, pairs64):
    """The precondition of the exact tier: everything before the division has the same value in float and in double."""
    for a, b in zip(pairs32, pairs64):
        for x, y in zip(a[5], b[5]):
            assert x.dtype == np.float32 and y.dtype == np.float64
            assert (x.astype(np.float64) == y).all()


# ---- the float64 flattened truth ------------------------------------------------------------------------------------------------------

def world_triangles(scene):
    """Every enabled instance's triangles in world space, float64: (p0, p1, p2 (m, 3) each, instance (m,), original primitive id (m,))."""
    p, inst, prim = [], [], []
    for i in range(scene.n):
        if not scene.enabled(i):
            continue
        g = scene.geoms[scene.gid(i)]
        m = scene.obj2world[i].astype(np.float64).reshape(3, 4)
        p.append(g.tris9.astype(np.float64).reshape(-1, 3) @ m[:, :3].T + m[:, 3])
        inst.append(np.full(len(g.tris9), i, dtype=np.uint32))
        prim.append(np.arange(len(g.tris9), dtype=np.uint32))
    tri = np.concatenate(p).reshape(-1, 3, 3)
    return tri[:, 0], tri[:, 1], tri[:, 2], np.concatenate(inst), np.concatenate(prim)


def float64_truth(scene, rays, margin=M_UNCLEAR, chunk=48):
    """Moeller-Trumbore in float64 over all world triangles. -> (hit, instance, original primitive id, t, unclear). A ray is unclear if
    a triangle not farther than (1 + margin) times the best t (the ray's tmax on a miss) passes within `margin` (in barycentric units)
    of its own boundary, if the two nearest accepted t differ by less than `margin` relative, if a triangle the ray passes through lies
    within `margin` relative of tmin or tmax, or if the ray has a non-finite component (an infinite tmax aside)."""
    p0, p1, p2, t_inst, t_prim = world_triangles(scene)
    e1, e2 = p1 - p0, p2 - p0
    r64 = np.asarray(rays, dtype=np.float64)
    n = len(r64)
    hit, inst, prim = np.zeros(n, dtype=bool), np.full(n, INVALID, dtype=np.uint32), np.full(n, INVALID, dtype=np.uint32)
    best_t, unclear = r64[:, 7].copy(), np.zeros(n, dtype=bool)
    finite = np.isfinite(r64[:, :7]).all(axis=1) & ~np.isnan(r64[:, 7])
    with np.errstate(all="ignore"):
        for a in range(0, n, chunk):
            r = r64[a:a + chunk]
            o, d, tmin, tmax = r[:, None, 0:3], r[:, None, 3:6], r[:, None, 6], r[:, None, 7]
            pvec = np.cross(d, e2[None])
            det = (e1[None] * pvec).sum(axis=2)
            tvec = o - p0[None]
            u = (tvec * pvec).sum(axis=2) / det
            qvec = np.cross(tvec, e1[None])
            v = (d * qvec).sum(axis=2) / det
            t = (e2[None] * qvec).sum(axis=2) / det
            inside = np.minimum(np.minimum(u, v), 1.0 - u - v)  # > 0 inside the triangle, < 0 outside, ~0 on its boundary
            good = np.isfinite(t) & np.isfinite(inside)
            ok = good & (inside >= 0) & (t >= tmin) & (t <= tmax)
            tt = np.where(ok, t, np.inf)
            j = tt.argmin(axis=1)
            rows = np.arange(len(r))
            h = ok[rows, j]
            bt = np.where(h, tt[rows, j], r[:, 7])
            hit[a:a + chunk], best_t[a:a + chunk] = h, bt
            inst[a:a + chunk], prim[a:a + chunk] = np.where(h, t_inst[j], INVALID), np.where(h, t_prim[j], INVALID)
            reach = good & (t >= tmin - margin * np.abs(tmin)) & (t <= (bt + margin * np.abs(bt))[:, None])
            edge = (reach & (np.abs(inside) <= margin)).any(axis=1)
            tt[rows, j] = np.inf
            second = tt.min(axis=1)
            close = h & (second - bt <= margin * np.abs(bt))
            through = good & (inside >= -margin)
            near_end = (np.abs(t - tmin) <= margin * np.abs(tmin)) | (np.isfinite(tmax) & (np.abs(t - tmax) <= margin * np.abs(tmax)))
            ends = (through & near_end).any(axis=1)
            unclear[a:a + chunk] = edge | close | ends
    unclear |= ~finite
    return hit, inst, prim, best_t, unclear


def truth_mismatch(truth, hits, inst):
    """The clear rays on which records traced with ORIGINAL_IDS differ from float64_truth in hit or miss, instance or primitive."""
    hit, t_inst, t_prim, _, unclear = truth
    got_hit = hits["prim"] != INVALID
    return ~unclear & ((got_hit != hit) | (hit & ((inst != t_inst) | (hits["prim"] != t_prim))))


def check_against_truth(truth, hits, inst, what, excused=None):
    """Records traced with ORIGINAL_IDS against float64_truth on the clear rays (but the `excused` ones): hit or miss, instance and
    primitive exactly. -> (the worst relative error in t over the clear hits, the unclear share)."""
    hit, _, _, t, unclear = truth
    bad = truth_mismatch(truth, hits, inst)
    if excused is not None:
        bad &= ~excused
    assert not bad.any(), (what, np.flatnonzero(bad)[:8])
    sel = ~unclear & hit & (hits["prim"] != INVALID)
    if excused is not None:
        sel &= ~excused
    assert sel.sum() >= 0.2 * len(hit), (what, int(sel.sum()))
    err = np.abs(hits["t"][sel].astype(np.float64) - t[sel]) / np.abs(t[sel])
    return float(err.max()), float(unclear.mean())


# ---- a built top tree, robust mode: the order-free properties ---------------------------------------------------------------------------

def order_free(orc, scene, rays, got, inst, got_any, inst_any):
    """The properties of test_instanced_host.check_order_free for closest-hit records `got` and any-hit records `got_any` of a robust
    walk, with two differences that the grazing rays force. The precondition is checked here: the box-free composition forwards and
    backwards hits the same rays, and t is compared where the two agree on it (everywhere, unless a genuine tie between instances
    lets the order decide which of two equal hits ends the other's interval; at least 99 % of the rays). And a reported instance is
    re-evaluated alone with the RAY'S OWN tmax, not with tmax = the reported t: a hit on a face of its geometry's root box, which is
    where the grazing rays aim, has an entry parameter that can round above its own t, and the single-level query then culls the box
    it was found in (the reference does the same). -> the number of rays that hit."""
    from test_instanced_host import single_triangle_records
    forward, _, _ = sc.compose(scene, rays, range(scene.n), False, True)
    backward, _, _ = sc.compose(scene, rays, range(scene.n - 1, -1, -1), False, True)
    hit = forward["prim"] != INVALID
    assert ((backward["prim"] != INVALID) == hit).all()
    same = (forward["t"] == backward["t"]) | (np.isnan(forward["t"]) & np.isnan(backward["t"]))
    assert same.mean() >= 0.99
    assert np.ascontiguousarray(got["t"][same]).tobytes() == np.ascontiguousarray(forward["t"][same]).tobytes()
    lower = np.minimum(forward["t"], backward["t"])
    assert (got["t"][~same] >= lower[~same]).all()
    assert ((got["prim"] != INVALID) == hit).all() and ((inst != INVALID) == hit).all()
    assert (got["u"][~hit] == 0).all() and (got["v"][~hit] == 0).all()
    for i in np.unique(inst[hit]):
        idx = np.flatnonzero(hit & (inst == i))
        alone, alone_inst, _ = sc.compose(scene, rays[idx], [int(i)], False, True)
        assert (alone_inst == i).all() and sc.same_records(alone, got[idx]), i
    hit_any = got_any["prim"] != INVALID
    assert (hit_any == hit).all() and ((inst_any != INVALID) == hit).all()
    idx = np.flatnonzero(hit_any)
    single = single_triangle_records(orc, scene, rays[idx], inst_any[idx], got_any["prim"][idx], True)
    assert (single["prim"] == 0).all()
    for f in ("t", "u", "v"):
        assert single[f].tobytes() == np.ascontiguousarray(got_any[f][idx]).tobytes(), f
    assert np.ascontiguousarray(got_any["t"][~hit_any]).tobytes() == np.ascontiguousarray(rays[~hit_any, 7]).tobytes()
    return int(hit.sum())


# ---- a built top tree, fast mode: the one-sided contract ------------------------------------------------------------------------------

def order_insensitive(scene, rays):
    """The rays on which the box-free closest-hit composition gives one t forwards and backwards, in robust and in fast mode."""
    t = [sc.compose(scene, rays, order, False, robust)[0]["t"] for robust in (True, False) for order in (range(scene.n), range(scene.n - 1, -1, -1))]
    with np.errstate(invalid="ignore"):
        return np.all([(x == t[0]) | (np.isnan(x) & np.isnan(t[0])) for x in t[1:]], axis=0)


def one_sided(orc, scene, rays, common, got, inst, robust, what, stable=None):
    """What a fast-mode walk under a built top tree must keep even where its boxes cull: every reported hit is that (instance,
    triangle)'s own evaluation byte for byte, a ray the box-free composition `common` misses is missed, and t is never below the
    composition's on the rays `stable` (order_insensitive; all rays if None). `common` is the ROBUST composition in forward order. The
    restriction is needed because the geometry trees' own box tests, fast and robust, can cull a box whose entry parameter rounds
    above the t of a hit on its face once tmax has come down to that t: which hits a composition keeps then depends on the tmax an
    instance is entered with, that is on the order (seen: the fast composition forwards and backwards differ on a squashed scene;
    a fast walk found a hit nearer than the robust forward composition's on a scene of 1e4 / 1e-4 scales).
    -> (the hits of the composition that the walk lost, the composition's hits)."""
    from test_instanced_host import single_triangle_records
    want_hit, got_hit = common["prim"] != INVALID, got["prim"] != INVALID
    assert not (got_hit & ~want_hit).any(), what
    assert ((inst != INVALID) == got_hit).all(), what
    sel = got_hit if stable is None else got_hit & stable
    assert (got["t"][sel] >= common["t"][sel]).all(), what
    assert got["t"][~got_hit].tobytes() == np.ascontiguousarray(rays[~got_hit, 7]).tobytes(), what
    idx = np.flatnonzero(got_hit)
    single = single_triangle_records(orc, scene, rays[idx], inst[idx], got["prim"][idx], robust)
    assert (single["prim"] == 0).all(), what
    for f in ("t", "u", "v"):
        assert single[f].tobytes() == np.ascontiguousarray(got[f][idx]).tobytes(), (what, f)
    return int((want_hit & ~got_hit).sum()), int(want_hit.sum())


# ---- deep stacks: a chain-shaped top tree over instances of a chain-shaped geometry ---------------------------------------------------

CHAIN_CASES = ((7, 3), (8, 3), (63, 2), (64, 2), (31, 32), (32, 32), (70, 70))


def chain_top_scene(dll, orc, top_depth, geom_depth, n_rays, seed=None):
    """test_closest_point_host.chain_tree's node layout twice: as the geometry (depth geom_depth, its triangles shifted to x in
    [0, geom_depth]) and as the top tree over top_depth + 1 instances, instance k at x = X - k with the geometry squeezed into half a
    unit of x. Rays from x < 0 going +x: the deepest instance and in it the deepest triangle are the nearest, so closest-hit stacks
    top_depth top leaves, then the marker (at stack height top_depth), then geom_depth entries. -> (scene, rays, the spill's deep_cap
    as the host computes it, the closest-hit order of the instances)."""
    from test_closest_point_host import chain_tree
    tris, nodes, ids = chain_tree(geom_depth, orc.prep_tris)
    shift = np.float32(4000 - geom_depth)                      # (integers below 2^24: exact)
    tris = tris.copy()
    tris[:, 0::3] -= shift
    nodes = nodes.copy()
    nodes["bounds"][:, 0:2] -= shift
    geom = sc.Geometry(orc, tris, nodes, ids)
    n = top_depth + 1
    m = np.zeros((n, 3, 4))
    m[:, 0, 0], m[:, 1, 1], m[:, 2, 2] = 0.5 / geom_depth, 1.0, 1.0
    m[:, 0, 3] = (n + 4) - np.arange(n)
    scene = sc.Scene(dll, [geom], m.reshape(n, 12).astype(np.float32), None)
    _, top, _ = chain_tree(top_depth, lambda _t: (scene.bboxes, None))
    scene.top_nodes, scene.top_ids = top, np.arange(n, dtype=np.uint64)
    assert scene.top_depth() == top_depth
    rng = np.random.default_rng(1000 * top_depth + geom_depth if seed is None else seed)
    rays = np.zeros((n_rays, 8), dtype=np.float32)
    rays[:, 0] = -1.0 - 99.0 * rng.random(n_rays)
    rays[:, 1:3] = (rng.random((n_rays, 2)) - 0.5) * 1.2
    rays[:, 3], rays[:, 4], rays[:, 5] = 1.0, 2e-4 + rng.uniform(-1e-4, 1e-4, n_rays), -2e-4 + rng.uniform(-1e-4, 1e-4, n_rays)
    rays[:, 7] = np.inf
    bound = top_depth + 1 + geom_depth
    return scene, rays, (bound - 64 + 1 if bound > 64 else 0), list(range(n - 1, -1, -1))
