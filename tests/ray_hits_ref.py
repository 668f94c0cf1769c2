"""What the all-hits ray tests (tests/test_ray_hits_host.py, tests/test_gpu_ray_hits.py) share: dense scenes and rays, and the expected
hit lists, obtained from the UNMODIFIED reference without a leaf callback of our own.

For each BVH-order primitive i the reference's closest-hit intersect runs on the real tree with a primitive array that is all NaN
except entry i. A NaN PrecomputedTri or sphere can never be hit, so the walk never shortens the ray before it meets i: it reports i
exactly when i's leaf is reachable under the full [tmin, tmax] and the leaf test passes, and the (t, u, v) it returns are the
reference's own. The list of a ray is those primitives in the order of the left-first depth-first walk."""
import numpy as np

import oracle

INVALID = 0xFFFFFFFF


def reference_lib():
    """The compiled, unmodified reference where it is in the tree, else its restatement (pinned to the reference's golden vectors)."""
    return oracle.gpu_checker()


def dfs_prim_order(index):
    """BVH-order primitive indices in the order of a depth-first walk that takes a node's left child (first_id) before its right."""
    index = np.asarray(index).astype(np.uint64)
    out, stack = [], [0]
    while stack:
        w = int(index[stack.pop()])
        first, count = w >> 4, w & 15
        if count:
            out.extend(range(first, first + count))
        else:
            stack.append(first + 1)
            stack.append(first)
    return np.array(out, dtype=np.int64)


def dense_tris(n, seed, dtype=np.float32):
    """n large triangles with vertices anywhere in the unit cube: a ray through the cube crosses many of them."""
    rng = np.random.default_rng(seed)
    return rng.random((n, 9)).astype(dtype)


def dense_spheres(n, seed, dtype=np.float64):
    """n spheres in the unit cube with radii of 0.1 - 0.3: they overlap heavily."""
    rng = np.random.default_rng(seed)
    s = rng.random((n, 4))
    s[:, 3] = 0.1 + 0.2 * s[:, 3]
    return s.astype(dtype)


def points_on(raw, n, seed):
    """n points on randomly chosen primitives: inside a triangle (9 columns), or the centre of a sphere (4 columns)."""
    rng = np.random.default_rng(seed)
    raw = np.asarray(raw, np.float64)
    pick = raw[rng.integers(0, len(raw), n)]
    if raw.shape[1] == 4:
        return pick[:, :3]
    w = rng.dirichlet(np.ones(3), n)
    return (pick.reshape(n, 3, 3) * w[:, :, None]).sum(axis=1)


def rays_through(lo, hi, n, seed, dtype, targets=None):
    """n rays {org, dir, tmin, tmax} from a sphere around the box [lo, hi] through random points inside it (or through `targets`, n
    points), tmax beyond the far side; every fourth ray starts INSIDE the box, every fifth has tmin > 0 and a tmax that ends inside."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c, ext = (lo + hi) / 2, np.maximum(hi - lo, 1e-3)
    diag = float(np.linalg.norm(ext))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    org = c + 1.2 * diag * d
    org[::4] = lo + rng.random((len(org[::4]), 3)) * ext
    target = lo + rng.random((n, 3)) * ext if targets is None else np.asarray(targets, np.float64)
    r = np.zeros((n, 8))
    r[:, :3] = org
    r[:, 3:6] = target - org                                    # not normalised: t = 1 at the target
    r[:, 6] = 0.0
    r[:, 7] = 4.0
    r[::5, 6] = 0.5
    r[::5, 7] = 1.0 + 0.5 * rng.random(len(r[::5]))
    return r.astype(dtype)


def build_tree(lib, raw, sphere):
    """The reference's default build over the primitives -> (nodes, prim ids, BVH-order prims)."""
    bb, cc = lib.sphere_bboxes(raw) if sphere else lib.prep_tris(raw)
    bvh = lib.build(bb, cc)
    nodes, ids = bvh.nodes(), bvh.prim_ids()
    prims = np.ascontiguousarray(raw[ids.astype(np.int64)]) if sphere else lib.precompute_tris(raw, ids)
    return nodes, ids, prims


def reference_records(lib, nodes, prims, rays, leaf, robust):
    """(hit (n_prims, n_rays) bool, rec (n_prims, n_rays) hit records): what the reference's intersect reports for every BVH-order
    primitive alone in the real tree."""
    n = len(prims)
    bvh = lib.from_arrays(np.ascontiguousarray(nodes), np.arange(n, dtype=np.uint64))
    masked = np.full_like(prims, np.nan)
    hit = np.zeros((n, len(rays)), dtype=bool)
    rec = None
    fn = bvh.intersect_sphere if leaf else bvh.intersect_tri
    for i in range(n):
        masked[i] = prims[i]
        out = fn(masked, rays, any_hit=False, robust=robust)
        masked[i] = np.nan
        if "pad" in out.dtype.names:
            out["pad"] = 0                                      # (the record's padding word carries nothing; the library writes 0)
        if rec is None:
            rec = np.zeros((n, len(rays)), dtype=out.dtype)
        h = out["prim"] != INVALID
        assert (out["prim"][h] == i).all()
        hit[i], rec[i] = h, out
    return hit, rec


def expected_lists(hit, rec, index, prim_ids=None):
    """-> (counts (n_rays,) uint32, records of all rays back to back in walk order). prim_ids: the records' prim mapped through it."""
    dfs = dfs_prim_order(index)
    assert len(dfs) == hit.shape[0] and len(set(dfs.tolist())) == len(dfs)
    h, r = hit[dfs].T, rec[dfs].T                               # (n_rays, n_prims in walk order)
    counts = h.sum(axis=1).astype(np.uint32)
    flat = np.ascontiguousarray(r[h])
    if prim_ids is not None:
        flat["prim"] = np.asarray(prim_ids)[flat["prim"].astype(np.int64)].astype(np.uint32)
    return counts, flat
