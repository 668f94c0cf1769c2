"""Shared by tests/test_refit_fuzz_host.py (CPU) and tests/test_gpu_refit_fuzz.py (-m gpu): the cases, the tree-aware moves and the
expectations of the refit from moved primitives (Bvh.refit_boxes / Bvh.refit_tris) on signed zeros, NaN, infinities, degenerate and
foreign geometry, on trees from one primitive to 1500.

The fold `acc < other ? acc : other` (refit_body.inc, the reference's robust_min with the accumulated value first) and the climb
`min(left, right)` select values and never compute them, so a planted np.nan comes through with its payload and every comparison of
nodes is on bytes. What makes the cases bite is WHERE a value sits in the tree: the last slot of a leaf, a left or a right child, the
leaf reached from the root by right children only. So a move sees the built tree.

The expectation is tests/test_gpu_refit_prims.py::expected_tree (the numpy model of the leaf fold, then the checker's own Bvh::refit).
Beside it, `refit_model` restates the whole refit in numpy with the selection rule as a parameter, for three WRONG rules a device
build could fall into without any test on ordinary numbers noticing; `witnesses` counts the node bounds each of them gets wrong."""
import functools

import numpy as np

import adversarial_queries as adv

MOVES = ("zeros", "nan_leaf", "nan_root", "inf", "collapse", "explode", "other_kind")
WRONG_MODELS = ("reversed", "ieee", "right_acc")
MAX_N = 1500                                                   # the smallest of adv.SIZES that gives a climb of real depth
KINDS3 = ("lattice", "dups", "flat", "scales", "uniform", "points_lattice", "spheres")
OTHER_KINDS = ("dups", "lattice", "scales", "points_lattice")
SEED3 = 6


def _cases3():
    return [(kind, min(n, MAX_N), lim, bq, dtype, seed) for kind, n, lim, bq, dtype, seed in adv.cases(SEED3, KINDS3, 20)]


CASES3 = _cases3()
# circles (Node<T, 2>): lattice centres, radius 0 included; the builders that exist in 2D
CASES2 = [("circles", 1, (1, 8), (2, 0), np.float32, 901), ("circles", 2, (1, 1), (0, 2), np.float64, 902),
          ("circles", 200, (9, 15), (0, 2), np.float32, 903), ("circles", 1500, (3, 15), (3, 0), np.float64, 904),
          ("circles", 65, (1, 1), (2, 0), np.float64, 905), ("circles", 17, (2, 4), (0, 1), np.float32, 906)]
CASES = CASES3 + CASES2


def dim_of(case):
    return 2 if case[0] == "circles" else 3


def is_tri(case):
    return case[0] not in ("spheres", "circles")


def salt_of(case):
    """The position of the case in its list: deals the NaN's column over the cases."""
    return case[5] % 100


def scene(case):
    kind, n, lim, bq, dtype, seed = case
    rng = np.random.default_rng(seed)
    if kind == "circles":
        ctr = rng.integers(0, 6, size=(n, 2)).astype(dtype)
        rad = rng.integers(0, 3, size=(n, 1)).astype(dtype) * dtype(0.25)
        return np.ascontiguousarray(np.concatenate([ctr, rad], axis=1))
    return adv.scene(rng, n, kind, dtype)


def bounds(orc, raw):
    """(boxes, centres) by the checker: Tri::get_bbox / get_center for (n, 9), Sphere's for (n, 4) spheres and (n, 3) circles."""
    return orc.prep_tris(raw) if raw.shape[1] == 9 else orc.sphere_bboxes(raw)


def sphere_boxes(sph):
    """Sphere::get_bbox in numpy: {centre - radius, centre + radius}, one rounding each."""
    d = sph.shape[1] - 1
    return np.ascontiguousarray(np.concatenate([sph[:, :d] - sph[:, d:], sph[:, :d] + sph[:, d:]], axis=1))


def moved_boxes(orc, moved):
    """The (n, 2 dim) boxes by original id a move stands for: a move of triangles returns triangles, every other move boxes."""
    return orc.prep_tris(moved)[0] if moved.shape[1] == 9 else moved


def checker_tree(orc, case):
    """(raw, nodes, prim_ids) of the checker's build with the case's builder, quality and leaf limits."""
    kind, n, lim, bq, dtype, seed = case
    raw = scene(case)
    bb, cc = bounds(orc, raw)
    t = orc.build(bb, cc, builder=bq[0], quality=bq[1], min_leaf=lim[0], max_leaf=lim[1])
    return raw, t.nodes(), t.prim_ids()


# ---- the tree as the moves see it -----------------------------------------------------------------------------------------------------

class Topology:
    """first / count per node, parent (-1: the root), is_left, depth, the leaves, the right spine (root, its right child, ...)."""

    def __init__(self, nodes):
        idx = nodes["index"].astype(np.uint64)
        n = len(nodes)
        self.count = (idx & np.uint64(15)).astype(np.int64)
        self.first = (idx >> np.uint64(4)).astype(np.int64)
        self.parent = np.full(n, -1, dtype=np.int64)
        self.is_left = np.zeros(n, dtype=bool)
        self.depth = np.full(n, -1, dtype=np.int64)
        self.depth[0] = 0
        todo = [0]
        while todo:                                            # (from the root: an optimized tree keeps no index order)
            i = todo.pop()
            if self.count[i] == 0:
                f = int(self.first[i])
                self.parent[f] = self.parent[f + 1] = i
                self.is_left[f] = True
                self.depth[f] = self.depth[f + 1] = self.depth[i] + 1
                todo += [f, f + 1]
        assert (self.depth >= 0).all()                         # every node of the array is reachable
        self.leaves = np.flatnonzero(self.count)
        self.spine = [0]
        while self.count[self.spine[-1]] == 0:
            self.spine.append(int(self.first[self.spine[-1]]) + 1)

    def slots(self, leaf):
        return range(int(self.first[leaf]), int(self.first[leaf] + self.count[leaf]))

    def last(self, leaf):
        return int(self.first[leaf] + self.count[leaf] - 1)

    def sibling_leaf_pairs(self):
        """Inner nodes both of whose children are leaves."""
        inner = np.flatnonzero(self.count == 0)
        f = self.first[inner]
        return inner[(self.count[f] > 0) & (self.count[f + 1] > 0)]


def move_rng(case, name):
    return np.random.default_rng([case[5], MOVES.index(name)])


# ---- the moves: (rng, raw, nodes, ids, kind, salt) -> (n, 9) triangles, or (n, 2 dim) boxes for spheres and circles --------------------

def _start(raw):
    """A working copy: triangles as (n, 3, 3), spheres and circles as their boxes; and the dimension."""
    if raw.shape[1] == 9:
        return raw.copy().reshape(-1, 3, 3), 3
    return sphere_boxes(raw), raw.shape[1] - 1


def _done(out):
    return np.ascontiguousarray(out.reshape(len(out), -1))


def zeros_plan(rng, nodes):
    """(axis draw, [(left leaf, right leaf)] up to two sibling pairs, up to two other leaves of two or more primitives)."""
    t = Topology(nodes)
    draw = int(rng.integers(0, 6))
    pairs = [int(i) for i in rng.permutation(t.sibling_leaf_pairs())[:2]]
    taken = {int(t.first[i]) + d for i in pairs for d in (0, 1)}
    big = [int(l) for l in rng.permutation(t.leaves) if t.count[l] >= 2 and int(l) not in taken][:2]
    return draw, [(int(t.first[i]), int(t.first[i]) + 1) for i in pairs], big


def move_zeros(rng, raw, nodes, ids, kind=None, salt=0):
    """One axis of every vertex (of both bounds of every box) is a zero of random sign. Then, where the tree has them: one pair of
    sibling leaves all +0 on the left and all -0 on the right, a second pair the other way round; one leaf of two or more whose last
    slot is -0 after a +0, a second leaf the other way round."""
    draw, pairs, big = zeros_plan(rng, nodes)
    t = Topology(nodes)
    out, dim = _start(raw)
    axis = draw % dim
    tri = out.ndim == 3
    dt = out.dtype.type
    signs = np.where(rng.random((len(out), 3 if tri else 2)) < 0.5, dt(0.0), -dt(0.0))
    if tri:
        out[:, :, axis] = signs
    else:
        out[:, axis], out[:, dim + axis] = signs[:, 0], signs[:, 1]

    def put(slot, negative):
        p = int(ids[slot])
        if tri:
            out[p, :, axis] = -dt(0.0) if negative else dt(0.0)
        else:
            out[p, axis] = out[p, dim + axis] = -dt(0.0) if negative else dt(0.0)

    for j, (l, r) in enumerate(pairs):
        for s in t.slots(l):
            put(s, j == 1)
        for s in t.slots(r):
            put(s, j == 0)
    for j, leaf in enumerate(big):
        put(t.last(leaf) - 1, j == 1)
        put(t.last(leaf), j == 0)
    return _done(out)


def nan_leaf_plan(rng, nodes):
    """(stays, vanishes, vanishes_in_the_triangle): three different leaves where the tree has them (None where it has no such leaf); the
    second has two or more slots."""
    t = Topology(nodes)
    order = [int(l) for l in rng.permutation(t.leaves)]
    stays = order[0]
    big = [l for l in order[1:] if t.count[l] >= 2]
    vanishes = big[0] if big else None
    rest = [l for l in order[1:] if l != vanishes]
    return stays, vanishes, (rest[0] if rest else vanishes)    # (two leaves in all: the last slot of the second serves)


def _box_slot(col, dim):
    """The node-layout slot {min.x, max.x, min.y, ...} of input column `col` of {min, max}."""
    return (col % dim) * 2 + col // dim


def move_nan_leaf(rng, raw, nodes, ids, kind=None, salt=0):
    """A NaN in the last slot of one leaf (it stays), one in the first slot of another leaf of two or more (the next primitive
    replaces it). Boxes: in column salt % (2 dim) and the next one. Triangles: through p2 (Tri::get_bbox keeps it, in the minimum and
    the maximum of that axis), and in p0 or p1 of the last slot of a third leaf (the triangle's own fold drops it)."""
    stays, vanishes, in_tri = nan_leaf_plan(rng, nodes)
    t = Topology(nodes)
    out, dim = _start(raw)
    if out.ndim == 3:
        axis = salt % 3
        out[int(ids[t.last(stays)]), 2, axis] = np.nan
        if vanishes is not None:
            out[int(ids[t.first[vanishes]]), 2, (axis + 1) % 3] = np.nan
        if in_tri is not None:
            out[int(ids[t.last(in_tri)]), (salt // 3) % 2, (axis + 2) % 3] = np.nan
    else:
        col = salt % (2 * dim)
        out[int(ids[t.last(stays)]), col] = np.nan
        if vanishes is not None:
            out[int(ids[t.first[vanishes]]), (col + 1) % (2 * dim)] = np.nan
    return _done(out)


def nan_root_plan(rng, nodes):
    """(the leaf reached from the root by right children only, a leaf that is a left child of a node off that path or None)."""
    t = Topology(nodes)
    spine = set(t.spine)
    left = [int(l) for l in rng.permutation(t.leaves) if t.is_left[l] and int(t.parent[l]) not in spine]
    return t.spine[-1], (left[0] if left else None)


def nan_root_columns(case):
    """(column of the NaN that reaches the root, column of the one that stops): triangles: axes; boxes: columns of {min, max}."""
    salt = salt_of(case)
    if is_tri(case):
        return salt % 3, (salt + 1) % 3
    d = dim_of(case)
    return salt % (2 * d), (salt + d) % (2 * d)


def move_nan_root(rng, raw, nodes, ids, kind=None, salt=0):
    """A NaN in the last slot of the rightmost leaf: every climb step takes it from the right child, up to the root. A second one in
    the last slot of a left child elsewhere: its parent takes the right child's value instead."""
    right, left = nan_root_plan(rng, nodes)
    t = Topology(nodes)
    out, dim = _start(raw)
    if out.ndim == 3:
        out[int(ids[t.last(right)]), 2, salt % 3] = np.nan
        if left is not None:
            out[int(ids[t.last(left)]), 2, (salt + 1) % 3] = np.nan
    else:
        out[int(ids[t.last(right)]), salt % (2 * dim)] = np.nan
        if left is not None:
            out[int(ids[t.last(left)]), (salt + dim) % (2 * dim)] = np.nan
    return _done(out)


def move_inf(rng, raw, nodes, ids, kind=None, salt=0):
    """About 5 % of the coordinates +inf or -inf (one at least); boxes also get about 5 % empty ones, {+max, -max} as
    BBox::make_empty() writes them."""
    out, dim = _start(raw)
    flat = out.reshape(len(out), -1)
    mask = rng.random(flat.shape) < 0.05
    mask[int(rng.integers(0, len(flat))), int(rng.integers(0, flat.shape[1]))] = True
    flat[mask] = np.where(rng.random(int(mask.sum())) < 0.5, np.inf, -np.inf).astype(flat.dtype)
    if out.ndim == 2:
        fmax = np.finfo(out.dtype).max
        empty = rng.random(len(out)) < 0.05
        out[empty, :dim], out[empty, dim:] = fmax, -fmax
    return _done(out)


def collapsed_spheres(rng, raw):
    """Every sphere / circle at one lattice point with radius 0."""
    d = raw.shape[1] - 1
    one = np.zeros(d + 1, dtype=raw.dtype)
    one[:d] = rng.integers(0, 5, size=d)
    return np.ascontiguousarray(np.tile(one, (len(raw), 1)))


def move_collapse(rng, raw, nodes, ids, kind=None, salt=0):
    """Every primitive at one lattice point: a root box of zero extent on all axes."""
    if raw.shape[1] != 9:
        return sphere_boxes(collapsed_spheres(rng, raw))
    return np.ascontiguousarray(np.tile(rng.integers(0, 5, size=3).astype(raw.dtype), (len(raw), 3)))


def exploded(raw):
    """The scene itself, translated by ten times its extent."""
    d = 3 if raw.shape[1] == 9 else raw.shape[1] - 1
    pts = raw.reshape(-1, 3) if raw.shape[1] == 9 else raw[:, :d]
    shift = (10.0 * (pts.max(axis=0).astype(np.float64) - pts.min(axis=0).astype(np.float64))).astype(raw.dtype)
    out = raw.copy()
    if raw.shape[1] == 9:
        out = (out.reshape(-1, 3, 3) + shift).reshape(-1, 9)
    else:
        out[:, :d] += shift
    return np.ascontiguousarray(out.astype(raw.dtype))


def move_explode(rng, raw, nodes, ids, kind=None, salt=0):
    out = exploded(raw)
    return out if raw.shape[1] == 9 else sphere_boxes(out)


def sphere_source(case, name, raw):
    """The spheres / circles whose Sphere::get_bbox the `collapse` and `explode` moves of a sphere family return (None otherwise):
    what the device's sphere_bounds is fed."""
    if raw.shape[1] == 9 or name not in ("collapse", "explode"):
        return None
    return collapsed_spheres(move_rng(case, name), raw) if name == "collapse" else exploded(raw)


def move_other_kind(rng, raw, nodes, ids, kind=None, salt=0):
    """The geometry of another adv.scene kind on the topology of the built one."""
    pick = [k for k in OTHER_KINDS if k != kind]
    tris = adv.scene(rng, len(raw), pick[int(rng.integers(0, len(pick)))], raw.dtype.type)
    if raw.shape[1] == 9:
        return tris
    d = raw.shape[1] - 1
    v = tris.reshape(-1, 3, 3)[:, :, :d]
    return np.ascontiguousarray(np.concatenate([v.min(axis=1), v.max(axis=1)], axis=1))


MOVE_FUNCTIONS = {"zeros": move_zeros, "nan_leaf": move_nan_leaf, "nan_root": move_nan_root, "inf": move_inf, "collapse": move_collapse,
                  "explode": move_explode, "other_kind": move_other_kind}


def apply(case, name, raw, nodes, ids):
    """Move `name` of the case on the tree (nodes, ids): seeded by the case and the move, so every caller gets the same array."""
    return MOVE_FUNCTIONS[name](move_rng(case, name), raw, nodes, ids, kind=case[0], salt=salt_of(case))


def finite_extent(moved, dim):
    """(lo, hi) in float64 over the finite coordinates of a moved array, per axis; (0, 1) on an axis that has none."""
    pts = moved.reshape(-1, 3) if moved.shape[1] == 9 else moved.reshape(-1, dim)
    big = np.finfo(moved.dtype).max
    p = np.where(np.isfinite(pts) & (np.abs(pts) < big), pts, np.nan).astype(np.float64)
    some = np.isfinite(p).any(axis=0)
    with np.errstate(all="ignore"):
        lo = np.where(some, np.nanmin(np.where(some, p, 0.0), axis=0), 0.0)
        hi = np.where(some, np.nanmax(np.where(some, p, 1.0), axis=0), 1.0)
    return lo, hi


# ---- the refit in numpy, with the selection rule as a parameter -----------------------------------------------------------------------

def _min_ref(acc, other):
    return np.where(acc < other, acc, other)                   # robust_min(acc, other): the reference's, and refit_body.inc's


def _max_ref(acc, other):
    return np.where(acc > other, acc, other)


def _min_reversed(acc, other):
    return np.where(other < acc, other, acc)                   # (a): the comparison the other way round


def _max_reversed(acc, other):
    return np.where(other > acc, other, acc)


def _min_ieee(acc, other):
    tie = acc == other                                         # (b): minNum — the non-NaN operand wins, -0 < +0
    return np.where(tie, np.where(np.signbit(acc), acc, other), np.fmin(acc, other))


def _max_ieee(acc, other):
    tie = acc == other
    return np.where(tie, np.where(np.signbit(acc), other, acc), np.fmax(acc, other))


RULES = {"reference": (_min_ref, _max_ref, False), "reversed": (_min_reversed, _max_reversed, False), "ieee": (_min_ieee, _max_ieee, False),
         "right_acc": (_min_ref, _max_ref, True)}              # (c): the reference's rule, the right child as accumulator in the climb


def refit_model(nodes, ids, bb, dim, rule="reference"):
    """The node array after a refit from boxes `bb` under `rule`: the leaf fold in slot order from BBox::make_empty(), then every
    inner box from its children, deepest level first."""
    fmin, fmax, swap = RULES[rule]
    t = Topology(nodes)
    out = nodes.copy()
    big = np.finfo(bb.dtype).max
    leaves = t.leaves
    lo = np.full((len(leaves), dim), big, bb.dtype)
    hi = np.full((len(leaves), dim), -big, bb.dtype)
    with np.errstate(invalid="ignore"):
        for k in range(int(t.count.max())):
            ok = (t.count[leaves] > k)[:, None]
            p = ids[np.minimum(t.first[leaves] + k, len(ids) - 1)].astype(np.int64)
            lo = np.where(ok, fmin(lo, bb[p, :dim]), lo)
            hi = np.where(ok, fmax(hi, bb[p, dim:]), hi)
        b = out["bounds"]
        b[leaves, 0::2], b[leaves, 1::2] = lo, hi
        for depth in range(int(t.depth.max()) - 1, -1, -1):
            inner = np.flatnonzero((t.depth == depth) & (t.count == 0))
            l, r = b[t.first[inner]], b[t.first[inner] + 1]
            acc, other = (r, l) if swap else (l, r)
            b[inner, 0::2] = fmin(acc[:, 0::2], other[:, 0::2])
            b[inner, 1::2] = fmax(acc[:, 1::2], other[:, 1::2])
    return out


def differing_bounds(a, b):
    """How many node bounds of two node arrays differ bytewise."""
    u = np.uint32 if a["bounds"].dtype == np.float32 else np.uint64
    return int((np.ascontiguousarray(a["bounds"]).view(u) != np.ascontiguousarray(b["bounds"]).view(u)).sum())


@functools.lru_cache(maxsize=None)
def _checker():
    import oracle
    return oracle.load_oracle()


def witnesses(case, orc=None, moves=MOVES):
    """{move: {wrong model: node bounds that differ bytewise from the expectation}} on the checker's tree of the case. The
    expectation is expected_tree (the checker's own Bvh::refit); refit_model under the reference's rule must reproduce it."""
    from test_gpu_refit_prims import expected_tree
    orc = orc or _checker()
    raw, nodes, ids = checker_tree(orc, case)
    dim = dim_of(case)
    out = {}
    for name in moves:
        bb = moved_boxes(orc, apply(case, name, raw, nodes, ids))
        want = expected_tree(orc, nodes, ids, bb, dim).nodes()
        assert differing_bounds(refit_model(nodes, ids, bb, dim), want) == 0, (adv.case_id(case), name)
        out[name] = {rule: differing_bounds(refit_model(nodes, ids, bb, dim, rule), want) for rule in WRONG_MODELS}
    return out
