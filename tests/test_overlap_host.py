"""CPU: the TEXT of the box-overlap kernel (bvh_amd/csrc/overlap_body.inc + list_walk.inc + point_walk.inc + trace_device.h) compiled for the host by
tests/cpp/overlap_body_host.cpp. The walk over the golden trees against a numpy brute force (the closed-interval test in the scene's
scalar type, mapped to BVH order through prim_ids and listed in the tree's left-first depth-first order): EXACT equality, nothing
excluded. The shapes of the output (count pass, exact offsets, fixed segments, padding, guard zones); self mode and its pair totals;
edge boxes; a loose tree; trees deeper than 64 levels; the exported symbols. The device's counts, lists and counters must equal this
harness's byte for byte (tests/test_gpu_overlap.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden, parse_stream
from test_closest_point_host import GOLDEN_SCENES, chain_tree, scene_queries
from test_kernel_body_host import _aligned, pair_records
from test_radius_search_host import GUARD, INVALID, SENT_PRIM, _p, dfs_prim_order, guards_intact

HARNESS = os.path.join(ROOT, "tests", "cpp", "overlap_body_host.cpp")
TREES = ["binned", "parallel_high"]
# numpy, closed intervals, over the scenes' own boxes: unordered overlapping pairs, and how many of them merely touch (they overlap
# with closed intervals and not with open ones)
SELF_PAIRS = {"cornell": 197, "soup2k": 400, "terrain2k": 15453, "soup2k_f64": 400, "spheres2k_f64": 2364}
TOUCHING_PAIRS = {"cornell": 166, "terrain2k": 14429}


def compile_harness(out_dir):
    out = os.path.join(str(out_dir), "liboverlap_body_host.so")
    cmd = ["g++", "-std=c++20", "-O1", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-strict-aliasing", "-Wall", "-Wextra", "-Wno-unused-parameter",
           "-Wno-unknown-pragmas", "-Werror", "-shared", "-fPIC", "-pthread", HARNESS, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    dll = C.CDLL(out)
    P, Z, I, U = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32
    dll.overlap_host_walk.restype = I
    dll.overlap_host_walk.argtypes = [I, P, U, P, P, P, Z, P, I, U, I, P, P, P, P]
    return dll


def prim_boxes(raw):
    """(n, 6) {min.xyz, max.xyz} by original id: Tri::get_bbox of (n, 9) triangles, {c - r, c + r} of (n, 4) spheres, in raw's dtype."""
    raw = np.asarray(raw)
    if raw.shape[1] == 4:
        c, r = raw[:, :3], raw[:, 3:4]
        return np.ascontiguousarray(np.concatenate([c - r, c + r], axis=1))
    t = raw.reshape(-1, 3, 3)
    return np.ascontiguousarray(np.concatenate([t.min(axis=1), t.max(axis=1)], axis=1))


class Tree:
    """What the harness walks: pair records, root word, the boxes by original id, BVH-order index -> original id."""

    def __init__(self, bounds6, index, bboxes, prim_ids):
        self.double = bounds6.dtype == np.float64
        self.bounds, self.index = np.asarray(bounds6), np.asarray(index)
        self.pairs = _aligned(pair_records(bounds6, index))
        self.root = int(index[0]) & 0xFFFFFFFF
        self.dtype = bounds6.dtype
        self.bboxes = _aligned(np.ascontiguousarray(bboxes, dtype=self.dtype))
        self.ids = np.ascontiguousarray(prim_ids, dtype=np.uint32)
        self.dfs = dfs_prim_order(index)

    @property
    def n(self):
        return len(self.ids)

    def ordered_boxes(self):
        """The boxes in BVH order."""
        return self.bboxes[self.ids.astype(np.int64)]

    def with_boxes(self, bboxes):
        t = Tree.__new__(Tree)
        t.__dict__.update(self.__dict__)
        t.bboxes = _aligned(np.ascontiguousarray(bboxes, dtype=self.dtype))
        return t


def golden_tree(scene, mode):
    g = load_golden(scene)
    nodes, ids = parse_stream(g[f"bvh_{mode}"].tobytes(), g["prims"].dtype == np.float64)
    return Tree(nodes["bounds"], nodes["index"], prim_boxes(g["prims"]), ids), g["prims"]


def query_boxes(raw, n, dtype, seed):
    """n boxes: centres from scene_queries, cubes of edge 0 .. 0.3 of the scene diagonal (every 16th of zero extent), every 64th moved
    far outside the scene, every 128th covering the whole scene."""
    pts, diag = scene_queries(raw, n, dtype, seed, raw.shape[1] == 4)
    pts = pts[::len(pts) // n][:n]
    rng = np.random.default_rng(seed)
    half = (0.15 * diag * rng.random((n, 1))).astype(dtype)
    half[::16] = 0
    q = np.concatenate([pts - half, pts + half], axis=1).astype(dtype)
    q[5::64] += np.asarray(10 * diag, dtype=dtype)
    b = prim_boxes(raw)
    q[7::128, :3] = b[:, :3].min(axis=0) - 1
    q[7::128, 3:] = b[:, 3:].max(axis=0) + 1
    return np.ascontiguousarray(q)


def brute(pb, q):
    """within[k, i]: query box k overlaps BVH-order box i. Closed intervals in the arrays' dtype; a NaN or min > max on either side
    makes the pair false."""
    pb, q = np.asarray(pb), np.asarray(q)
    with np.errstate(invalid="ignore"):
        ok = (pb[:, :3] <= pb[:, 3:]).all(axis=1)[None, :] & (q[:, :3] <= q[:, 3:]).all(axis=1)[:, None]
        for k in range(3):
            ok &= (pb[None, :, k] <= q[:, None, 3 + k]) & (q[:, None, k] <= pb[None, :, 3 + k])
    return ok


def expected_lists(within, dfs):
    """(counts, concatenated lists) of a brute-force matrix, each row listed in the walk's order."""
    w = within[:, dfs]
    rows, cols = np.nonzero(w)                                 # (row-major: ascending position in dfs within a row)
    return w.sum(axis=1).astype(np.uint32), dfs[cols].astype(np.uint32)


def host_walk(dll, tree, queries, offsets=None, total=0, counts=True, order=None, original_ids=False, deep_cap=0, threads=1):
    """One call of the kernel's walk. queries None: self mode. offsets None: the count pass. Otherwise the list buffer holds `total`
    entries between two guard zones of GUARD sentinels and is returned WITH the guards. -> (counts or None, list or None, counters)."""
    q = None if queries is None else _aligned(np.ascontiguousarray(queries, dtype=tree.dtype))
    n = tree.n if q is None else len(q)
    cnt = np.zeros(3, dtype=np.uint64)
    c = np.full(n, 0xABABABAB, dtype=np.uint32) if counts else None
    off = lp = lp_arg = None
    if offsets is not None:
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        lp = np.full(total + 2 * GUARD, SENT_PRIM, dtype=np.uint32)
        lp_arg = lp[GUARD:].ctypes.data_as(C.c_void_p)
    order = None if order is None else np.ascontiguousarray(order, dtype=np.uint32)
    assert dll.overlap_host_walk(int(tree.double), _p(tree.pairs), tree.root, _p(tree.bboxes), _p(tree.ids), _p(q), n, _p(order), int(original_ids),
                                 deep_cap, threads, _p(c), _p(off), lp_arg, _p(cnt)) == 0
    return c, lp, cnt


def host_overlap(dll, tree, queries, **kw):
    """Count, offsets, fill: (offsets (n + 1) uint64, ids, counts, counters of the fill pass). Checks what every such call must
    satisfy: the fill pass reports the counts of the count pass, exact offsets leave no padding, the guard zones stay untouched."""
    counts, _, cnt0 = host_walk(dll, tree, queries, **kw)
    offsets = np.concatenate([[0], np.cumsum(counts.astype(np.uint64))]).astype(np.uint64)
    total = int(offsets[-1])
    c2, lp, cnt = host_walk(dll, tree, queries, offsets=offsets, total=total, **kw)
    assert (c2 == counts).all() and (cnt == cnt0).all()
    assert guards_intact(lp, total)
    ids = lp[GUARD:GUARD + total]
    assert (ids != INVALID).all()
    return offsets, ids, counts, cnt


def self_expected(tree):
    """Brute-force self mode: row q lists the i > q (BVH order) whose box overlaps box q."""
    pb = tree.ordered_boxes()
    within = brute(pb, pb) & (np.arange(tree.n)[None, :] > np.arange(tree.n)[:, None])
    return within, expected_lists(within, tree.dfs)


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return compile_harness(tmp_path_factory.mktemp("overlap"))


def test_trees_are_fitted_to_the_boxes():
    """What makes the walk exact: every leaf box of the golden trees is the union of the boxes computed here."""
    for scene in GOLDEN_SCENES:
        for mode in TREES:
            tree, _ = golden_tree(scene, mode)
            pb = tree.ordered_boxes()
            for k in np.flatnonzero(tree.index & 15):
                first, count = int(tree.index[k]) >> 4, int(tree.index[k]) & 15
                b = tree.bounds[k]
                assert (b[0::2] == pb[first:first + count, :3].min(axis=0)).all() and (b[1::2] == pb[first:first + count, 3:].max(axis=0)).all()


@pytest.mark.parametrize("scene", GOLDEN_SCENES)
@pytest.mark.parametrize("mode", TREES)
def test_walk_equals_brute_force(dll, scene, mode):
    tree, raw = golden_tree(scene, mode)
    assert len(tree.dfs) == tree.n and len(set(tree.dfs.tolist())) == tree.n
    pb = tree.ordered_boxes()
    for name, q in (("random", query_boxes(raw, 1024, tree.dtype, 11)), ("own", prim_boxes(raw))):
        offsets, ids, counts, cnt = host_overlap(dll, tree, q, threads=4)
        assert cnt[0] > 0 and cnt[1] > 0 and cnt[2] > 0
        want_counts, want_ids = expected_lists(brute(pb, q), tree.dfs)
        print(f"{scene} {mode} {name}: {len(want_ids)} listed primitives (mean list {len(want_ids) / len(q):.2f})")
        assert (counts == want_counts).all() and ids.tobytes() == want_ids.tobytes()
        assert len(want_ids) >= len(q) // 2 and (counts == 0).any() == (name == "random")
        if name == "random":
            assert (counts[7::128] == tree.n).all() and (counts[5::64] == 0).all()
            # original ids map values only; reading the batch through a permuted order changes nothing
            oo, oi, oc, _ = host_overlap(dll, tree, q, original_ids=True)
            assert (oo == offsets).all() and (oi == tree.ids[ids.astype(np.int64)]).all() and (oc == counts).all()
            perm = np.random.default_rng(5).permutation(len(q)).astype(np.uint32)
            po, pi, pc, pcnt = host_overlap(dll, tree, q, order=perm)
            assert (po == offsets).all() and pi.tobytes() == ids.tobytes() and (pcnt == cnt).all()


@pytest.mark.parametrize("scene", GOLDEN_SCENES)
@pytest.mark.parametrize("mode", TREES)
def test_self_mode(dll, scene, mode):
    tree, _ = golden_tree(scene, mode)
    within, (want_counts, want_ids) = self_expected(tree)
    offsets, ids, counts, _ = host_overlap(dll, tree, None, threads=4)
    assert (counts == want_counts).all() and ids.tobytes() == want_ids.tobytes()
    assert int(offsets[-1]) == SELF_PAIRS[scene]
    rows = np.repeat(np.arange(tree.n), counts)
    assert (ids > rows).all()                                   # i > q: no primitive with itself, every pair once
    if scene in TOUCHING_PAIRS:                                 # pairs that overlap only because the intervals are closed
        pb = tree.ordered_boxes()
        open_ = np.ones_like(within)
        for k in range(3):
            open_ &= (pb[None, :, k] < pb[:, None, 3 + k]) & (pb[:, None, k] < pb[None, :, 3 + k])
        strictly = within & open_
        assert SELF_PAIRS[scene] - int(strictly.sum()) == TOUCHING_PAIRS[scene]
    oo, oi, oc, _ = host_overlap(dll, tree, None, original_ids=True)
    assert (oo == offsets).all() and (oi == tree.ids[ids.astype(np.int64)]).all()


def test_output_shapes(dll):
    tree, raw = golden_tree("soup2k", "parallel_high")
    q = query_boxes(raw, 300, np.float32, 5)
    n = len(q)
    offsets, ids, counts, _ = host_overlap(dll, tree, q)            # count pass == list lengths, no padding, guards: checked inside
    assert counts.max() > 4 and (counts == 0).any() and (counts > 0).any()
    _, lp, _ = host_walk(dll, tree, q, offsets=offsets, total=len(ids), counts=False)          # without the optional counts: same lists
    assert (lp[GUARD:GUARD + len(ids)] == ids).all() and guards_intact(lp, len(ids))
    # k = 4 slots per query, the buffer starting at a non-zero offset: prefix in walk order, padding, untruncated counts, guards
    k, base = 4, 7
    fixed = (base + k * np.arange(n + 1)).astype(np.uint64)
    total = base + k * n + 5                                   # entries before offsets[0] and after offsets[n] belong to nobody
    c4, lp, _ = host_walk(dll, tree, q, offsets=fixed, total=total)
    assert (c4 == counts).all()
    assert (lp[GUARD:GUARD + base] == SENT_PRIM).all() and (lp[GUARD + base + k * n:] == SENT_PRIM).all() and guards_intact(lp, total)
    seg = lp[GUARD + base:GUARD + base + k * n].reshape(n, k)
    for i in range(n):
        m = min(int(counts[i]), k)
        assert (seg[i, :m] == ids[int(offsets[i]):int(offsets[i]) + m]).all() and (seg[i, m:] == INVALID).all()
    # stale offsets: a segment that ends before it begins is empty, the others (here all [0, 9)) are kept to; counts are still reported
    stale = np.zeros(n + 1, dtype=np.uint64)
    stale[::2] = 9
    c5, lp, _ = host_walk(dll, tree, q, offsets=stale, total=16)
    assert (c5 == counts).all()
    assert not (lp[GUARD + 9:GUARD + 16] != SENT_PRIM).any() and guards_intact(lp, 16)
    # self mode, fixed slots
    so, si, sc, _ = host_overlap(dll, tree, None)
    fixed = (2 * np.arange(tree.n + 1)).astype(np.uint64)
    c6, lp, _ = host_walk(dll, tree, None, offsets=fixed, total=2 * tree.n)
    seg = lp[GUARD:GUARD + 2 * tree.n].reshape(tree.n, 2)
    assert (c6 == sc).all() and sc.max() > 2 and guards_intact(lp, 2 * tree.n)
    for i in range(tree.n):
        m = min(int(sc[i]), 2)
        assert (seg[i, :m] == si[int(so[i]):int(so[i]) + m]).all() and (seg[i, m:] == INVALID).all()


def test_edge_queries(dll):
    tree, raw = golden_tree("cornell", "binned")
    dt = tree.dtype
    pb = tree.ordered_boxes()
    j = int(np.flatnonzero((pb[:, :3] < pb[:, 3:]).sum(axis=1) >= 2)[3])          # a box with extent on two axes at least
    lo, hi = pb[j, :3], pb[j, 3:]
    mid = ((lo + hi) / 2).astype(dt)
    scene_lo, scene_hi = pb[:, :3].min(axis=0), pb[:, 3:].max(axis=0)
    face = mid.copy()
    face[0] = lo[0]
    far = (scene_hi + 5).astype(dt)
    z = int(np.flatnonzero(pb[:, :3] == 0)[0])                # some primitive box has a min face at +0 on axis z % 3 ...
    zi, zk = divmod(z, 3)
    neg = np.concatenate([scene_lo - 1, scene_hi + 1]).astype(dt)
    neg[3 + zk] = -0.0                                        # ... and this box ends at -0 there: they touch
    below = neg.copy()
    below[3 + zk] = -np.finfo(dt).tiny                        # ... and this one ends just before it
    inf = np.array([-np.inf] * 3 + [np.inf] * 3, dtype=dt)
    half_inf = np.concatenate([scene_lo - 1, [np.inf] * 3]).astype(dt)
    q = np.array([np.concatenate([lo, hi]),                   # 0: a primitive's own box
                  np.concatenate([[np.nan], lo[1:], hi]),     # 1: a NaN component
                  np.concatenate([lo, [np.nan], hi[1:]]),     # 2
                  np.concatenate([[hi[0] + 1], lo[1:], hi]),  # 3: min > max on one axis (and the interval still straddles the box)
                  np.concatenate([mid, mid]),                 # 4: a point inside the box
                  np.concatenate([face, face]),               # 5: a point on its face
                  np.concatenate([far, far]),                 # 6: a point outside everything
                  neg, below, inf, half_inf], dtype=dt)
    within = brute(pb, q)
    want_counts, want_ids = expected_lists(within, tree.dfs)
    offsets, ids, counts, _ = host_overlap(dll, tree, q)
    assert (counts == want_counts).all() and ids.tobytes() == want_ids.tobytes()
    seg = lambda k: ids[int(offsets[k]):int(offsets[k + 1])]
    assert j in seg(0) and counts[1] == 0 and counts[2] == 0 and counts[3] == 0 and counts[6] == 0
    assert j in seg(4) and j in seg(5)
    assert zi in seg(7) and zi not in seg(8)
    assert (seg(9) == tree.dfs).all() and (seg(10) == tree.dfs).all()
    # invalid queries with a segment: padded with INVALID
    fixed = (2 * np.arange(len(q) + 1)).astype(np.uint64)
    _, lp, _ = host_walk(dll, tree, q, offsets=fixed, total=2 * len(q))
    assert (lp[GUARD:-GUARD].reshape(-1, 2)[[1, 2, 3, 6]] == INVALID).all()
    # a primitive box with a NaN, and one with min > max, are never listed; everything else is as before. (The tree is not refitted:
    # the result is the walk's set, which still reaches every other primitive.)
    bb = tree.bboxes.copy()
    bb[tree.ids[j], 4] = np.nan
    other = (j + 5) % tree.n
    bb[tree.ids[other], 0], bb[tree.ids[other], 3] = bb[tree.ids[other], 3] + 1, bb[tree.ids[other], 0] - 1
    bad = tree.with_boxes(bb)
    o2, i2, c2, _ = host_overlap(dll, bad, q)
    w2 = brute(bad.ordered_boxes(), q)
    assert not w2[:, j].any() and not w2[:, other].any() and (w2 == within)[:, [k for k in range(tree.n) if k not in (j, other)]].all()
    wc, wi = expected_lists(w2, tree.dfs)
    assert (c2 == wc).all() and i2.tobytes() == wi.tobytes() and c2[9] == tree.n - 2
    so, si, sc, _ = host_overlap(dll, bad, None)
    assert sc[j] == 0 and sc[other] == 0 and j not in si and other not in si


def python_walk(tree, bboxes_ordered, q):
    """The contract's walk in Python: a node is entered iff its box overlaps the query, left child first."""
    def hit(lo, hi):
        with np.errstate(invalid="ignore"):
            return bool((lo <= hi).all() and (q[:3] <= q[3:]).all() and (lo <= q[3:]).all() and (q[:3] <= hi).all())
    out, stack = [], [0]
    while stack:
        k = stack.pop()
        w = int(tree.index[k])
        first, count = w >> 4, w & 15
        if count:
            out += [i for i in range(first, first + count) if hit(bboxes_ordered[i, :3], bboxes_ordered[i, 3:])]
        else:
            for c in (first + 1, first):
                if hit(tree.bounds[c][0::2], tree.bounds[c][1::2]):
                    stack.append(c)
    return np.array(out, dtype=np.uint32)


def test_loose_tree_gives_the_walks_set(dll):
    """An inner box shrunk by hand so that it no longer contains a primitive below it: the result is the walk's set."""
    fitted, raw = golden_tree("soup2k", "parallel_high")
    bounds = fitted.bounds.copy()
    inner = int(np.flatnonzero((fitted.index & 15) == 0)[40])
    assert inner != 0
    k = inner                                                  # the primitives below it: follow first children to a leaf
    below = []
    todo = [inner]
    while todo:
        w = int(fitted.index[todo.pop()])
        if w & 15:
            below += list(range(w >> 4, (w >> 4) + (w & 15)))
        else:
            todo += [w >> 4, (w >> 4) + 1]
    pb = fitted.ordered_boxes()
    p = below[int(np.argmax(pb[below, 3]))]                    # the one that reaches farthest in +x
    others = [i for i in below if i != p]
    cut = np.float32((float(pb[others, 3].max()) + float(pb[p, 3])) / 2)
    assert pb[others, 3].max() < cut < pb[p, 3]
    bounds[inner][1] = cut
    loose = Tree(bounds, fitted.index, fitted.bboxes, fitted.ids)
    mid = (pb[p, :3] + pb[p, 3:]) / 2
    point = np.array([pb[p, 3], mid[1], mid[2]], dtype=np.float32)            # on the +x face of p: beyond the shrunk box
    q = np.concatenate([[np.concatenate([point, point])], query_boxes(raw, 64, np.float32, 3)]).astype(np.float32)
    offsets, ids, counts, _ = host_overlap(dll, loose, q)
    fo, fi, fc, _ = host_overlap(dll, fitted, q)
    assert p in fi[int(fo[0]):int(fo[1])] and p not in ids[int(offsets[0]):int(offsets[1])]
    for n in range(len(q)):
        assert (ids[int(offsets[n]):int(offsets[n + 1])] == python_walk(loose, pb, q[n])).all()
        assert (fi[int(fo[n]):int(fo[n + 1])] == python_walk(fitted, pb, q[n])).all()


def chain(depth, prep_tris, stacked):
    """chain_tree as a Tree over the triangles' boxes; stacked: every inner child on the left, so that the left-first walk of a box
    that overlaps every level stacks one leaf per level."""
    tris, nodes, ids = chain_tree(depth, prep_tris)
    if stacked:
        nodes[1::2], nodes[2::2] = nodes[2::2].copy(), nodes[1::2].copy()
    return Tree(nodes["bounds"], nodes["index"], prim_boxes(tris), ids), nodes, tris


def chain_boxes(depth, n):
    """Boxes over the chain (triangles at x = 4000 - k, |y|, |z| <= 1): every 4th covers every level, the others the far end only."""
    rng = np.random.default_rng(depth)
    q = np.zeros((n, 6), dtype=np.float32)
    q[:, 0] = 4000 - depth - 1 - rng.random(n)
    q[:, 3] = 4000 - depth + 10 * rng.random(n)
    q[::4, 3] = 4001
    q[:, 1:3] = -1.5 * rng.random((n, 2))
    q[:, 4:6] = 1.5 * rng.random((n, 2))
    return q


@pytest.mark.parametrize("depth", [70, 300])
@pytest.mark.parametrize("stacked", [False, True])
def test_deep_chain(dll, orc, depth, stacked):
    """Stacked, 70 levels cross LDS -> scratch (entry 16), scratch -> HBM (entry 64) and end on the last of the 6 HBM entries given;
    300 levels fill 236."""
    tree, _, _ = chain(depth, orc.prep_tris, stacked)
    assert (tree.dfs == (np.arange(depth, -1, -1) if stacked else np.arange(depth + 1))).all()
    q = chain_boxes(depth, 48)
    offsets, ids, counts, _ = host_overlap(dll, tree, q, deep_cap=depth - 64 if stacked else depth - 64 + 1)
    want_counts, want_ids = expected_lists(brute(tree.ordered_boxes(), q), tree.dfs)
    assert (counts == want_counts).all() and ids.tobytes() == want_ids.tobytes()
    assert (counts[::4] == depth + 1).all() and 0 < counts[1::4].min() and counts[1::4].max() < 16
    # self mode on the chain: neighbouring triangles' boxes are 1 apart and flat in x, so nothing overlaps ... until they are fattened
    # (and the tree's boxes with them: every union grows by the same half)
    fat, bounds = tree.bboxes.copy(), tree.bounds.copy()
    fat[:, 0] -= 0.5
    fat[:, 3] += 0.5                                           # now box k touches box k + 1, and only that one
    bounds[:, 0] -= 0.5
    bounds[:, 1] += 0.5
    t2 = Tree(bounds, tree.index, fat, tree.ids)
    so, si, sc, _ = host_overlap(dll, t2, None, deep_cap=depth - 64 + 1)
    w, (wc, wi) = self_expected(t2)
    assert (sc == wc).all() and si.tobytes() == wi.tobytes() and int(so[-1]) == depth


def test_overlap_symbols_are_declared_and_exported():
    from bvh_amd import _lib, build
    build.build()
    dll = _lib.load()
    header = open(os.path.join(ROOT, "include", "bvh_amd.h")).read()
    declared = set(re.findall(r"BVH_AMD_API[^;]*?\b(bvh\w+)\s*\(", header))
    want = {f"bvh{s}_overlap_{kind}" for s in ("3f", "3d") for kind in ("boxes", "self")}
    assert {n for n in declared if "overlap" in n} == want
    assert want <= set(_lib.exported_symbols())
    for name in sorted(want):
        assert hasattr(dll, name), name
    for s in ("2f", "2d"):
        for kind in ("boxes", "self"):
            assert not hasattr(dll, f"bvh{s}_overlap_{kind}")
            assert f"bvh{s}_overlap_{kind}" not in _lib.exported_symbols()
