"""What the triangle-intersection tests share (test_tri_intersect_host.py, test_gpu_tri_intersect.py): the host harness
(tests/cpp/tri_intersect_body_host.cpp: the kernel's text compiled for the CPU), the trees it walks, the lattice scene on which the
kernel's arithmetic is exact, and the exact reference for that scene: an integer separating-axis test."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT, load_golden, parse_stream
from test_kernel_body_host import _aligned, pair_records
from test_radius_search_host import GUARD, INVALID, SENT_PRIM, dfs_prim_order, guards_intact

HARNESS = os.path.join(ROOT, "tests", "cpp", "tri_intersect_body_host.cpp")
TREES = ["binned", "parallel_high"]
TRI_SCENES = ["cornell", "soup2k", "terrain2k", "soup2k_f64"]
SKIP_SHARED = 32                                              # BVH_AMD_TRI_SKIP_SHARED
LATTICE_N, LATTICE_SEED = 400, 2024


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def compile_harness(out_dir):
    """g++ with the flags of test_overlap_host.compile_harness."""
    out = os.path.join(str(out_dir), "libtri_intersect_body_host.so")
    cmd = ["g++", "-std=c++20", "-O1", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-strict-aliasing", "-Wall", "-Wextra", "-Wno-unused-parameter",
           "-Wno-unknown-pragmas", "-Werror", "-shared", "-fPIC", "-pthread", HARNESS, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    dll = C.CDLL(out)
    P, Z, I, U = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32
    dll.tri_tri_intersects.restype = I
    dll.tri_tri_intersects.argtypes = [I, P, P, I]
    dll.tri_tri_matrix.restype = None
    dll.tri_tri_matrix.argtypes = [I, P, Z, P, Z, I, P]
    dll.tri_intersect_host_walk.restype = I
    dll.tri_intersect_host_walk.argtypes = [I, P, U, P, P, P, Z, P, I, I, U, I, P, P, P, P]
    dll.tri_intersect_host_walk_slice.restype = C.c_longlong
    dll.tri_intersect_host_walk_slice.argtypes = [I, P, U, P, P, P, Z, Z, Z, P, I, I, U, P, P, P, P]
    return dll


# ---- the exact reference: separating axes in integers -------------------------------------------------------------------------------

def _cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def _sub(u, v):
    return (u[0] - v[0], u[1] - v[1], u[2] - v[2])


def sat_intersects(a, b):
    """Two triangles of three integer points each (Python ints: no rounding, no overflow) intersect as closed sets iff none of 17
    axes separates them: the two normals, the nine edge x edge products, and each normal x each edge of its own triangle (the six
    that decide the coplanar case). A zero axis is skipped; an axis separates iff the projections' max < min strictly. A triangle
    with a zero normal intersects nothing."""
    a = [tuple(int(x) for x in p) for p in a]
    b = [tuple(int(x) for x in p) for p in b]
    ea = [_sub(a[1], a[0]), _sub(a[2], a[1]), _sub(a[0], a[2])]
    eb = [_sub(b[1], b[0]), _sub(b[2], b[1]), _sub(b[0], b[2])]
    na, nb = _cross(ea[0], ea[1]), _cross(eb[0], eb[1])
    if na == (0, 0, 0) or nb == (0, 0, 0):
        return False
    axes = [na, nb] + [_cross(u, v) for u in ea for v in eb] + [_cross(na, u) for u in ea] + [_cross(nb, v) for v in eb]
    assert len(axes) == 17
    for ax in axes:
        if ax == (0, 0, 0):
            continue
        pa = [ax[0] * p[0] + ax[1] * p[1] + ax[2] * p[2] for p in a]
        pb = [ax[0] * p[0] + ax[1] * p[1] + ax[2] * p[2] for p in b]
        if max(pa) < min(pb) or max(pb) < min(pa):
            return False
    return True


def sat_matrix(ta, tb):
    """sat_intersects for every pair of two (n, 3, 3) integer arrays, in int64 (on the lattice |coordinate| <= 8: an axis component
    stays below 2^15, a projection below 2^20). The tests check it against sat_intersects itself on a sample."""
    ta, tb = np.asarray(ta, dtype=np.int64), np.asarray(tb, dtype=np.int64)
    ea = np.stack([ta[:, 1] - ta[:, 0], ta[:, 2] - ta[:, 1], ta[:, 0] - ta[:, 2]], axis=1)         # (n, 3 edges, 3)
    eb = np.stack([tb[:, 1] - tb[:, 0], tb[:, 2] - tb[:, 1], tb[:, 0] - tb[:, 2]], axis=1)
    na, nb = np.cross(ea[:, 0], ea[:, 1]), np.cross(eb[:, 0], eb[:, 1])
    A, B = len(ta), len(tb)
    out = np.ones((A, B), dtype=bool)

    def apply(axes):                                           # axes (A, B, 3)
        pa = np.einsum("abk,avk->abv", axes, ta)               # (A, B, 3 vertices)
        pb = np.einsum("abk,bvk->abv", axes, tb)
        sep = (pa.max(axis=2) < pb.min(axis=2)) | (pb.max(axis=2) < pa.min(axis=2))
        return sep & (axes != 0).any(axis=2)

    sep = apply(np.broadcast_to(na[:, None, :], (A, B, 3))) | apply(np.broadcast_to(nb[None, :, :], (A, B, 3)))
    for i in range(3):
        for j in range(3):
            sep |= apply(np.cross(ea[:, None, i, :], eb[None, :, j, :]))
        sep |= apply(np.broadcast_to(np.cross(na, ea[:, i])[:, None, :], (A, B, 3)))
        sep |= apply(np.broadcast_to(np.cross(nb, eb[:, i])[None, :, :], (A, B, 3)))
    out &= ~sep
    out &= (na != 0).any(axis=1)[:, None] & (nb != 0).any(axis=1)[None, :]
    return out


# ---- the lattice scene ---------------------------------------------------------------------------------------------------------------

def lattice_tris(n=LATTICE_N, seed=LATTICE_SEED):
    """(n, 3, 3) int64 triangles with coordinates in [-8, 8]: each has its vertices within 1 .. 5 of a random centre (so that most
    pairs are apart and the intersecting ones are of every kind), every fourth is flattened onto one of the planes z = -2, 0, 3
    (coplanar pairs), and nothing keeps vertices apart or triangles from having no area."""
    rng = np.random.default_rng(seed)
    centre = rng.integers(-6, 7, size=(n, 1, 3))
    reach = rng.integers(1, 6, size=(n, 1, 1))
    t = np.clip(centre + rng.integers(-5, 6, size=(n, 3, 3)) * reach // 5, -8, 8).astype(np.int64)
    flat = np.arange(n) % 4 == 0
    t[flat, :, 2] = rng.choice([-2, 0, 3], size=int(flat.sum()))[:, None]
    return t


def shares_vertex_matrix(ta, tb):
    """[i, j]: some vertex of ta[i] equals some vertex of tb[j] on all three coordinates (== of the arrays' dtype)."""
    ta, tb = np.asarray(ta).reshape(len(ta), 3, 3), np.asarray(tb).reshape(len(tb), 3, 3)
    with np.errstate(invalid="ignore"):
        return (ta[:, None, :, None, :] == tb[None, :, None, :, :]).all(axis=4).any(axis=(2, 3))


# ---- trees and walks -----------------------------------------------------------------------------------------------------------------

def tri_boxes(tris9):
    t = np.asarray(tris9).reshape(-1, 3, 3)
    return np.ascontiguousarray(np.concatenate([t.min(axis=1), t.max(axis=1)], axis=1))


class TriTree:
    """What the harness walks: pair records, root word, the triangles by original id, BVH-order index -> original id."""

    def __init__(self, bounds6, index, tris9, prim_ids):
        self.double = bounds6.dtype == np.float64
        self.bounds, self.index = np.asarray(bounds6), np.asarray(index)
        self.pairs = _aligned(pair_records(bounds6, index))
        self.root = int(index[0]) & 0xFFFFFFFF
        self.dtype = bounds6.dtype
        self.tris = _aligned(np.ascontiguousarray(np.asarray(tris9).reshape(-1, 9), dtype=self.dtype))
        self.ids = np.ascontiguousarray(prim_ids, dtype=np.uint32)
        self.dfs = dfs_prim_order(index)

    @property
    def n(self):
        return len(self.ids)

    def ordered_tris(self):
        """The triangles in BVH order."""
        return np.ascontiguousarray(self.tris[self.ids.astype(np.int64)])

    def with_tris(self, tris9):
        t = TriTree.__new__(TriTree)
        t.__dict__.update(self.__dict__)
        t.tris = _aligned(np.ascontiguousarray(np.asarray(tris9).reshape(-1, 9), dtype=self.dtype))
        return t


def golden_tree(scene, mode):
    g = load_golden(scene)
    nodes, ids = parse_stream(g[f"bvh_{mode}"].tobytes(), g["prims"].dtype == np.float64)
    return TriTree(nodes["bounds"], nodes["index"], g["prims"], ids)


def built_tree(orc, tris9, dtype):
    """The tree the checker builds over the boxes of the triangles."""
    tris9 = np.ascontiguousarray(np.asarray(tris9).reshape(-1, 9), dtype=dtype)
    bb, cc = orc.prep_tris(tris9)
    cpu = orc.build(bb, cc)
    nodes, ids = parse_stream(cpu.serialize(), dtype == np.float64)
    return TriTree(nodes["bounds"], nodes["index"], tris9, ids)


def chain_tris(depth, dtype=np.float32):
    """depth + 1 triangles at x = base - k (query_slices.chain_base), standing across the x axis like test_closest_point_host.chain_tree's
    but turned about the vertical by turns one way and the other: each crosses its two neighbours and is parallel to the ones after."""
    import query_slices as qs
    n = depth + 1
    x = (qs.chain_base(depth) - np.arange(n)).astype(dtype)
    turn = np.where(np.arange(n) % 2 == 0, 0.75, -0.75).astype(dtype)
    tris = np.zeros((n, 9), dtype=dtype)
    tris[:, 0], tris[:, 1], tris[:, 2] = x - turn, -1, -1
    tris[:, 3], tris[:, 4], tris[:, 5] = x + turn, 1, -1
    tris[:, 6], tris[:, 7], tris[:, 8] = x, 0, 1
    return tris


def chain_tree(depth, dtype=np.float32, stacked=False, ids=None):
    """chain_tris under query_slices.chain_nodes (a tree `depth` levels deep, fitted to them); stacked: every inner child on the left,
    so that the left-first walk of a query that reaches every level stacks one leaf per level. ids: BVH-order index -> original id."""
    import query_slices as qs
    tris = chain_tris(depth, dtype)
    nodes = qs.chain_nodes(tri_boxes(tris), stacked)
    ids = np.arange(depth + 1, dtype=np.uint32) if ids is None else np.asarray(ids, dtype=np.uint32)
    by_id = np.zeros_like(tris)
    by_id[ids.astype(np.int64)] = tris
    return TriTree(nodes["bounds"], nodes["index"], by_id, ids)


def chain_queries(depth, n, dtype=np.float32):
    """Query triangles over the chain: every 4th a sliver along the x axis that crosses every level, the others a small triangle at
    the far end that crosses a few."""
    import query_slices as qs
    rng = np.random.default_rng(depth)
    base, far = qs.chain_base(depth), qs.chain_base(depth) - depth
    q = np.zeros((n, 9), dtype=dtype)
    cx = far + 6 * rng.random(n)
    q[:, 0], q[:, 1], q[:, 2] = cx - 1, -0.5, -0.5
    q[:, 3], q[:, 4], q[:, 5] = cx + 1, 0.5, -0.5
    q[:, 6], q[:, 7], q[:, 8] = cx, 0, 0.5
    q[::4] = np.array([far - 2, 0, -0.5, base + 2, 0, -0.5, base + 2, 0.05, 0], dtype=dtype)
    return q


def pair_matrix(dll, qa, tb, skip_shared=False):
    """[k, i]: tri_tri_intersects(query qa[k], primitive tb[i]), by the harness (the kernel's own pair test)."""
    qa, tb = np.ascontiguousarray(qa).reshape(-1, 9), np.ascontiguousarray(tb).reshape(-1, 9)
    assert qa.dtype == tb.dtype and qa.dtype in (np.float32, np.float64)
    m = np.empty((len(qa), len(tb)), dtype=np.uint8)
    dll.tri_tri_matrix(int(qa.dtype == np.float64), _p(qa), len(qa), _p(tb), len(tb), int(skip_shared), _p(m))
    return m.astype(bool)


def pair_test(dll, a, b, dtype=np.float32, skip_shared=False):
    a, b = np.ascontiguousarray(a, dtype=dtype).reshape(9), np.ascontiguousarray(b, dtype=dtype).reshape(9)
    return bool(dll.tri_tri_intersects(int(dtype == np.float64), _p(a), _p(b), int(skip_shared)))


def expected_lists(within, dfs):
    """(counts, concatenated lists) of a brute-force matrix, each row listed in the walk's order."""
    w = within[:, dfs]
    _, cols = np.nonzero(w)                                    # (row-major: ascending position in dfs within a row)
    return w.sum(axis=1).astype(np.uint32), dfs[cols].astype(np.uint32)


def self_mask(n):
    return np.arange(n)[None, :] > np.arange(n)[:, None]


def host_walk(dll, tree, queries, offsets=None, total=0, counts=True, order=None, original_ids=False, skip_shared=False, deep_cap=0, threads=1):
    """One call of the kernel's walk. queries None: self mode. offsets None: the count pass. Otherwise the list buffer holds `total`
    entries between two guard zones of GUARD sentinels and is returned WITH the guards. -> (counts or None, list or None, counters)."""
    q = None if queries is None else _aligned(np.ascontiguousarray(np.asarray(queries).reshape(-1, 9), dtype=tree.dtype))
    n = tree.n if q is None else len(q)
    cnt = np.zeros(3, dtype=np.uint64)
    c = np.full(n, 0xABABABAB, dtype=np.uint32) if counts else None
    off = lp = lp_arg = None
    if offsets is not None:
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        lp = np.full(total + 2 * GUARD, SENT_PRIM, dtype=np.uint32)
        lp_arg = lp[GUARD:].ctypes.data_as(C.c_void_p)
    order = None if order is None else np.ascontiguousarray(order, dtype=np.uint32)
    assert dll.tri_intersect_host_walk(int(tree.double), _p(tree.pairs), tree.root, _p(tree.tris), _p(tree.ids), _p(q), n, _p(order), int(original_ids),
                                       int(skip_shared), deep_cap, threads, _p(c), _p(off), lp_arg, _p(cnt)) == 0
    return c, lp, cnt


def host_intersect(dll, tree, queries, **kw):
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


def query_tris(tris9, n, seed, shift=0.02):
    """n query triangles for a scene: its own triangles (every (len / n)-th), moved by up to `shift` of the scene's diagonal, every 64th moved
    far outside, every 16th left where it is (it intersects itself at least)."""
    t = np.asarray(tris9).reshape(-1, 3, 3)
    rng = np.random.default_rng(seed)
    pick = np.arange(n) * len(t) // n
    diag = float(np.linalg.norm(t.max(axis=(0, 1)).astype(np.float64) - t.min(axis=(0, 1)).astype(np.float64)))
    move = (shift * diag * (2 * rng.random((n, 1, 3)) - 1)).astype(t.dtype)
    move[::16] = 0
    move[5::64] = np.asarray(10 * diag, dtype=t.dtype)
    return np.ascontiguousarray((t[pick] + move).reshape(n, 9))
