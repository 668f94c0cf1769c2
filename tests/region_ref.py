"""What the convex-region tests share (test_region_host.py, test_gpu_region.py): the host harness (tests/cpp/region_body_host.cpp: the
kernel's text compiled for the CPU), the trees it walks, region generators, the numpy brute force of the stated plane expression in the
tree's scalar type, the float64 restatement of the EXACT predicate, and exact clipping in rational arithmetic."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np

from conftest import ROOT, load_golden, parse_stream
from test_kernel_body_host import _aligned, pair_records
from test_radius_search_host import GUARD, INVALID, SENT_PRIM, _p, dfs_prim_order, guards_intact
from tri_intersect_ref import expected_lists  # noqa: F401  (re-exported)

HARNESS = os.path.join(ROOT, "tests", "cpp", "region_body_host.cpp")
TREES = ["serial_low", "parallel_high"]
REGION_EXACT = 64                                             # BVH_AMD_REGION_EXACT
SENT_INSIDE = 0xA5
MAX_PLANES = 8


def compile_harness(out_dir):
    """g++ with the flags of test_overlap_host.compile_harness."""
    out = os.path.join(str(out_dir), "libregion_body_host.so")
    cmd = ["g++", "-std=c++20", "-O1", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-strict-aliasing", "-Wall", "-Wextra", "-Wno-unused-parameter",
           "-Wno-unknown-pragmas", "-Werror", "-shared", "-fPIC", "-pthread", HARNESS, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    dll = C.CDLL(out)
    P, Z, I, U = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32
    dll.region_host_walk.restype = I
    dll.region_host_walk.argtypes = [I, P, U, P, P, I, I, P, U, Z, I, U, I, P, P, P, P, P]
    dll.region_host_walk_slice.restype = C.c_longlong
    dll.region_host_walk_slice.argtypes = [I, P, U, P, P, I, I, P, U, Z, Z, Z, I, U, P, P, P, P, P]
    dll.region_host_pairs.restype = I
    dll.region_host_pairs.argtypes = [I, I, P, P, U, Z, P]
    return dll


class PrimTree:
    """What the harness walks: pair records, root word, the primitives by original id ((n, 9) triangles or (n, 4) spheres), BVH-order
    index -> original id."""

    def __init__(self, bounds6, index, prims, prim_ids):
        self.double = bounds6.dtype == np.float64
        self.bounds, self.index = np.asarray(bounds6), np.asarray(index)
        self.pairs = _aligned(pair_records(bounds6, index))
        self.root = int(index[0]) & 0xFFFFFFFF
        self.dtype = bounds6.dtype
        self.prims = _aligned(np.ascontiguousarray(prims, dtype=self.dtype))
        self.leaf = 1 if self.prims.shape[1] == 4 else 0
        self.ids = np.ascontiguousarray(prim_ids, dtype=np.uint32)
        self.dfs = dfs_prim_order(index)

    @property
    def n(self):
        return len(self.ids)

    def ordered(self):
        """The primitives in BVH order."""
        return np.ascontiguousarray(self.prims[self.ids.astype(np.int64)])

    def with_prims(self, prims):
        t = PrimTree.__new__(PrimTree)
        t.__dict__.update(self.__dict__)
        t.prims = _aligned(np.ascontiguousarray(prims, dtype=self.dtype))
        return t


def golden_tree(scene, mode):
    g = load_golden(scene)
    nodes, ids = parse_stream(g[f"bvh_{mode}"].tobytes(), g["prims"].dtype == np.float64)
    return PrimTree(nodes["bounds"], nodes["index"], g["prims"], ids)


def chain_tree(depth, stacked, dtype=np.float32):
    from tri_intersect_ref import chain_tree as tri_chain
    t = tri_chain(depth, dtype, stacked)
    return PrimTree(t.bounds, t.index, t.tris, t.ids)


# ---- regions ---------------------------------------------------------------------------------------------------------------------------

PAD = ([0, 0, 0, 0], [0, 0, 0, -1], [-0.0, 0, -0.0, -0.0])      # planes that hold everywhere


def pad_planes(planes, m, k=0):
    """A list of planes padded to m with planes that hold everywhere."""
    planes = [list(map(float, p)) for p in planes]
    assert len(planes) <= m
    return planes + [list(PAD[(k + i) % len(PAD)]) for i in range(m - len(planes))]


def rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.diag(r))


def box_planes(centre, axes, half):
    """The six planes of the oriented box |axes[:, k] . (x - centre)| <= half[k], outward unit normals."""
    out = []
    for k in range(3):
        for s in (1.0, -1.0):
            n = s * axes[:, k]
            out.append([n[0], n[1], n[2], -(n @ centre) - half[k]])
    return out


def prim_points(raw):
    raw = np.asarray(raw, dtype=np.float64)
    return raw[:, :3] if raw.shape[1] == 4 else raw.reshape(-1, 3)


def make_regions(raw, n, m, dtype, seed):
    """(n, m, 4) regions for a scene, in turn: an oriented box, a view frustum, a half-space, a slab, an empty region (zero normal, d >
    0), an everything region; kinds of more than m planes are left out; all padded to m."""
    from bvh_amd.api import frustum_planes
    pts = prim_points(raw)
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    diag = float(np.linalg.norm(hi - lo))
    rng = np.random.default_rng(seed)
    kinds = [k for k, need in (("box", 6), ("frustum", 6), ("half", 1), ("slab", 2), ("empty", 1), ("all", 1)) if need <= m]
    out = np.zeros((n, m, 4), dtype=np.float64)
    for q in range(n):
        kind = kinds[q % len(kinds)]
        c = pts[rng.integers(len(pts))] + 0.05 * diag * rng.normal(size=3)
        if kind == "box":
            planes = box_planes(c, rotation(rng), diag * (0.02 + 0.25 * rng.random(3)))
        elif kind == "frustum":
            eye = c + diag * (0.2 + rng.random()) * rotation(rng)[:, 0]
            planes = frustum_planes(eye, c - eye, rotation(rng)[:, 1], np.radians(10 + 50 * rng.random()), 0.5 + 1.5 * rng.random(),
                                    0.01 * diag, diag * (0.3 + 2 * rng.random()), dtype=np.float64).tolist()
        elif kind == "half":
            nrm = rotation(rng)[:, 0] * (0.1 + 3 * rng.random())
            planes = [[nrm[0], nrm[1], nrm[2], -(nrm @ c)]]
        elif kind == "slab":
            nrm = rotation(rng)[:, 0]
            t = 0.02 * diag * rng.random()
            planes = [[nrm[0], nrm[1], nrm[2], -(nrm @ c) - t], [-nrm[0], -nrm[1], -nrm[2], (nrm @ c) - t]]
        elif kind == "empty":
            planes = [[0, 0, 0, 1.0]]
        else:
            planes = [[0, 0, 0, 0.0]]
        out[q] = pad_planes(planes, m, q)
    return np.ascontiguousarray(out.astype(dtype))


# ---- brute force in the tree's scalar type -----------------------------------------------------------------------------------------------

def plane_values(planes, pts):
    """[q, p, i]: the value of plane p of region q at point i, ((nx*x0 + ny*x1) + nz*x2) + d in the arrays' dtype, one rounding per
    operation."""
    pl, x = np.asarray(planes), np.asarray(pts)
    assert pl.dtype == x.dtype
    with np.errstate(invalid="ignore", over="ignore"):
        return ((pl[:, :, None, 0] * x[None, None, :, 0] + pl[:, :, None, 1] * x[None, None, :, 1]) + pl[:, :, None, 2] * x[None, None, :, 2]) + pl[:, :, None, 3]


def valid_regions(planes):
    return np.isfinite(np.asarray(planes)).all(axis=(1, 2))


def brute_cull(prims, planes):
    """(match[q, i], inside[q, i]) of the CULL test (triangles) or the sphere test for BVH-order primitives `prims`."""
    prims, planes = np.asarray(prims), np.asarray(planes)
    n, N = len(planes), len(prims)
    valid = valid_regions(planes)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        if prims.shape[1] == 9:
            ins = np.stack([plane_values(planes, prims[:, 3 * v:3 * v + 3]) <= 0 for v in range(3)], axis=3)      # [q, p, i, v]
            match = ins.any(axis=3).all(axis=1)
            inside = ins.all(axis=3).all(axis=1)
        else:
            s = plane_values(planes, prims[:, :3])
            ln = np.sqrt((planes[:, :, 0] * planes[:, :, 0] + planes[:, :, 1] * planes[:, :, 1]) + planes[:, :, 2] * planes[:, :, 2])
            rl = prims[None, None, :, 3] * ln[:, :, None]
            match = (s <= rl).all(axis=1)
            inside = (s <= -rl).all(axis=1)
    assert match.shape == (n, N)
    return match & valid, inside & match & valid


def exact64(D, delta=0.0):
    """The EXACT predicate restated in float64 on plane values D[k, p, i] (pair k, plane p, vertex i), every value moved by delta:
    some pair of the m + 3 constraints crosses at a point where all the others hold."""
    D = np.asarray(D, dtype=np.float64) + delta
    K, m = D.shape[0], D.shape[1]
    tri = np.broadcast_to(np.array([[-1.0, 0, 0], [0, -1, 0], [1, 1, -1]]), (K, 3, 3))
    L = np.concatenate([tri, np.stack([D[:, :, 1] - D[:, :, 0], D[:, :, 2] - D[:, :, 0], D[:, :, 0]], axis=2)], axis=1)
    found = np.zeros(K, dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(m + 3):
            for j in range(i + 1, m + 3):
                c = np.cross(L[:, i], L[:, j])
                w = c[:, 2]
                ok = (w > 0) | (w < 0)
                for k in range(m + 3):
                    if k != i and k != j:
                        t = (L[:, k] * c).sum(axis=1)
                        ok &= np.where(w > 0, t <= 0, t >= 0)
                found |= ok
    return found


def clip_exact(tri, planes):
    """Sutherland-Hodgman in rational arithmetic: does the closed triangle (3 x 3 integers) share a point with the closed region?"""
    poly = [tuple(Fraction(int(c)) for c in v) for v in tri]
    for pl in planes:
        a, b, c, d = (Fraction(int(x)) for x in pl)
        val = lambda p: a * p[0] + b * p[1] + c * p[2] + d
        out = []
        for k in range(len(poly)):
            p, q = poly[k], poly[(k + 1) % len(poly)]
            vp, vq = val(p), val(q)
            if vp <= 0:
                out.append(p)
            if (vp < 0 < vq) or (vq < 0 < vp):
                t = vp / (vp - vq)
                out.append(tuple(p[i] + t * (q[i] - p[i]) for i in range(3)))
        poly = out
        if not poly:
            return False
    return True


# ---- the harness ----------------------------------------------------------------------------------------------------------------------------

def host_pairs(dll, prims, planes, dtype):
    """The kernel's primitive tests on bare pairs (primitive k, region k): (cull, exact, inside) bool arrays."""
    pr = np.ascontiguousarray(prims, dtype=dtype)
    pl = np.ascontiguousarray(planes, dtype=dtype)
    out = np.zeros(len(pr), dtype=np.uint8)
    assert dll.region_host_pairs(int(dtype == np.float64), int(pr.shape[1] == 4), _p(pr), _p(pl), pl.shape[1], len(pr), _p(out)) == 0
    return (out & 1) != 0, (out & 2) != 0, (out & 4) != 0


def host_walk(dll, tree, planes, exact=False, offsets=None, total=0, counts=True, original_ids=False, inside=False, deep_cap=0, threads=1):
    """One call of the kernel's walk. offsets None: the count pass. Otherwise the list buffers hold `total` entries between two guard
    zones of GUARD sentinels and are returned WITH the guards. -> (counts or None, list or None, inside flags or None, counters)."""
    q = _aligned(np.ascontiguousarray(planes, dtype=tree.dtype))
    n, m = q.shape[0], q.shape[1]
    cnt = np.zeros(3, dtype=np.uint64)
    c = np.full(n, 0xABABABAB, dtype=np.uint32) if counts else None
    off = lp = lp_arg = li = li_arg = None
    if offsets is not None:
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        lp = np.full(total + 2 * GUARD, SENT_PRIM, dtype=np.uint32)
        lp_arg = lp[GUARD:].ctypes.data_as(C.c_void_p)
        if inside:
            li = np.full(total + 2 * GUARD, SENT_INSIDE, dtype=np.uint8)
            li_arg = li[GUARD:].ctypes.data_as(C.c_void_p)
    assert dll.region_host_walk(int(tree.double), _p(tree.pairs), tree.root, _p(tree.prims), _p(tree.ids), tree.leaf, int(exact), _p(q), m, n,
                                int(original_ids), deep_cap, threads, _p(c), _p(off), lp_arg, li_arg, _p(cnt)) == 0
    return c, lp, li, cnt


def inside_guards_intact(li, total):
    return bool((li[:GUARD] == SENT_INSIDE).all() and (li[GUARD + total:] == SENT_INSIDE).all())


def host_region(dll, tree, planes, **kw):
    """Count, offsets, fill with inside flags: (offsets (n + 1) uint64, ids, inside flags, counts, counters of the fill pass). Checks
    what every such call must satisfy: the fill pass reports the counts of the count pass, exact offsets leave no padding, the guard
    zones stay untouched."""
    counts, _, _, cnt0 = host_walk(dll, tree, planes, **kw)
    offsets = np.concatenate([[0], np.cumsum(counts.astype(np.uint64))]).astype(np.uint64)
    total = int(offsets[-1])
    c2, lp, li, cnt = host_walk(dll, tree, planes, offsets=offsets, total=total, inside=True, **kw)
    assert (c2 == counts).all() and (cnt == cnt0).all()
    assert guards_intact(lp, total) and inside_guards_intact(li, total)
    ids, ins = lp[GUARD:GUARD + total], li[GUARD:GUARD + total]
    assert (ids != INVALID).all() and (ins <= 1).all()
    return offsets, ids, ins, counts, cnt


def expected_inside(match, inside, dfs):
    """The inside flags beside expected_lists(match, dfs)[1]."""
    w = match[:, dfs]
    return inside[:, dfs][w].astype(np.uint8)
