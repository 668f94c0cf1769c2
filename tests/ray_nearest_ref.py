"""What the nearest-hits ray tests (tests/test_ray_nearest_host.py, tests/test_gpu_ray_nearest.py) share: the host harness
(tests/cpp/ray_nearest_body_host.cpp) and its call, the expected rows — each ray's list from the UNMODIFIED reference
(tests/ray_hits_ref.py: reference_records / expected_lists) sorted by (t, prim) and cut at k — and the scene in which t ties."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle
from conftest import ROOT
from query_slices import knn_block_lanes
from ray_hits_ref import INVALID, build_tree, expected_lists, reference_records

HARNESS = os.path.join(ROOT, "tests", "cpp", "ray_nearest_body_host.cpp")
GUARD = 8                                                      # sentinel records / words on either side of an output buffer
SENT_BYTE = 0xA5
SENT_COUNT = 0xABABABAB
K_DENSE = [1, 2, 3, 8, 9, 16, 17, 33, 64]                      # the 200-primitive and golden scenes
K_TINY = [1, 2, 64]                                            # scenes of 1, 2 and 3 primitives
MAX_K = 64


def compile_harness(out_dir):
    out = os.path.join(str(out_dir), "libray_nearest_body_host.so")
    cmd = ["g++", "-std=c++20", "-O1", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-strict-aliasing", "-Wall", "-Wextra", "-Wno-unused-parameter",
           "-Wno-unknown-pragmas", "-Werror", "-shared", "-fPIC", "-pthread", HARNESS, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    dll = C.CDLL(out)
    P, Z, I, U = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32
    dll.ray_nearest_host_walk.restype = I
    dll.ray_nearest_host_walk.argtypes = [I, I, I, I, P, U, P, P, Z, U, U, P, P, U, I, P, P, P]
    dll.ray_nearest_host_walk_slice.restype = C.c_longlong
    dll.ray_nearest_host_walk_slice.argtypes = [I, I, I, P, U, P, P, Z, Z, Z, U, U, P, P, U, P, P, P]
    return dll


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def hit_dtype(tree):
    return oracle.HITD if tree.double else oracle.HITF


def block_lanes(tree, k):
    """Lanes per block the launch path picks for k (point_query.h: knn_block_lanes): the stride of the LDS arrays."""
    return knn_block_lanes(k, 8 if tree.double else 4)


def guarded_records(dtype, total):
    """`total` records between two zones of GUARD records, every byte SENT_BYTE, aligned to 32 bytes: (whole buffer, the records)."""
    nbytes = (total + 2 * GUARD) * dtype.itemsize
    raw = np.empty(nbytes + 32, dtype=np.uint8)
    off = (-raw.ctypes.data) % 32
    buf = raw[off:off + nbytes]
    buf[:] = SENT_BYTE
    buf = buf.view(dtype)
    return buf, buf[GUARD:GUARD + total]


def record_guards_intact(buf, total):
    b = buf.view(np.uint8).reshape(len(buf), -1)
    return bool((b[:GUARD] == SENT_BYTE).all() and (b[GUARD + total:] == SENT_BYTE).all())


def host_nearest(dll, tree, rays, k, robust=False, stride=None, counts=True, order=None, prim_ids=None, deep_cap=0, threads=1, mutant=0):
    """One call of the kernel's walk -> (rows (n, k) records, counts (n,) or None, counters). The row buffer and the counts sit between
    guard zones, which must come back untouched; the LDS stand-in's guards are the harness's (return code 2)."""
    from test_kernel_body_host import _aligned
    r = _aligned(np.ascontiguousarray(rays, dtype=tree.dtype))
    n = len(r)
    cnt = np.zeros(3, dtype=np.uint64)
    buf, rows = guarded_records(hit_dtype(tree), n * k)
    c = np.full(n + 2 * GUARD, SENT_COUNT, dtype=np.uint32) if counts else None
    order = None if order is None else np.ascontiguousarray(order, dtype=np.uint32)
    prim_ids = None if prim_ids is None else np.ascontiguousarray(prim_ids, dtype=np.uint32)
    rc = dll.ray_nearest_host_walk(int(tree.double), tree.leaf, int(robust), mutant, _p(tree.pairs), tree.root, _p(tree.prims), _p(r), n, k,
                                   stride or block_lanes(tree, k), _p(order), _p(prim_ids), deep_cap, threads, _p(rows),
                                   None if c is None else c[GUARD:].ctypes.data_as(C.c_void_p), _p(cnt))
    assert rc == 0, rc
    assert record_guards_intact(buf, n * k)
    if c is not None:
        assert (c[:GUARD] == SENT_COUNT).all() and (c[GUARD + n:] == SENT_COUNT).all()
        c = c[GUARD:GUARD + n].copy()
    return rows.reshape(n, k).copy(), c, cnt


def miss_rows(tree, rays, k):
    """(n, k) of intersect's miss record {INVALID, the ray's tmax bits, 0, 0}."""
    rays = np.ascontiguousarray(rays, dtype=tree.dtype)
    m = np.zeros((len(rays), k), dtype=hit_dtype(tree))
    m["prim"] = INVALID
    bits = np.uint64 if tree.double else np.uint32
    t = np.zeros((len(rays), k), dtype=tree.dtype)
    t.view(bits)[:] = np.ascontiguousarray(rays[:, 7]).view(bits)[:, None]      # (the bits, not the value: a NaN keeps its payload)
    m["t"] = t
    return m


def sorted_lists(hit, rec, index):
    """The reference's list of every ray sorted by (t, BVH-order prim): (all-hits counts, [records of ray r])."""
    counts, flat = expected_lists(hit, rec, index)
    off = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    return counts, [np.sort(flat[off[r]:off[r + 1]], order=["t", "prim"]) for r in range(len(counts))]


def expected_rows(tree, rays, lists, k, prim_ids=None):
    """The rows the contract asks for: each sorted list cut at k (prim mapped through prim_ids AFTER the sort), padded with the miss
    record. -> (rows (n, k), counts (n,) uint32)."""
    rows = miss_rows(tree, rays, k)
    counts = np.zeros(len(lists), dtype=np.uint32)
    for r, seg in enumerate(lists):
        m = min(len(seg), k)
        rows[r, :m] = seg[:m]
        if prim_ids is not None:
            rows["prim"][r, :m] = np.asarray(prim_ids)[seg["prim"][:m].astype(np.int64)]
        counts[r] = m
    return rows, counts


def differing_rows(got, want):
    """How many rows differ in any byte."""
    g = got.view(np.uint8).reshape(got.shape[0], -1)
    w = want.view(np.uint8).reshape(want.shape[0], -1)
    return int((g != w).any(axis=1).sum())


def first_two_tie(lists):
    """Per ray: its sorted list has at least two records and the first two have the same t."""
    return np.array([len(s) >= 2 and s["t"][0] == s["t"][1] for s in lists])


def layered_grid(n_rays, seed=11):
    """The scene in which t ties exactly: 8 layers z = j / 8 of 4 x 4 quads over the unit square, each quad two triangles with the
    first of them duplicated (384 triangles), and rays from (a / 32, b / 32, -1) along +z, tmin 0, tmax 4, a and b seeded integers in
    [0, 32]: every coordinate is a small multiple of a power of two, so a duplicated triangle gives the same t bits twice, and rays on
    a quad's diagonal or edge cross neighbours at one t as well. -> (raw (384, 9) float32, rays (n_rays, 8) float32)."""
    tris = []
    for j in range(8):
        z = j / 8
        for qx in range(4):
            for qy in range(4):
                x0, x1, y0, y1 = qx / 4, (qx + 1) / 4, qy / 4, (qy + 1) / 4
                first = [x0, y0, z, x1, y0, z, x1, y1, z]
                tris += [first, first, [x0, y0, z, x1, y1, z, x0, y1, z]]
    raw = np.array(tris, dtype=np.float32)
    assert raw.shape == (384, 9)
    rng = np.random.default_rng(seed)
    rays = np.zeros((n_rays, 8), dtype=np.float32)
    rays[:, 0] = rng.integers(0, 33, n_rays) / 32
    rays[:, 1] = rng.integers(0, 33, n_rays) / 32
    rays[:, 2], rays[:, 5], rays[:, 7] = -1, 1, 4
    return raw, rays


_GRID = {}


def grid_case(lib, n_rays=256):
    """layered_grid under the reference's default build, with the reference's records: (tree, rays, {robust: (hit, rec)}, ids, nodes),
    computed once and shared, never changed."""
    from test_radius_search_host import Tree
    if n_rays not in _GRID:
        raw, rays = layered_grid(n_rays)
        nodes, ids, prims = build_tree(lib, raw, False)
        tree = Tree(nodes["bounds"], nodes["index"], prims, 0)
        ref = {rb: reference_records(lib, nodes, prims, rays, 0, rb) for rb in (False, True)}
        _GRID[n_rays] = (tree, rays, ref, ids, nodes)
    return _GRID[n_rays]
