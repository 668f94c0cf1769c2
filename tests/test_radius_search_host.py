"""CPU: the TEXT of the radius-query kernel (bvh_amd/csrc/radius_body.inc + list_walk.inc + point_walk.inc + trace_device.h) compiled for the host by
tests/cpp/radius_body_host.cpp. The walk over the golden trees against a brute force over the same distance functions, filtered in
the tree's left-first depth-first order; the shapes of the output (count pass, exact offsets, fixed segments, padding, guard zones);
edge queries; trees deeper than 64 levels; the exported symbols. The device's counts, lists and distances must equal this harness's
bit for bit (tests/test_gpu_radius_search.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_closest_point_host import GOLDEN_SCENES, chain_queries, chain_tree, golden_scene, precompute, scene_queries
from test_kernel_body_host import _aligned, pair_records

HARNESS = os.path.join(ROOT, "tests", "cpp", "radius_body_host.cpp")
INVALID = 0xFFFFFFFF
GUARD = 64                                                     # sentinel entries on either side of a list buffer
SENT_PRIM = 0xDEADBEEF
SENT_DIST = -12345.0


def compile_harness(out_dir):
    out = os.path.join(str(out_dir), "libradius_body_host.so")
    cmd = ["g++", "-std=c++20", "-O1", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-strict-aliasing", "-Wall", "-Wextra", "-Wno-unused-parameter",
           "-Wno-unknown-pragmas", "-Werror", "-shared", "-fPIC", "-pthread", HARNESS, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    dll = C.CDLL(out)
    P, Z, I, U = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32
    dll.radius_host_walk.restype = I
    dll.radius_host_walk.argtypes = [I, I, P, U, P, P, Z, P, P, U, I, P, P, P, P, P]
    dll.radius_host_brute.argtypes = [I, I, P, Z, P, Z, P, I]
    return dll


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Tree:
    """What the harness walks: pair records, root word, BVH-order primitives, leaf kind (0 triangles, 1 spheres)."""

    def __init__(self, bounds6, index, prims, leaf):
        self.double = bounds6.dtype == np.float64
        self.pairs = _aligned(pair_records(bounds6, index))
        self.root = int(index[0]) & 0xFFFFFFFF
        self.prims = _aligned(np.ascontiguousarray(prims))
        self.leaf = leaf
        self.index = np.asarray(index)
        self.dtype = self.prims.dtype


def host_walk(dll, tree, queries, offsets=None, total=0, counts=True, dist=True, order=None, prim_ids=None, deep_cap=0, threads=1):
    """One call of the kernel's walk. offsets None: the count pass. Otherwise the list buffers hold `total` entries between two guard
    zones of GUARD sentinels and are returned WITH the guards. -> (counts or None, list prims or None, list dist or None, counters)."""
    q = _aligned(np.ascontiguousarray(queries, dtype=tree.dtype))
    n = len(q)
    cnt = np.zeros(3, dtype=np.uint64)
    c = np.full(n, 0xABABABAB, dtype=np.uint32) if counts else None
    off = lp = ld = None
    lp_arg = ld_arg = None
    if offsets is not None:
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        lp = np.full(total + 2 * GUARD, SENT_PRIM, dtype=np.uint32)
        lp_arg = lp[GUARD:].ctypes.data_as(C.c_void_p)
        if dist:
            ld = np.full(total + 2 * GUARD, SENT_DIST, dtype=tree.dtype)
            ld_arg = ld[GUARD:].ctypes.data_as(C.c_void_p)
    order = None if order is None else np.ascontiguousarray(order, dtype=np.uint32)
    prim_ids = None if prim_ids is None else np.ascontiguousarray(prim_ids, dtype=np.uint32)
    assert dll.radius_host_walk(int(tree.double), tree.leaf, _p(tree.pairs), tree.root, _p(tree.prims), _p(q), n, _p(order), _p(prim_ids), deep_cap,
                                threads, _p(c), _p(off), lp_arg, ld_arg, _p(cnt)) == 0
    return c, lp, ld, cnt


def guards_intact(lp, total, ld=None):
    """The sentinels on either side of the `total` list entries (and of the distances beside them, if any) are untouched."""
    ok = (lp[:GUARD] == SENT_PRIM).all() and (lp[GUARD + total:] == SENT_PRIM).all()
    if ld is not None:
        ok = ok and (ld[:GUARD] == SENT_DIST).all() and (ld[GUARD + total:] == SENT_DIST).all()
    return bool(ok)


def host_radius(dll, tree, queries, **kw):
    """Count, offsets, fill: (offsets (n + 1) uint64, ids, dist, counts, counters of the fill pass). Checks what every such call must
    satisfy: the fill pass reports the counts of the count pass, exact offsets leave no padding, the guard zones stay untouched."""
    counts, _, _, cnt0 = host_walk(dll, tree, queries, **kw)
    offsets = np.concatenate([[0], np.cumsum(counts.astype(np.uint64))]).astype(np.uint64)
    total = int(offsets[-1])
    c2, lp, ld, cnt = host_walk(dll, tree, queries, offsets=offsets, total=total, **kw)
    assert (c2 == counts).all() and (cnt == cnt0).all()
    assert guards_intact(lp, total, ld)
    ids, dist = lp[GUARD:GUARD + total], ld[GUARD:GUARD + total]
    if kw.get("prim_ids") is None:
        assert (ids < len(tree.prims)).all()
    else:
        assert (ids != INVALID).all()
    return offsets, ids, dist, counts, cnt


def host_brute(dll, tree, queries, threads=4):
    """d2[k, i]: the kernel's squared distance of query k to BVH-order primitive i."""
    q = np.ascontiguousarray(queries, dtype=tree.dtype)
    out = np.zeros((len(q), len(tree.prims)), dtype=tree.dtype)
    dll.radius_host_brute(int(tree.double), tree.leaf, _p(tree.prims), len(tree.prims), _p(q), len(q), _p(out), threads)
    return out


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


def _queries(pts, r, dt):
    q = np.zeros((len(pts), 4), dtype=dt)
    q[:, :3] = pts
    q[:, 3] = r
    return q


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return compile_harness(tmp_path_factory.mktemp("radius"))


@pytest.mark.parametrize("scene", GOLDEN_SCENES)
@pytest.mark.parametrize("mode", ["serial_low", "parallel_high"])
def test_walk_equals_brute_force(dll, orc, scene, mode):
    bounds, index, prims, leaf, raw, _ = golden_scene(scene, mode, orc)
    tree = Tree(bounds, index, prims, leaf)
    dt = tree.dtype
    pts, diag = scene_queries(raw, 1024, dt, 11, leaf == 1)     # 1024 uniform, and for triangles 1024 more near the surface
    dfs = dfs_prim_order(index)
    assert len(dfs) == len(prims) and len(set(dfs.tolist())) == len(prims)
    pos = np.empty(len(prims), dtype=np.int64)
    pos[dfs] = np.arange(len(dfs))
    tol = 8 * np.finfo(dt).eps * (1.0 + float(np.abs(raw).max()) + diag)
    d2 = host_brute(dll, tree, _queries(pts, 0, dt))
    d2_dfs = d2[:, dfs]
    expected_total = lacking_total = 0
    for frac in (0.05, 0.1):
        r = np.asarray(frac * diag, dtype=dt)
        q = _queries(pts, r, dt)
        offsets, ids, dist, counts, cnt = host_radius(dll, tree, q, threads=4)
        assert cnt[0] > 0 and cnt[1] > 0 and cnt[2] > 0
        within = d2_dfs <= r * r                                # (r * r rounded in the scalar type, as the kernel does)
        n_expected = int(within.sum())
        lacking = 0
        for k in range(len(q)):
            got = ids[int(offsets[k]):int(offsets[k + 1])].astype(np.int64)
            p = pos[got]
            assert (np.diff(p) > 0).all(), (scene, k)          # (1) in the expected order ...
            assert within[k, p].all(), (scene, k)              # ... and nothing the brute force does not list
            assert (dist[int(offsets[k]):int(offsets[k + 1])] == np.sqrt(d2[k, got])).all()
            missed = within[k].copy()
            missed[p] = False
            if missed.any():                                   # (2) only pairs within rounding of the boundary may be lacking
                dm = np.sqrt(d2_dfs[k, missed].astype(np.float64))
                assert (np.abs(dm - float(r)) <= tol).all(), (scene, k, dm, float(r))
                lacking += int(missed.sum())
        mean_len = n_expected / len(q)
        print(f"{scene} {mode} r={frac} diag: expected {n_expected} pairs (mean list {mean_len:.2f}), lacking {lacking}")
        assert 1.0 <= mean_len <= len(prims) / 4, (scene, frac, mean_len)       # not vacuous
        expected_total += n_expected
        lacking_total += lacking
    assert lacking_total <= 0.001 * expected_total, (scene, lacking_total, expected_total)   # (3) a cap, not a tolerance


def test_output_shapes(dll, orc):
    bounds, index, prims, leaf, raw, _ = golden_scene("soup2k", "parallel_high", orc)
    tree = Tree(bounds, index, prims, leaf)
    pts, diag = scene_queries(raw, 300, np.float32, 5, False)
    q = _queries(pts, np.float32(0.1 * diag), np.float32)
    n = len(q)
    offsets, ids, dist, counts, _ = host_radius(dll, tree, q)       # count pass == list lengths, no padding, guards: checked inside
    assert counts.max() > 4 and (counts == 0).any() and (counts > 0).any()
    # without the optional outputs: same lists
    _, lp, ld, _ = host_walk(dll, tree, q, offsets=offsets, total=len(ids), counts=False, dist=False)
    assert ld is None and (lp[GUARD:GUARD + len(ids)] == ids).all() and guards_intact(lp, len(ids))
    # k = 4 slots per query, the buffer starting at a non-zero offset: prefix in walk order, padding, untruncated counts, guards
    k, base = 4, 7
    fixed = (base + k * np.arange(n + 1)).astype(np.uint64)
    total = base + k * n + 5                                   # entries before offsets[0] and after offsets[n] belong to nobody
    c4, lp, ld, _ = host_walk(dll, tree, q, offsets=fixed, total=total)
    assert (c4 == counts).all()
    assert (lp[GUARD:GUARD + base] == SENT_PRIM).all() and (lp[GUARD + base + k * n:] == SENT_PRIM).all()
    assert (ld[GUARD:GUARD + base] == SENT_DIST).all() and (ld[GUARD + base + k * n:] == SENT_DIST).all() and guards_intact(lp, total, ld)
    seg_p = lp[GUARD + base:GUARD + base + k * n].reshape(n, k)
    seg_d = ld[GUARD + base:GUARD + base + k * n].reshape(n, k)
    for i in range(n):
        m = min(int(counts[i]), k)
        full = ids[int(offsets[i]):int(offsets[i + 1])]
        assert (seg_p[i, :m] == full[:m]).all() and (seg_d[i, :m] == dist[int(offsets[i]):int(offsets[i]) + m]).all()
        assert (seg_p[i, m:] == INVALID).all() and (seg_d[i, m:] == q[i, 3]).all()
    # stale offsets: a segment that ends before it begins is empty, the others (here all [0, 9)) are kept to; counts are still reported
    stale = np.zeros(n + 1, dtype=np.uint64)
    stale[::2] = 9
    c5, lp, ld, _ = host_walk(dll, tree, q, offsets=stale, total=16)
    assert (c5 == counts).all()
    written = lp[GUARD:GUARD + 16] != SENT_PRIM
    assert not written[9:].any() and guards_intact(lp, 16, ld)


def test_edge_queries(dll, orc):
    bounds, index, prims, leaf, raw, ids = golden_scene("cornell", "serial_low", orc)
    tree = Tree(bounds, index, prims, leaf)
    c = raw.reshape(-1, 3).mean(axis=0)
    on = raw.reshape(-1, 3)[5]                                   # a vertex: at distance exactly 0 of its triangles
    q = np.array([[c[0], c[1], c[2], np.inf], [np.nan, c[1], c[2], np.inf], [c[0], np.nan, c[2], 1.0], [c[0], c[1], c[2], -1.0],
                  [c[0], c[1], c[2], np.nan], [on[0], on[1], on[2], 0.0], [c[0], c[1], c[2], 1e30], [c[0], c[1], c[2], -np.inf]], dtype=np.float32)
    offsets, lst, dist, counts, _ = host_radius(dll, tree, q)
    dfs = dfs_prim_order(index)
    assert len(dfs) == 36
    seg = lambda k: lst[int(offsets[k]):int(offsets[k + 1])]
    assert (seg(0) == dfs).all() and (seg(6) == dfs).all()       # +inf (and a radius whose square overflows): everything, in DFS order
    for k in (1, 2, 3, 4, 7):
        assert counts[k] == 0
    d2 = host_brute(dll, tree, q)
    assert counts[5] >= 1 and set(seg(5).tolist()) == set(np.flatnonzero(d2[5] == 0).tolist())
    assert (dist[int(offsets[5]):int(offsets[6])] == 0).all()
    assert (dist[int(offsets[0]):int(offsets[1])] == np.sqrt(d2[0, dfs])).all()
    # invalid queries with a segment: padded with INVALID and their own max_distance, bit for bit
    fixed = (2 * np.arange(len(q) + 1)).astype(np.uint64)
    _, lp, ld, _ = host_walk(dll, tree, q, offsets=fixed, total=2 * len(q))
    lp, ld = lp[GUARD:-GUARD].reshape(-1, 2), ld[GUARD:-GUARD].reshape(-1, 2)
    for k in (1, 2, 3, 4, 7):
        assert (lp[k] == INVALID).all() and ld[k].tobytes() == np.repeat(q[k, 3], 2).tobytes()
    # original ids: the same walk, mapped through prim_ids
    oo, ol, od, oc, _ = host_radius(dll, tree, q, prim_ids=ids.astype(np.uint32))
    assert (oo == offsets).all() and (ol == ids[lst.astype(np.int64)]).all() and od.tobytes() == dist.tobytes()
    # reading the batch through a permuted order changes nothing
    pts, diag = scene_queries(raw, 200, np.float32, 9, False)
    q2 = _queries(pts, np.float32(0.2 * diag), np.float32)
    base = host_radius(dll, tree, q2)
    perm = np.random.default_rng(5).permutation(len(q2)).astype(np.uint32)
    again = host_radius(dll, tree, q2, order=perm)
    for x, y in zip(base, again):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("depth", [65, 300])
def test_deep_chain(dll, orc, depth):
    tris, nodes, _ = chain_tree(depth, orc.prep_tris)
    tree = Tree(nodes["bounds"], nodes["index"], precompute(tris, np.float32), 0)
    q = chain_queries(depth, 300)                              # 300: not a multiple of the block
    dfs = dfs_prim_order(nodes["index"])
    assert (dfs == np.arange(depth + 1)).all()
    offsets, ids, dist, counts, _ = host_radius(dll, tree, q, deep_cap=depth - 64 + 1)
    d2 = host_brute(dll, tree, q)
    assert (counts == depth + 1).all() and (ids.reshape(len(q), depth + 1) == dfs).all()
    assert (dist.reshape(len(q), depth + 1) == np.sqrt(d2)).all()
    # a radius that reaches only the far end of the chain (the triangles sit at x = 4000 - k; the queries at x in [0, 100))
    q[:, 3] = np.float32(4000 - depth + 10.5) - q[:, 0]
    offsets, ids, dist, counts, _ = host_radius(dll, tree, q, deep_cap=depth - 64 + 1)
    within = d2 <= (q[:, 3] * q[:, 3])[:, None]
    assert (counts == within.sum(axis=1)).all() and 0 < counts.min() and counts.max() < 20
    for k in range(len(q)):
        assert (ids[int(offsets[k]):int(offsets[k + 1])] == np.flatnonzero(within[k])).all()


def test_deep_chain_fills_the_spill(dll, orc):
    """The chain with every inner child on the left, so that this left-first walk stacks one leaf per level: 70 levels cross LDS ->
    scratch (entry 16), scratch -> HBM (entry 64) and end on the last of the 6 HBM entries given."""
    depth = 70
    tris, nodes, _ = chain_tree(depth, orc.prep_tris)
    nodes[1::2], nodes[2::2] = nodes[2::2].copy(), nodes[1::2].copy()
    tree = Tree(nodes["bounds"], nodes["index"], precompute(tris, np.float32), 0)
    q = chain_queries(depth, 48)
    dfs = dfs_prim_order(nodes["index"])
    assert (dfs == np.arange(depth, -1, -1)).all()
    offsets, ids, dist, counts, _ = host_radius(dll, tree, q, deep_cap=depth - 64)
    d2 = host_brute(dll, tree, q)
    assert (counts == depth + 1).all() and (ids.reshape(len(q), depth + 1) == dfs).all()
    assert (dist.reshape(len(q), depth + 1) == np.sqrt(d2)[:, dfs]).all()


def test_radius_symbols_are_declared_and_exported():
    from bvh_amd import _lib, build
    build.build()
    dll = _lib.load()
    header = open(os.path.join(ROOT, "include", "bvh_amd.h")).read()
    declared = set(re.findall(r"BVH_AMD_API[^;]*?\b(bvh\w+)\s*\(", header))
    want = {f"bvh{s}_radius_search_{leaf}" for s in ("3f", "3d") for leaf in ("tri", "sphere")} | {"bvh_amd_offsets_from_counts"}
    mine = {n for n in declared if "radius" in n or "offsets_from_counts" in n}
    assert mine == want
    assert want <= set(_lib.exported_symbols())
    for name in sorted(want):
        assert hasattr(dll, name), name
    for s in ("2f", "2d"):
        for leaf in ("tri", "sphere"):
            assert not hasattr(dll, f"bvh{s}_radius_search_{leaf}")
            assert f"bvh{s}_radius_search_{leaf}" not in _lib.exported_symbols()
