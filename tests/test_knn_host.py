"""CPU: the TEXT of the k-nearest kernel (bvh_amd/csrc/knn_body.inc + point_walk.inc + trace_device.h) compiled for the host by
tests/cpp/knn_body_host.cpp. The walk over the golden trees against the k smallest (d2, index) pairs of a brute force over the same
distance functions; k = 1 against the closest-point harness, byte for byte; short rows against the radius harness's lists; edge
queries, padding and guard zones; trees deeper than 64 levels; the lane stride of the LDS arrays; the exported symbols. The device's
rows, counts and counters must equal this harness's bit for bit (tests/test_gpu_knn.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import test_closest_point_host as closest_host
from conftest import ROOT
from test_closest_point_host import GOLDEN_SCENES, chain_queries, chain_tree, golden_scene, precompute, scene_queries
from test_radius_search_host import GUARD, INVALID, SENT_DIST, SENT_PRIM, Tree, host_brute, host_radius
from test_radius_search_host import compile_harness as compile_radius_harness

HARNESS = os.path.join(ROOT, "tests", "cpp", "knn_body_host.cpp")
MAX_K = 64


def compile_harness(out_dir):
    out = os.path.join(str(out_dir), "libknn_body_host.so")
    cmd = ["g++", "-std=c++20", "-O1", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-strict-aliasing", "-Wall", "-Wextra", "-Wno-unused-parameter",
           "-Wno-unknown-pragmas", "-Werror", "-shared", "-fPIC", "-pthread", HARNESS, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    dll = C.CDLL(out)
    P, Z, I, U = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32
    dll.knn_host_walk.restype = I
    dll.knn_host_walk.argtypes = [I, I, P, U, P, P, Z, U, U, P, P, U, I, P, P, P, P]
    return dll


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_knn(dll, tree, queries, k, stride=256, dist=True, counts=True, order=None, prim_ids=None, deep_cap=0, threads=1):
    """One call of the kernel's walk: (ids (n, k) uint32, dist (n, k) or None, counts (n,) or None, counters). The rows are written
    between two guard zones of GUARD sentinels, which must come back untouched."""
    from test_kernel_body_host import _aligned
    q = _aligned(np.ascontiguousarray(queries, dtype=tree.dtype))
    n = len(q)
    cnt = np.zeros(3, dtype=np.uint64)
    c = np.full(n, 0xABABABAB, dtype=np.uint32) if counts else None
    op = np.full(n * k + 2 * GUARD, SENT_PRIM, dtype=np.uint32)
    od = np.full(n * k + 2 * GUARD, SENT_DIST, dtype=tree.dtype) if dist else None
    order = None if order is None else np.ascontiguousarray(order, dtype=np.uint32)
    prim_ids = None if prim_ids is None else np.ascontiguousarray(prim_ids, dtype=np.uint32)
    assert dll.knn_host_walk(int(tree.double), tree.leaf, _p(tree.pairs), tree.root, _p(tree.prims), _p(q), n, k, stride, _p(order), _p(prim_ids), deep_cap,
                             threads, op[GUARD:].ctypes.data_as(C.c_void_p), None if od is None else od[GUARD:].ctypes.data_as(C.c_void_p), _p(c), _p(cnt)) == 0
    assert (op[:GUARD] == SENT_PRIM).all() and (op[GUARD + n * k:] == SENT_PRIM).all()
    assert od is None or ((od[:GUARD] == SENT_DIST).all() and (od[GUARD + n * k:] == SENT_DIST).all())
    return op[GUARD:GUARD + n * k].reshape(n, k).copy(), None if od is None else od[GUARD:GUARD + n * k].reshape(n, k).copy(), c, cnt


def _queries(pts, r, dt):
    q = np.zeros((len(pts), 4), dtype=dt)
    q[:, :3] = pts
    q[:, 3] = r
    return q


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def brute_order(d2, r2):
    """Every row of the brute-force matrix sorted by (d2, i), the primitives beyond r2 last: (d2 with inf beyond r2, sorted indices,
    primitives within r2 per row). Computed once per radius and shared by the k of a case."""
    within = d2 <= r2
    masked = np.where(within, d2, np.inf)
    return masked, np.argsort(masked, axis=1, kind="stable"), within.sum(axis=1)    # (stable: equal d2 by ascending index)


def expected_rows(brute, k):
    """The k smallest (d2, i) with d2 <= r2 of every row: (ids (n, k) int64, d2 (n, k), counts (n,)); the slots beyond a row's count
    hold -1 / inf."""
    masked, order, n_within = brute
    ids = order[:, :k]
    if ids.shape[1] < k:
        ids = np.concatenate([ids, np.zeros((len(ids), k - ids.shape[1]), dtype=ids.dtype)], axis=1)
    counts = np.minimum(n_within, k)
    valid = np.arange(k)[None, :] < counts[:, None]
    ed2 = np.where(valid, np.take_along_axis(masked, ids, axis=1), np.inf)
    return np.where(valid, ids, -1), ed2, counts


def check_rows(ids, dist, counts, d2, r, k, tol, brute=None):
    """What every row must satisfy against the brute-force matrix d2 (n x prims), radius r (scalar of the tree's type; brute =
    brute_order(d2, r * r), if the caller has it). Returns (rows that differ from the expected ones, entries that differ, counts that
    differ, equal-d2 neighbours listed)."""
    n = len(ids)
    r2 = r * r                                                # (rounded in the scalar type, as the kernel does)
    valid = np.arange(k)[None, :] < counts[:, None]
    assert (counts <= k).all()
    assert (ids[~valid] == INVALID).all() and (ids[valid] < d2.shape[1]).all()
    assert (_bits(dist)[~valid] == _bits(np.asarray([r], dtype=dist.dtype))[0]).all()            # the padding, bit for bit
    gi = np.where(valid, ids, 0).astype(np.int64)
    gd2 = np.take_along_axis(d2, gi, axis=1)
    assert (gd2[valid] <= r2).all()
    assert _bits(dist[valid]).tobytes() == _bits(np.sqrt(gd2[valid])).tobytes()                   # sqrt of the matrix entry, bit for bit
    pair = valid[:, 1:]                                       # (valid[:, j + 1] implies valid[:, j])
    asc = (gd2[:, :-1] < gd2[:, 1:]) | ((gd2[:, :-1] == gd2[:, 1:]) & (gi[:, :-1] < gi[:, 1:]))
    assert asc[pair].all()                                    # strictly ascending in (d2, i)
    ties = int(((gd2[:, :-1] == gd2[:, 1:]) & pair).sum())
    eids, ed2, ecounts = expected_rows(brute if brute is not None else brute_order(d2, r2), k)
    assert (counts <= ecounts).all()                          # the walk tests a subset of what the brute force tests ...
    both = np.arange(k)[None, :] < np.minimum(counts, ecounts)[:, None]
    assert (gd2[both] >= ed2[both]).all()                     # ... with the same function: its j-th d2 is never below the brute force's
    diff = np.where(valid, gi, -1) != eids
    rows = diff.any(axis=1)
    gap = np.abs(np.sqrt(gd2.astype(np.float64)) - np.sqrt(np.where(both, ed2, 0).astype(np.float64)))
    assert (gap[both & rows[:, None]] <= tol).all()
    # Counts: min(k, primitives within the radius). Only a primitive within rounding of the radius can be lacking (its box computed
    # farther than r2), so wherever no distance of the row is within tol of the radius the counts are equal — the rows whose k-th and
    # (k + 1)-th distances are within tol of each other included.
    if np.isfinite(r):
        clear = ~(np.abs(np.sqrt(d2.astype(np.float64)) - float(r)) <= tol).any(axis=1)
    else:
        clear = np.ones(n, dtype=bool)
    assert (counts[clear] == ecounts[clear]).all()
    return int(rows.sum()), int(diff.sum()), int((counts != ecounts).sum()), ties


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return compile_harness(tmp_path_factory.mktemp("knn"))


@pytest.fixture(scope="module")
def closest_dll(tmp_path_factory):
    return closest_host.compile_harness(tmp_path_factory.mktemp("knn_closest"))


@pytest.fixture(scope="module")
def radius_dll(tmp_path_factory):
    return compile_radius_harness(tmp_path_factory.mktemp("knn_radius"))


@pytest.mark.parametrize("scene", GOLDEN_SCENES)
@pytest.mark.parametrize("mode", ["serial_low", "parallel_high"])
def test_walk_equals_brute_force(dll, radius_dll, orc, scene, mode):
    bounds, index, prims, leaf, raw, _ = golden_scene(scene, mode, orc)
    tree = Tree(bounds, index, prims, leaf)
    dt = tree.dtype
    pts, diag = scene_queries(raw, 1024, dt, 11, leaf == 1)     # 1024 uniform, and for triangles 1024 more near the surface
    tol = 8 * np.finfo(dt).eps * (1.0 + float(np.abs(raw).max()) + diag)
    d2 = host_brute(radius_dll, tree, _queries(pts, 0, dt))
    entries = differing = 0
    for r in (np.asarray(np.inf, dtype=dt), np.asarray(0.05 * diag, dtype=dt)):
        q = _queries(pts, r, dt)
        brute = brute_order(d2, r[()] * r[()])                   # (r * r rounded in the scalar type, as the kernel does)
        for k in (1, 3, 8, 17, 64):
            ids, dist, counts, cnt = host_knn(dll, tree, q, k, threads=4)
            assert cnt[0] > 0 and cnt[1] > 0 and cnt[2] > 0
            rows, ents, cdiff, ties = check_rows(ids, dist, counts, d2, r[()], k, tol, brute)
            print(f"{scene} {mode} r={float(r):.4g} k={k}: {rows} of {len(q)} rows differ ({ents} entries), {cdiff} counts differ, "
                  f"{ties} equal-d2 neighbour pairs, mean count {counts.mean():.2f}, tests/query {int(cnt[1]) / len(q):.1f}")
            assert rows <= 0.01 * len(q), (scene, mode, float(r), k, rows)                        # a cap, not a tolerance
            entries += ids.size
            differing += ents
    assert differing <= 0.001 * entries, (scene, mode, differing, entries)


@pytest.mark.parametrize("scene", ["cornell", "terrain2k", "spheres2k_f64"])
def test_k1_equals_closest_points(dll, closest_dll, orc, scene):
    bounds, index, prims, leaf, raw, _ = golden_scene(scene, "parallel_high", orc)
    tree = Tree(bounds, index, prims, leaf)
    dt = tree.dtype
    pts, diag = scene_queries(raw, 1024, dt, 11, leaf == 1)
    for r in (np.inf, 0.05 * diag):
        q = _queries(pts, r, dt)
        hits, ccnt = closest_host.host_walk(closest_dll, bounds, index, prims, q, leaf, threads=4)
        ids, dist, counts, cnt = host_knn(dll, tree, q, 1, threads=4)
        assert ids[:, 0].tobytes() == np.ascontiguousarray(hits["prim"]).tobytes()
        assert dist[:, 0].tobytes() == np.ascontiguousarray(hits["t"]).tobytes()
        assert (counts == (hits["prim"] != INVALID)).all()
        assert cnt.tobytes() == ccnt.tobytes(), (cnt, ccnt)
        assert r == np.inf or ((counts == 0).any() and (counts == 1).any())


@pytest.mark.parametrize("scene", ["cornell", "terrain2k", "spheres2k_f64"])
def test_short_rows_equal_radius_lists(dll, radius_dll, orc, scene):
    bounds, index, prims, leaf, raw, _ = golden_scene(scene, "parallel_high", orc)
    tree = Tree(bounds, index, prims, leaf)
    dt = tree.dtype
    pts, diag = scene_queries(raw, 1024, dt, 11, leaf == 1)
    q = _queries(pts, np.asarray(0.05 * diag, dtype=dt), dt)
    offsets, lst, _, rcounts, _ = host_radius(radius_dll, tree, q, threads=4)
    ids, _, counts, _ = host_knn(dll, tree, q, 8, threads=4)
    short = np.flatnonzero(rcounts < 8)
    print(f"{scene}: {len(short)} of {len(q)} queries have fewer than 8 primitives within the radius")
    assert len(short) >= 0.25 * len(q)
    for j in short:
        assert counts[j] == rcounts[j], (scene, j)
        assert sorted(ids[j, :counts[j]].tolist()) == sorted(lst[int(offsets[j]):int(offsets[j + 1])].tolist()), (scene, j)


def test_edge_queries(dll, radius_dll, orc):
    bounds, index, prims, leaf, raw, pids = golden_scene("cornell", "serial_low", orc)
    tree = Tree(bounds, index, prims, leaf)
    assert len(prims) == 36
    c = raw.reshape(-1, 3).mean(axis=0)
    on = raw.reshape(-1, 3)[5]                                   # a vertex: at distance exactly 0 of its triangles
    q = np.array([[c[0], c[1], c[2], np.inf], [np.nan, c[1], c[2], np.inf], [c[0], np.nan, c[2], 1.0], [c[0], c[1], c[2], -1.0],
                  [c[0], c[1], c[2], np.nan], [on[0], on[1], on[2], 0.0], [c[0], c[1], c[2], 1e30], [c[0], c[1], c[2], -np.inf]], dtype=np.float32)
    d2 = host_brute(radius_dll, tree, q)
    k = 5
    ids, dist, counts, _ = host_knn(dll, tree, q, k)
    for j in (1, 2, 3, 4, 7):                                   # invalid: empty, padded with their own max_distance bits
        assert counts[j] == 0 and (ids[j] == INVALID).all() and dist[j].tobytes() == np.repeat(q[j, 3], k).tobytes()
    zero = np.flatnonzero(d2[5] == 0)
    assert 1 <= len(zero) and counts[5] == min(len(zero), k)
    assert (ids[5, :counts[5]] == zero[:k]).all() and (dist[5, :counts[5]] == 0).all()            # radius 0: d2 == 0 only, ascending index
    assert (ids[5, counts[5]:] == INVALID).all() and (dist[5, counts[5]:] == 0).all()
    want = np.lexsort((np.arange(36), d2[0]))                  # ascending (d2, i)
    for j in (0, 6):                                            # +inf, and a radius whose square overflows
        assert counts[j] == k and (ids[j] == want[:k]).all() and (dist[j] == np.sqrt(d2[0, want[:k]])).all()
    # more slots than primitives: all 36, sorted, then 28 padded slots
    i64, d64, c64, _ = host_knn(dll, tree, q, 64)
    assert c64[0] == 36 and (i64[0, :36] == want).all() and (d64[0, :36] == np.sqrt(d2[0, want])).all()
    assert (i64[0, 36:] == INVALID).all() and np.isinf(d64[0, 36:]).all() and len(i64[0, 36:]) == 28
    # without the optional outputs: the same ids
    i2, d_none, c_none, _ = host_knn(dll, tree, q, k, dist=False, counts=False)
    assert d_none is None and c_none is None and i2.tobytes() == ids.tobytes()
    # original ids: the same rows, mapped through prim_ids, order and distances unchanged
    oi, od, oc, _ = host_knn(dll, tree, q, k, prim_ids=pids.astype(np.uint32))
    valid = ids != INVALID
    assert (oi[valid] == pids[ids[valid].astype(np.int64)]).all() and (oi[~valid] == INVALID).all()
    assert od.tobytes() == dist.tobytes() and (oc == counts).all()
    # reading the batch through a permuted order changes nothing
    pts, diag = scene_queries(raw, 200, np.float32, 9, False)
    q2 = _queries(pts, np.float32(0.2 * diag), np.float32)
    base = host_knn(dll, tree, q2, k)
    perm = np.random.default_rng(5).permutation(len(q2)).astype(np.uint32)
    again = host_knn(dll, tree, q2, k, order=perm)
    for x, y in zip(base, again):
        assert x.tobytes() == y.tobytes()
    assert dll.knn_host_walk(0, 0, _p(tree.pairs), tree.root, _p(tree.prims), _p(q), 0, 0, 64, None, None, 0, 1, None, None, None, _p(np.zeros(3, np.uint64))) == 1
    assert dll.knn_host_walk(0, 0, _p(tree.pairs), tree.root, _p(tree.prims), _p(q), 0, MAX_K + 1, 64, None, None, 0, 1, None, None, None, _p(np.zeros(3, np.uint64))) == 1


@pytest.mark.parametrize("depth", [65, 300])
def test_deep_chain(dll, orc, depth):
    tris, nodes, _ = chain_tree(depth, orc.prep_tris)
    tree = Tree(nodes["bounds"], nodes["index"], precompute(tris, np.float32), 0)
    q = chain_queries(depth, 300)                              # 300: not a multiple of the block
    ids, dist, counts, _ = host_knn(dll, tree, q, 5, deep_cap=depth - 63)
    assert (counts == 5).all() and (ids == np.arange(depth, depth - 5, -1, dtype=np.uint32)).all()
    assert (np.diff(dist, axis=1) > 0).all()


def test_deep_chain_fills_the_spill(dll, radius_dll, orc):
    """70 levels, one push per level: the stack crosses LDS -> scratch (entry 8), scratch -> HBM (entry 64) and ends on the last of
    the 6 HBM entries it is given; the rows are made of the entries popped from there."""
    depth = 70
    tris, nodes, _ = chain_tree(depth, orc.prep_tris)
    tree = Tree(nodes["bounds"], nodes["index"], precompute(tris, np.float32), 0)
    q = chain_queries(depth, 48)
    ids, dist, counts, _ = host_knn(dll, tree, q, 8, deep_cap=depth - 64)
    eids, ed2, _ = expected_rows(brute_order(host_brute(radius_dll, tree, q), np.float32(np.inf)), 8)
    assert (counts == 8).all() and (ids == eids).all() and (ids == np.arange(depth, depth - 8, -1)).all()
    assert (dist == np.sqrt(ed2)).all()


def test_stride_independence(dll, orc):
    bounds, index, prims, leaf, raw, _ = golden_scene("soup2k", "parallel_high", orc)
    tree = Tree(bounds, index, prims, leaf)
    pts, diag = scene_queries(raw, 300, np.float32, 7, False)
    q = _queries(pts, np.float32(0.1 * diag), np.float32)
    for k in (1, 16, 33):
        base = host_knn(dll, tree, q, k, stride=64)
        for stride in (128, 256):
            again = host_knn(dll, tree, q, k, stride=stride)
            for x, y in zip(base, again):
                assert x.tobytes() == y.tobytes()


def test_knn_symbols_are_declared_and_exported():
    from bvh_amd import _lib, build
    build.build()
    dll = _lib.load()
    header = open(os.path.join(ROOT, "include", "bvh_amd.h")).read()
    declared = set(re.findall(r"BVH_AMD_API[^;]*?\b(bvh\w+)\s*\(", header))
    want = {f"bvh{s}_knn_{leaf}" for s in ("3f", "3d") for leaf in ("tri", "sphere")}
    assert {n for n in declared if "knn" in n} == want
    assert re.search(r"#define\s+BVH_AMD_KNN_MAX_K\s+64\b", header)
    assert want <= set(_lib.exported_symbols())
    for name in sorted(want):
        assert hasattr(dll, name), name
        assert "radius" not in name and "offsets_from_counts" not in name
    for s in ("2f", "2d"):
        for leaf in ("tri", "sphere"):
            assert not hasattr(dll, f"bvh{s}_knn_{leaf}")
            assert f"bvh{s}_knn_{leaf}" not in _lib.exported_symbols()
