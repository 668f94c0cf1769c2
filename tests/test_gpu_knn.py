"""MI355X: batched k-nearest queries (bvhXX_knn_*, bvh_amd.knn). The device's rows, distances, counts and counters are byte-equal to
the host harness's (the same text compiled by g++, tests/test_knn_host.py) on both sides of every block-size boundary; the rows agree
with a float64 brute force over the original primitives; a row does not depend on batch order, size or the reordering flags; trees
deeper than 64 levels; k = 1 against closest_points; guard zones, flags, errors and the C++ mirror."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from test_closest_point_host import chain_queries, chain_tree, golden_scene, precompute, scene_queries
from test_gpu_closest_point import _dist_f64
from test_knn_host import compile_harness, host_knn
from test_radius_search_host import GUARD, INVALID, SENT_DIST, SENT_PRIM, Tree

pytestmark = pytest.mark.gpu


def block_lanes(k, scalar_bytes):
    """knn.hip's knn_block_lanes: of 256 / 128 / 64 lanes, the block that keeps the most lanes resident in a CU's 160 KB of LDS at
    (k + 8) * (scalar + 4) bytes per lane, within 64 KB per block and 2048 lanes per CU; ties to the larger."""
    best, best_resident = 64, 0
    for lanes in (256, 128, 64):
        size = (k + 8) * lanes * (scalar_bytes + 4)
        if size <= 64 << 10 and min((160 << 10) // size * lanes, 2048) > best_resident:
            best, best_resident = lanes, min((160 << 10) // size * lanes, 2048)
    return best


# The issue's k, and k = 5, 7, 9: every block size for either scalar type, and both neighbours of the sizes' boundaries at 8 / 9, 16 / 17
# and 32 / 33.
KS = (1, 5, 7, 8, 9, 16, 17, 32, 33, 64)
assert [block_lanes(k, 4) for k in KS] == [256, 256, 64, 256, 128, 64, 256, 128, 64, 64]
assert [block_lanes(k, 8) for k in KS] == [64, 256, 128, 64, 256, 128, 128, 64, 64, 64]


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return compile_harness(tmp_path_factory.mktemp("knn_gpu"))


def _queries(pts, r, dt):
    q = np.zeros((len(pts), 4), dtype=dt)
    q[:, :3] = pts
    q[:, 3] = r
    return q


def _np(t, dtype=None):
    a = t.detach().cpu().numpy()
    return a if dtype is None else a.view(dtype)


def device_knn(bvh, dprims, q, leaf, k, **kw):
    """bvh_amd.knn -> numpy (ids uint32 (n, k), dist (n, k), counts uint32, counters uint64)."""
    import bvh_amd
    ids, dist, counts, cnt = bvh_amd.knn(bvh, dprims, q, k, leaf="sphere" if leaf else "tri", counters=True, **kw)
    assert ids.shape == (len(q), k) and dist.shape == (len(q), k) and counts.shape == (len(q),)
    return _np(ids, np.uint32), _np(dist), _np(counts, np.uint32), _np(cnt).astype(np.uint64)


def _device_vs_host(dll, bvh, dprims, q, leaf, k, deep_cap=0):
    nodes = bvh.nodes
    tree = Tree(nodes["bounds"], nodes["index"], _np(dprims) if not isinstance(dprims, np.ndarray) else dprims, leaf)
    h_ids, h_dist, h_counts, h_cnt = host_knn(dll, tree, q, k, threads=8, deep_cap=deep_cap)
    ids, dist, counts, cnt = device_knn(bvh, dprims, q, leaf, k)
    assert ids.tobytes() == h_ids.tobytes(), k
    assert dist.tobytes() == h_dist.tobytes(), k
    assert counts.tobytes() == h_counts.tobytes(), k
    assert (cnt == h_cnt).all(), (k, cnt, h_cnt)
    return h_ids, h_dist, h_counts


@pytest.mark.parametrize("scene", ["cornell", "soup2k", "terrain2k", "soup2k_f64", "spheres2k_f64"])
def test_device_equals_host_golden(dll, orc, scene):
    import bvh_amd
    import torch
    g = load_golden(scene)
    double = g["prims"].dtype == np.float64
    bvh = bvh_amd.Bvh.deserialize(g["bvh_parallel_high"].tobytes(), dtype=np.float64 if double else np.float32)
    _, _, prims, leaf, raw, _ = golden_scene(scene, "parallel_high", orc)
    dprims = torch.from_numpy(prims).cuda()
    pts, diag = scene_queries(raw, 2048 if leaf == 1 else 1024, prims.dtype, 3, leaf == 1)      # 2048 queries either way
    assert len(pts) == 2048
    for r in (0.05 * diag, np.inf):
        q = _queries(pts, r, prims.dtype)
        for k in KS:
            _, _, counts = _device_vs_host(dll, bvh, dprims, q, leaf, k)
            assert counts.max() > 0 and (r != np.inf or (counts == min(k, len(prims))).all())


def test_device_equals_host_float_spheres(dll):
    import bvh_amd
    from bvh_amd import synth
    sph = synth.spheres(20000, dtype=np.float32)
    bb, cc = bvh_amd.sphere_bounds(sph)
    bvh = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.Medium))
    dprims = bvh_amd.gather(sph, bvh.device_prim_ids())
    pts, diag = scene_queries(sph, 4096, np.float32, 4, True)
    for k in (9, 17, 64):                                      # 128, 256 and 64 lanes per block
        _, _, counts = _device_vs_host(dll, bvh, dprims, _queries(pts, 0.05 * diag, np.float32), 1, k)
        assert counts.max() > 0


# ---- against a float64 brute force on the GPU -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["soup100k", "spheres100k"])
def test_against_f64_brute_force(name):
    import bvh_amd
    import torch
    from bvh_amd import synth
    raw = synth.soup(100_000) if name == "soup100k" else synth.spheres(100_000)      # (the spheres in the generator's native float64)
    sphere = raw.shape[1] == 4
    dt = raw.dtype
    assert dt == (np.float64 if sphere else np.float32)
    bb, cc = bvh_amd.sphere_bounds(raw) if sphere else bvh_amd.tri_bounds(raw)
    bvh = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.High))
    dprims = bvh_amd.gather(raw, bvh.device_prim_ids()) if sphere else bvh_amd.precompute_tris(raw, bvh.device_prim_ids())
    lo, hi = synth.scene_bounds(raw)
    n, k = 2048, 16
    pts = np.concatenate([synth.points_uniform(n, lo, hi, seed=21, dtype=np.float64),
                          synth.points_near_surface(raw.astype(np.float64), n, seed=22, sigma=0.01 * float(np.max(hi - lo))) if not sphere
                          else synth.points_uniform(n, lo, hi, seed=25, scale=0.5, dtype=np.float64)]).astype(dt)
    # The tolerance of tests/test_gpu_radius_search.py::test_against_f64_brute_force, by its derivation: 16 ulps of the largest coordinate.
    M = float(max(np.abs(raw).max(), np.abs(pts).max()))
    tol = 16 * np.finfo(dt).eps * M
    ids, dist, counts = bvh_amd.knn(bvh, dprims, pts, k, leaf="sphere" if sphere else "tri", original_ids=True)
    assert bool((counts == k).all())
    cols = ids.long()
    assert int(cols.min()) >= 0 and int(cols.max()) < len(raw)
    assert bool((cols.sort(dim=1).values.diff(dim=1) > 0).all())                 # k different primitives
    assert bool((dist.diff(dim=1) >= 0).all())
    P = torch.from_numpy(np.ascontiguousarray(raw, dtype=np.float64)).cuda()
    Q = torch.from_numpy(np.ascontiguousarray(pts[:, :3], dtype=np.float64)).cuda()
    chunk = max(1, (1 << 22) // len(raw))
    worst_kth = worst_listed = 0.0
    for s in range(0, len(pts), chunk):
        e = min(s + chunk, len(pts))
        d64 = _dist_f64(torch, Q[s:e, None, :], P[None], sphere)
        kth = d64.kthvalue(k, dim=1).values
        listed = torch.gather(d64, 1, cols[s:e])
        worst_kth = max(worst_kth, float((dist[s:e, k - 1].double() - kth).abs().max()))
        worst_listed = max(worst_listed, float((listed - kth[:, None]).max()))
        assert bool(((dist[s:e, k - 1].double() - kth).abs() <= tol).all()), (name, s)
        assert bool((listed <= kth[:, None] + tol).all()), (name, s)
        assert bool(((dist[s:e].double() - listed).abs() <= tol).all()), (name, s)
    print(f"{name}: k-th distance off the float64 k-th by at most {worst_kth:.3g}, a listed primitive beyond it by at most {worst_listed:.3g} (tol {tol:.3g})")


# ---- order and flag invariance ------------------------------------------------------------------------------------------------

def test_order_and_flag_invariance():
    import bvh_amd
    import torch
    from bvh_amd import synth
    tris = synth.soup(100_000)
    bb, cc = bvh_amd.tri_bounds(tris)
    bvh = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.Medium))
    dprims = bvh_amd.precompute_tris(tris, bvh.device_prim_ids())
    lo, hi = synth.scene_bounds(tris)
    diag = float(np.linalg.norm(hi - lo))
    pts = np.concatenate([synth.points_uniform(2500, lo, hi, seed=31), synth.points_near_surface(tris, 2500, seed=32, sigma=0.01)])
    q = _queries(pts, 0.02 * diag, np.float32)
    q[::7, 3] = 0.06 * diag
    q[::11, 3] = 0.0
    q[::500, 3] = np.inf
    q[13, 3] = -1.0
    q[17, 0] = np.nan
    k = 8
    base = device_knn(bvh, dprims, q, 0, k, sort_queries=False)
    assert base[2][13] == 0 and base[2][17] == 0 and (base[0][13] == INVALID).all() and (base[1][13] == -1.0).all() and np.isnan(q[17, 0])
    assert (base[2][::500] == k).all() and 0 < (base[2] < k).sum() < len(q)
    for sort in (True, None):
        again = device_knn(bvh, dprims, q, 0, k, sort_queries=sort)
        for x, y in zip(base[:3], again[:3]):
            assert x.tobytes() == y.tobytes()
    perm = np.random.default_rng(3).permutation(len(q))
    p_ids, p_dist, p_counts, _ = device_knn(bvh, dprims, torch.from_numpy(q[perm]).cuda(), 0, k, sort_queries=True)
    assert p_ids.tobytes() == base[0][perm].tobytes() and p_dist.tobytes() == base[1][perm].tobytes() and (p_counts == base[2][perm]).all()
    s_ids, s_dist, s_counts, _ = device_knn(bvh, dprims, q[1000:1100], 0, k)       # batch size and position do not matter either
    assert s_ids.tobytes() == base[0][1000:1100].tobytes() and s_dist.tobytes() == base[1][1000:1100].tobytes()
    assert (s_counts == base[2][1000:1100]).all()


@pytest.mark.parametrize("depth", [65, 300, 3000])
def test_trees_deeper_than_64_levels(dll, restatement, depth):
    import bvh_amd
    tris, nodes, ids = chain_tree(depth, restatement.prep_tris)
    bvh = bvh_amd.Bvh.from_nodes(nodes, ids)
    prims = precompute(tris, np.float32)
    q = chain_queries(depth, 4096)
    h_ids, h_dist, h_counts = _device_vs_host(dll, bvh, prims, q, 0, 5, deep_cap=depth - 63)
    assert (h_counts == 5).all() and (h_ids == np.arange(depth, depth - 5, -1, dtype=np.uint32)).all()
    assert (np.diff(h_dist, axis=1) > 0).all()


@pytest.mark.parametrize("scene", ["terrain2k", "spheres2k_f64"])
def test_k1_equals_closest_points(orc, scene):
    import bvh_amd
    import torch
    g = load_golden(scene)
    double = g["prims"].dtype == np.float64
    bvh = bvh_amd.Bvh.deserialize(g["bvh_parallel_high"].tobytes(), dtype=np.float64 if double else np.float32)
    _, _, prims, leaf, raw, _ = golden_scene(scene, "parallel_high", orc)
    dprims = torch.from_numpy(prims).cuda()
    pts, diag = scene_queries(raw, 2048 if leaf == 1 else 1024, prims.dtype, 3, leaf == 1)
    name = "sphere" if leaf else "tri"
    for r in (0.05 * diag, np.inf):
        q = _queries(pts, r, prims.dtype)
        hits, ccnt = bvh_amd.closest_points(bvh, dprims, q, leaf=name, counters=True)
        hits = bvh_amd.hits_to_numpy(hits)
        ids, dist, counts, cnt = device_knn(bvh, dprims, q, leaf, 1)
        assert ids[:, 0].tobytes() == np.ascontiguousarray(hits["prim"]).tobytes()
        assert dist[:, 0].tobytes() == np.ascontiguousarray(hits["t"]).tobytes()
        assert (counts == (hits["prim"] != INVALID)).all()
        assert (cnt == _np(ccnt).astype(np.uint64)).all()


# ---- guard zones, the C entry point ---------------------------------------------------------------------------------------------

def test_guard_zones_and_optional_outputs(orc):
    import bvh_amd
    import torch
    from bvh_amd import _lib
    g = load_golden("soup2k")
    bvh = bvh_amd.Bvh.deserialize(g["bvh_parallel_high"].tobytes())
    _, _, prims, _, raw, _ = golden_scene("soup2k", "parallel_high", orc)
    pts, diag = scene_queries(raw, 1500, np.float32, 5, False)
    q = _queries(pts, np.float32(0.1 * diag), np.float32)
    n = len(q)                                                 # 3000: not a multiple of any block size
    dq, dp = torch.from_numpy(q).cuda(), torch.from_numpy(prims).cuda()
    f = _lib.load().bvh3f_knn_tri
    sent = torch.from_numpy(np.array([SENT_PRIM], dtype=np.uint32).view(np.int32)).cuda()
    for k in (5, 9, 33):                                       # 256, 128 and 64 lanes per block
        ids, dist, counts, _ = device_knn(bvh, dp, dq, 0, k)
        assert (counts < k).any() and (counts == k).any()
        lp = torch.empty(n * k + 2 * GUARD, dtype=torch.int32, device="cuda")
        ld = torch.empty(n * k + 2 * GUARD, dtype=torch.float32, device="cuda")
        dc = torch.empty(n + 2 * GUARD, dtype=torch.int32, device="cuda")
        for flags, with_dist, with_counts in ((0, True, True), (4, False, True), (16, True, False), (0, False, False)):
            lp[:] = sent
            ld[:] = SENT_DIST
            dc[:] = sent
            assert f(bvh._h, dp.data_ptr(), dq.data_ptr(), n, k, flags, lp.data_ptr() + 4 * GUARD, ld.data_ptr() + 4 * GUARD if with_dist else None,
                     dc.data_ptr() + 4 * GUARD if with_counts else None, None, None) == 0, _lib.last_error()
            hp, hd, hc = _np(lp, np.uint32), _np(ld), _np(dc, np.uint32)
            assert (hp[:GUARD] == SENT_PRIM).all() and (hp[GUARD + n * k:] == SENT_PRIM).all()
            assert hp[GUARD:GUARD + n * k].tobytes() == ids.tobytes()                       # the optional outputs do not change the ids
            if with_dist:
                assert (hd[:GUARD] == SENT_DIST).all() and (hd[GUARD + n * k:] == SENT_DIST).all()
                assert hd[GUARD:GUARD + n * k].tobytes() == dist.tobytes()
            else:
                assert (hd == SENT_DIST).all()
            if with_counts:
                assert (hc[:GUARD] == SENT_PRIM).all() and (hc[GUARD + n:] == SENT_PRIM).all() and (hc[GUARD:GUARD + n] == counts).all()
            else:
                assert (hc == SENT_PRIM).all()


# ---- flags and errors ---------------------------------------------------------------------------------------------------------------

def test_flags_and_errors(orc):
    import bvh_amd
    import torch
    from bvh_amd import _lib
    g = load_golden("soup2k")
    bvh = bvh_amd.Bvh.deserialize(g["bvh_serial_low"].tobytes())
    _, _, prims, _, raw, pids = golden_scene("soup2k", "serial_low", orc)
    pts = np.random.default_rng(1).random((500, 3)).astype(np.float32)
    ids, dist, counts = bvh_amd.knn(bvh, prims, pts, 4, max_distance=0.1)
    oi, od, oc = bvh_amd.knn(bvh, prims, pts, 4, max_distance=0.1, original_ids=True)
    assert ids.dtype == torch.int32 and dist.dtype == torch.float32 and counts.dtype == torch.int32
    assert ids.shape == (500, 4) and dist.shape == (500, 4) and counts.shape == (500,)
    valid = _np(ids) >= 0
    assert valid.any() and (~valid).any() and (valid.sum(axis=1) == _np(counts)).all()
    assert (_np(oi)[valid] == pids[_np(ids)[valid]]).all() and (_np(oi)[~valid] == -1).all()
    assert _np(od).tobytes() == _np(dist).tobytes() and (_np(oc) == _np(counts)).all()
    assert (_np(dist)[~valid] == np.float32(0.1)).all()
    assert bvh_amd.knn(bvh, prims, pts, 4, max_distance=0.1, distances=False)[1] is None
    q4 = _queries(pts, 0.1, np.float32)
    i4, d4, c4 = bvh_amd.knn(bvh, prims, q4, 4)
    assert _np(i4).tobytes() == _np(ids).tobytes() and _np(d4).tobytes() == _np(dist).tobytes() and (_np(c4) == _np(counts)).all()
    with pytest.raises(ValueError):
        bvh_amd.knn(bvh, prims, q4, 4, max_distance=1.0)
    for bad_k in (0, 65):
        with pytest.raises(ValueError):
            bvh_amd.knn(bvh, prims, pts, bad_k)
    with pytest.raises(ValueError):
        bvh_amd.knn(bvh, prims, pts, 4, leaf="box")
    with pytest.raises(ValueError):
        bvh_amd.knn(bvh, prims, np.zeros((4, 2), np.float32), 4)
    e_ids, e_dist, e_counts = bvh_amd.knn(bvh, prims, np.zeros((0, 3), np.float32), 4)
    assert e_ids.shape == (0, 4) and e_dist.shape == (0, 4) and e_counts.shape == (0,)
    z_ids, z_dist, z_counts = bvh_amd.knn(bvh, prims, pts + 100, 4, max_distance=0.1)          # nothing within reach: padded rows
    assert (_np(z_ids) == -1).all() and (_np(z_dist) == np.float32(0.1)).all() and (_np(z_counts) == 0).all()

    lib = _lib.load()
    dp, dq = torch.from_numpy(prims).cuda(), torch.from_numpy(q4).cuda()
    n, k = len(q4), 4
    op = torch.zeros(n * k + 4, dtype=torch.int32, device="cuda")
    od = torch.zeros(n * k + 4, dtype=torch.float32, device="cuda")
    oc = torch.zeros(n + 4, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    f = lib.bvh3f_knn_tri
    P = lambda t: t.data_ptr()
    assert f(bvh._h, P(dp), P(dq), n, k, 0, P(op), P(od), P(oc), P(cnt), None) == 0
    assert f(bvh._h, P(dp), P(dq), 0, k, 0, None, None, None, None, None) == 0                   # n == 0: no-op
    for flags in (4, 8, 16, 4 | 8):
        assert f(bvh._h, P(dp), P(dq), n, k, flags, P(op), P(od), P(oc), None, None) == 0, _lib.last_error()
    for bad in (1, 2, 32, 1 << 20):                                                              # ANY_HIT, ROBUST, unknown bits
        assert f(bvh._h, P(dp), P(dq), n, k, bad, P(op), None, None, None, None) == -2
        assert "flags" in _lib.last_error()
    for bad_k in (0, 65, 1 << 20):
        assert f(bvh._h, P(dp), P(dq), n, bad_k, 0, P(op), None, None, None, None) == -2
        assert "k must" in _lib.last_error()
    assert f(bvh._h, None, P(dq), n, k, 0, P(op), None, None, None, None) == -2
    assert "null" in _lib.last_error()
    assert f(bvh._h, P(dp), None, n, k, 0, P(op), None, None, None, None) == -2
    assert f(bvh._h, P(dp), P(dq), n, k, 0, None, P(od), P(oc), None, None) == -2                # d_out_prims is required
    assert "null" in _lib.last_error()
    assert f(None, P(dp), P(dq), n, k, 0, P(op), None, None, None, None) == -2
    assert "null" in _lib.last_error()
    for args in ((P(dp), P(dq) + 4, n - 1, k, 0, P(op), None, None, None, None),                  # misaligned queries, prims, rows,
                 (P(dp) + 8, P(dq), n, k, 0, P(op), None, None, None, None),                      # distances, counts, counters
                 (P(dp), P(dq), n, k, 0, P(op) + 2, None, None, None, None),
                 (P(dp), P(dq), n, k, 0, P(op), P(od) + 2, None, None, None),
                 (P(dp), P(dq), n, k, 0, P(op), None, P(oc) + 2, None, None),
                 (P(dp), P(dq), n, k, 0, P(op), None, None, P(cnt) + 4, None)):
        assert f(bvh._h, *args) == -2
        assert "aligned" in _lib.last_error()
    assert f(bvh._h, P(dp), P(dq), n, k, 0, P(op) + 4, P(od) + 4, P(oc) + 4, None, None) == 0      # 4-byte alignment is enough for the outputs
    # doubles: d_out_dist needs 8 bytes
    gd = load_golden("soup2k_f64")
    bvhd = bvh_amd.Bvh.deserialize(gd["bvh_serial_low"].tobytes(), dtype=np.float64)
    _, _, primsd, _, _, _ = golden_scene("soup2k_f64", "serial_low", orc)
    dpd, dqd = torch.from_numpy(primsd).cuda(), torch.from_numpy(q4.astype(np.float64)).cuda()
    odd = torch.zeros(n * k + 4, dtype=torch.float64, device="cuda")
    fd = lib.bvh3d_knn_tri
    assert fd(bvhd._h, P(dpd), P(dqd), n, k, 0, P(op), P(odd), None, None, None) == 0
    assert fd(bvhd._h, P(dpd), P(dqd), n, k, 0, P(op), P(odd) + 4, None, None, None) == -2
    assert "aligned" in _lib.last_error()
    # a 2D tree, dtype mismatches
    g2 = load_golden("circles2k_2f")
    bb, cc = bvh_amd.sphere_bounds(g2["prims"])
    bvh2 = bvh_amd.DefaultBuilder.build(bb, cc)
    with pytest.raises(TypeError):
        bvh_amd.knn(bvh2, g2["prims"], np.zeros((4, 3), np.float32), 4, leaf="sphere")
    with pytest.raises(TypeError):
        bvh_amd.knn(bvh, prims, np.zeros((4, 3), np.float64), 4)
    with pytest.raises(TypeError):
        bvh_amd.knn(bvh, prims.astype(np.float64), np.zeros((4, 3), np.float32), 4)


def test_cpp_mirror_agrees(tmp_path):
    """tests/cpp/knn_amd.cpp (amd::knn_batch over the mirror, g++ -Wall -Wextra -Werror) gives the rows, distances and counts
    bvh_amd.knn gives on the same tree."""
    import bvh_amd
    from bvh_amd import build
    build.build()
    lib = os.path.join(ROOT, "bvh_amd", "lib")
    exe = str(tmp_path / "knn_amd")
    cmd = ["g++", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "knn_amd.cpp"),
           "-L", lib, "-lbvh_amd", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    prim_ids = [int(x) for x in lines[0].split()[1:]]
    cpp_counts = np.array([int(x) for x in lines[1].split()[1:]], dtype=np.int64)
    side, k = 12, 6                                           # the program's mesh, rebuilt here
    h = lambda i, j: np.float32(0.1 * np.sin(0.7 * i) * np.cos(0.4 * j))
    tris, queries = [], []
    for i in range(side):
        for j in range(side):
            a, b = [i, h(i, j), j], [i + 1, h(i + 1, j), j]
            c, d = [i + 1, h(i + 1, j + 1), j + 1], [i, h(i, j + 1), j + 1]
            tris += [a + b + c, a + c + d]
    radii = [np.float32(0.25), np.float32(1.5), np.inf]
    for m in range(200):
        queries.append([np.float32(-1.5 + 15.0 * ((m * 37) % 200) / 200.0), np.float32(-1.0 + 2.0 * ((m * 53) % 200) / 200.0),
                        np.float32(-1.5 + 15.0 * ((m * 91) % 200) / 200.0), radii[2] if m % 50 == 49 else radii[m % 2]])
    tris = np.array(tris, dtype=np.float32)
    bb, cc = bvh_amd.tri_bounds(tris)
    bvh = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.High))
    assert list(bvh.prim_ids) == prim_ids
    ids, dist, counts = bvh_amd.knn(bvh, bvh_amd.precompute_tris(tris, bvh.device_prim_ids()), np.array(queries, np.float32), k)
    ids, dist, counts = _np(ids, np.uint32), _np(dist), _np(counts)
    assert (cpp_counts == counts).all() and (counts == k).any() and (counts < k).any() and len(lines) == 2 + 200 * k
    for e, line in enumerate(lines[2:]):
        qk, s, p, t = line.split()
        assert int(qk) == e // k and int(s) == e % k and int(p) == ids[e // k, e % k], (line, e)
        assert np.float32(float.fromhex(t)).tobytes() == dist[e // k, e % k].tobytes(), (line, e)
