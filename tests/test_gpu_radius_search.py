"""MI355X: batched radius queries (bvhXX_radius_search_*, bvh_amd.radius_count / radius_search). The device's counts, lists,
distances and counters are byte-equal to the host harness's (the same text compiled by g++, tests/test_radius_search_host.py); the
listed sets agree with a float64 brute force over the original primitives; per-query results do not depend on batch order, size or
the reordering flags; trees deeper than 64 levels; fixed segments, guard zones and the offsets scan; flags, errors and the C++ mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from test_closest_point_host import chain_queries, chain_tree, golden_scene, precompute, scene_queries
from test_gpu_closest_point import _dist_f64
from test_radius_search_host import GUARD, INVALID, SENT_DIST, SENT_PRIM, Tree, compile_harness, host_radius, host_walk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return compile_harness(tmp_path_factory.mktemp("radius_gpu"))


def _queries(pts, r, dt):
    q = np.zeros((len(pts), 4), dtype=dt)
    q[:, :3] = pts
    q[:, 3] = r
    return q


def _np(t, dtype=None):
    a = t.detach().cpu().numpy()
    return a if dtype is None else a.view(dtype)


def device_lists(bvh, dprims, q, leaf, **kw):
    """bvh_amd.radius_search with exact lists -> numpy (offsets uint64, ids uint32, dist, counters uint64)."""
    import bvh_amd
    offsets, ids, dist, cnt = bvh_amd.radius_search(bvh, dprims, q, leaf="sphere" if leaf else "tri", counters=True, **kw)
    return _np(offsets, np.uint64), _np(ids, np.uint32), _np(dist), _np(cnt).astype(np.uint64)


def _device_vs_host(dll, bvh, dprims, q, leaf, deep_cap=0):
    import bvh_amd
    nodes = bvh.nodes
    tree = Tree(nodes["bounds"], nodes["index"], _np(dprims) if not isinstance(dprims, np.ndarray) else dprims, leaf)
    h_off, h_ids, h_dist, h_counts, h_cnt = host_radius(dll, tree, q, threads=8, deep_cap=deep_cap)
    counts, ccnt = bvh_amd.radius_count(bvh, dprims, q, leaf="sphere" if leaf else "tri", counters=True)
    assert _np(counts, np.uint32).tobytes() == h_counts.tobytes()
    assert (_np(ccnt).astype(np.uint64) == h_cnt).all(), (ccnt, h_cnt)
    off, ids, dist, cnt = device_lists(bvh, dprims, q, leaf)
    assert off.tobytes() == h_off.tobytes()
    assert ids.tobytes() == h_ids.tobytes()
    assert dist.tobytes() == h_dist.tobytes()
    assert (cnt == h_cnt).all(), (cnt, h_cnt)
    return h_off, h_ids, h_dist


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
        off, _, _ = _device_vs_host(dll, bvh, dprims, _queries(pts, r, prims.dtype), leaf)
        assert off[-1] > 0 and (r != np.inf or off[-1] == 2048 * len(prims))


def test_device_equals_host_float_spheres(dll):
    import bvh_amd
    from bvh_amd import synth
    sph = synth.spheres(20000, dtype=np.float32)
    bb, cc = bvh_amd.sphere_bounds(sph)
    bvh = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.Medium))
    dprims = bvh_amd.gather(sph, bvh.device_prim_ids())
    pts, diag = scene_queries(sph, 4096, np.float32, 4, True)
    off, _, _ = _device_vs_host(dll, bvh, dprims, _queries(pts, 0.05 * diag, np.float32), 1)
    assert off[-1] > 0


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
    n = 2048
    pts = np.concatenate([synth.points_uniform(n, lo, hi, seed=21, dtype=np.float64),
                          synth.points_near_surface(raw.astype(np.float64), n, seed=22, sigma=0.01 * float(np.max(hi - lo))) if not sphere
                          else synth.points_uniform(n, lo, hi, seed=25, scale=0.5, dtype=np.float64)]).astype(dt)
    diag = float(np.linalg.norm(hi - lo))
    r = float(np.asarray(0.02 * diag, dtype=dt))
    # The tolerance of tests/test_gpu_closest_point.py::test_against_f64_brute_force, by its derivation: the kernel forms q - p0 and the
    # edge dot products in the scalar type; with coordinates of magnitude M each rounding is at most ulp(M) / 2 and the distance collects a
    # handful of them, so 16 ulps of M.
    M = float(max(np.abs(raw).max(), np.abs(pts).max()))
    tol = 16 * np.finfo(dt).eps * M
    offsets, ids, dist = bvh_amd.radius_search(bvh, dprims, pts, radius=r, leaf="sphere" if sphere else "tri", original_ids=True)
    counts = (offsets[1:] - offsets[:-1])
    rows = torch.repeat_interleave(torch.arange(len(pts), device="cuda"), counts)
    cols = ids.long()
    assert int(cols.min()) >= 0 and int(cols.max()) < len(raw)
    P = torch.from_numpy(np.ascontiguousarray(raw, dtype=np.float64)).cuda()
    Q = torch.from_numpy(np.ascontiguousarray(pts[:, :3], dtype=np.float64)).cuda()
    chunk = max(1, (1 << 22) // len(raw))
    inside_total = unclear_total = 0
    for s in range(0, len(pts), chunk):
        e = min(s + chunk, len(pts))
        d64 = _dist_f64(torch, Q[s:e, None, :], P[None], sphere)
        inside, unclear = d64 <= r, (d64 - r).abs() <= tol
        a, b = int(offsets[s]), int(offsets[e])
        got = torch.zeros_like(inside)
        got[rows[a:b] - s, cols[a:b]] = True
        assert bool(((got == inside) | unclear).all()), (name, s)
        assert bool(((dist[a:b].double() - d64[rows[a:b] - s, cols[a:b]]).abs() <= tol).all()), (name, s)
        inside_total += int(inside.sum())
        unclear_total += int(unclear.sum())
    print(f"{name}: {inside_total} pairs within r = {r:.4g} (mean list {inside_total / len(pts):.2f}), {unclear_total} within tol of the boundary")
    assert inside_total > 0 and int(offsets[-1]) >= inside_total - unclear_total


# ---- order and flag invariance ------------------------------------------------------------------------------------------------

def _split(offsets, ids, dist):
    cut = offsets[1:-1].astype(np.int64)
    return np.split(ids, cut), np.split(dist, cut)


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
    base = device_lists(bvh, dprims, q, 0, sort_queries=False)
    assert base[0][-1] > 10 * 100_000
    for sort in (True, None):
        again = device_lists(bvh, dprims, q, 0, sort_queries=sort)
        for x, y in zip(base[:3], again[:3]):
            assert x.tobytes() == y.tobytes()
    lists, dists = _split(*base[:3])
    perm = np.random.default_rng(3).permutation(len(q))
    p_off, p_ids, p_dist, _ = device_lists(bvh, dprims, torch.from_numpy(q[perm]).cuda(), 0, sort_queries=True)
    assert (np.diff(p_off.astype(np.int64)) == np.diff(base[0].astype(np.int64))[perm]).all()
    assert p_ids.tobytes() == np.concatenate([lists[j] for j in perm]).tobytes()
    assert p_dist.tobytes() == np.concatenate([dists[j] for j in perm]).tobytes()
    s_off, s_ids, s_dist, _ = device_lists(bvh, dprims, q[1000:1100], 0)       # batch size and position do not matter either
    assert s_ids.tobytes() == np.concatenate(lists[1000:1100]).tobytes() and s_dist.tobytes() == np.concatenate(dists[1000:1100]).tobytes()
    assert (np.diff(s_off.astype(np.int64)) == np.diff(base[0].astype(np.int64))[1000:1100]).all()
    c = _np(bvh_amd.radius_count(bvh, dprims, q, sort_queries=True), np.uint32)
    assert (c == np.diff(base[0].astype(np.int64))).all()


@pytest.mark.parametrize("depth", [65, 300, 3000])
def test_trees_deeper_than_64_levels(dll, restatement, depth):
    import bvh_amd
    tris, nodes, ids = chain_tree(depth, restatement.prep_tris)
    bvh = bvh_amd.Bvh.from_nodes(nodes, ids)
    prims = precompute(tris, np.float32)
    q = chain_queries(depth, 4096)
    q[:, 3] = np.float32(4000 - depth + 10.5) - q[:, 0]        # reaches the ~10 triangles at the far end of the chain only
    q[::16, 3] = np.inf                                         # everything: depth + 1 primitives in DFS order
    off, h_ids, _ = _device_vs_host(dll, bvh, prims, q, 0, deep_cap=depth - 64 + 1)
    assert (np.diff(off.astype(np.int64))[::16] == depth + 1).all()
    assert (h_ids[:depth + 1] == np.arange(depth + 1)).all()
    assert 0 < np.diff(off.astype(np.int64))[1] < 20


# ---- segments, guard zones, the offsets scan -------------------------------------------------------------------------------------

def test_fixed_segments_and_guard_zones(orc):
    import bvh_amd
    import torch
    from bvh_amd import _lib
    g = load_golden("soup2k")
    bvh = bvh_amd.Bvh.deserialize(g["bvh_parallel_high"].tobytes())
    _, _, prims, _, raw, _ = golden_scene("soup2k", "parallel_high", orc)
    pts, diag = scene_queries(raw, 1500, np.float32, 5, False)
    q = _queries(pts, np.float32(0.1 * diag), np.float32)
    n = len(q)
    dq, dp = torch.from_numpy(q).cuda(), torch.from_numpy(prims).cuda()
    off, ids, dist, _ = device_lists(bvh, dp, dq, 0)
    exact = np.diff(off.astype(np.int64))
    assert exact.max() > 4 and (exact == 0).any()
    k = 4
    f_off, f_ids, f_dist, f_counts = bvh_amd.radius_search(bvh, dp, dq, max_per_query=k)
    assert (_np(f_off) == k * np.arange(n + 1)).all() and (_np(f_counts) == exact).all()           # counts are not truncated
    f_ids, f_dist = _np(f_ids).reshape(n, k), _np(f_dist).reshape(n, k)
    for i in range(n):
        m = min(int(exact[i]), k)
        assert (f_ids[i, :m].view(np.uint32) == ids[int(off[i]):int(off[i]) + m]).all() and (f_dist[i, :m] == dist[int(off[i]):int(off[i]) + m]).all()
        assert (f_ids[i, m:] == -1).all() and (f_dist[i, m:] == q[i, 3]).all()
    # the C entry point on sentinel-filled buffers: segments start at a non-zero offset; nothing before offsets[0], after offsets[n]
    # or in the guard zones is written
    base, tail = 7, 5
    total = base + k * n + tail
    fixed = torch.from_numpy((base + k * np.arange(n + 1)).astype(np.int64)).cuda()
    lp = torch.from_numpy(np.full(total + 2 * GUARD, SENT_PRIM, dtype=np.uint32).view(np.int32)).cuda()
    ld = torch.full((total + 2 * GUARD,), SENT_DIST, dtype=torch.float32, device="cuda")
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    f = _lib.load().bvh3f_radius_search_tri
    for flags in (0, 4, 16):
        lp[:] = torch.from_numpy(np.array([SENT_PRIM], dtype=np.uint32).view(np.int32)).cuda()
        ld[:] = SENT_DIST
        assert f(bvh._h, dp.data_ptr(), dq.data_ptr(), n, flags, counts.data_ptr(), fixed.data_ptr(), lp.data_ptr() + 4 * GUARD, ld.data_ptr() + 4 * GUARD,
                 None, None) == 0, _lib.last_error()
        hp, hd = _np(lp, np.uint32), _np(ld)
        inner = slice(GUARD + base, GUARD + base + k * n)
        assert (hp[:GUARD + base] == SENT_PRIM).all() and (hp[GUARD + base + k * n:] == SENT_PRIM).all()
        assert (hd[:GUARD + base] == SENT_DIST).all() and (hd[GUARD + base + k * n:] == SENT_DIST).all()
        assert hp[inner].tobytes() == f_ids.view(np.uint32).tobytes() and hd[inner].tobytes() == f_dist.tobytes()
        assert (_np(counts) == exact).all()


@pytest.mark.parametrize("n", [1, 5, 4096, 4097, 5000, 4096 * 1024 + 3])
def test_offsets_from_counts(n):
    import torch
    from bvh_amd import _lib
    rng = np.random.default_rng(n)
    counts = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)      # sums far beyond 32 bits
    dc = torch.from_numpy(counts.view(np.int32)).cuda()
    out = torch.full((n + 3,), -1, dtype=torch.int64, device="cuda")
    assert _lib.load().bvh_amd_offsets_from_counts(dc.data_ptr(), n, out.data_ptr() + 8, None) == 0, _lib.last_error()
    got = _np(out, np.uint64)
    want = np.concatenate([[0], np.cumsum(counts.astype(np.uint64), dtype=np.uint64)]).astype(np.uint64)
    assert (got[1:n + 2] == want).all()
    assert got[0] == np.uint64(0xFFFFFFFFFFFFFFFF) and got[n + 2] == np.uint64(0xFFFFFFFFFFFFFFFF)


def test_offsets_from_counts_python_and_empty():
    import bvh_amd
    import torch
    c = torch.tensor([3, 0, 2], dtype=torch.int32, device="cuda")
    assert bvh_amd.offsets_from_counts(c).tolist() == [0, 3, 3, 5]
    assert bvh_amd.offsets_from_counts(c[:0]).tolist() == [0]
    with pytest.raises(TypeError):
        bvh_amd.offsets_from_counts(c.long())


# ---- flags and errors ---------------------------------------------------------------------------------------------------------------

def test_flags_and_errors(orc):
    import bvh_amd
    import torch
    from bvh_amd import _lib
    g = load_golden("soup2k")
    bvh = bvh_amd.Bvh.deserialize(g["bvh_serial_low"].tobytes())
    _, _, prims, _, raw, ids = golden_scene("soup2k", "serial_low", orc)
    pts = np.random.default_rng(1).random((500, 3)).astype(np.float32)
    off, lst, dist = bvh_amd.radius_search(bvh, prims, pts, radius=0.1)
    oo, ol, od = bvh_amd.radius_search(bvh, prims, pts, radius=0.1, original_ids=True)
    assert len(lst) > 500 and (_np(oo) == _np(off)).all() and (_np(ol) == ids[_np(lst)]).all() and _np(od).tobytes() == _np(dist).tobytes()
    assert off.dtype == torch.int64 and lst.dtype == torch.int32 and dist.dtype == torch.float32 and off.shape == (501,)
    assert bvh_amd.radius_search(bvh, prims, pts, radius=0.1, distances=False)[2] is None
    q4 = _queries(pts, 0.1, np.float32)
    o4, l4, d4 = bvh_amd.radius_search(bvh, prims, q4)
    assert (_np(o4) == _np(off)).all() and _np(l4).tobytes() == _np(lst).tobytes() and _np(d4).tobytes() == _np(dist).tobytes()
    c = bvh_amd.radius_count(bvh, prims, q4)
    assert c.dtype == torch.int32 and c.shape == (500,) and (_np(c) == np.diff(_np(off))).all()
    with pytest.raises(ValueError):
        bvh_amd.radius_search(bvh, prims, q4, radius=1.0)
    with pytest.raises(ValueError):
        bvh_amd.radius_count(bvh, prims, q4, radius=1.0)
    e_off, e_ids, e_dist = bvh_amd.radius_search(bvh, prims, np.zeros((0, 3), np.float32), radius=1.0)
    assert e_off.tolist() == [0] and e_ids.shape == (0,) and e_dist.shape == (0,)
    assert bvh_amd.radius_count(bvh, prims, np.zeros((0, 3), np.float32), radius=1.0).shape == (0,)
    z_off, z_ids, _ = bvh_amd.radius_search(bvh, prims, pts + 100, radius=0.1)               # nothing within reach: empty lists
    assert z_off.tolist() == [0] * 501 and z_ids.shape == (0,)

    lib = _lib.load()
    dp, dq = torch.from_numpy(prims).cuda(), torch.from_numpy(q4).cuda()
    n = len(q4)
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    offs = (torch.arange(n + 1, dtype=torch.int64, device="cuda") * 2)
    lp = torch.zeros(2 * n + 4, dtype=torch.int32, device="cuda")
    ld = torch.zeros(2 * n + 4, dtype=torch.float32, device="cuda")
    f = lib.bvh3f_radius_search_tri
    P = lambda t: t.data_ptr()
    assert f(bvh._h, P(dp), P(dq), n, 0, P(counts), P(offs), P(lp), P(ld), None, None) == 0
    assert f(bvh._h, P(dp), P(dq), 0, 0, None, None, None, None, None, None) == 0                 # n == 0: no-op
    for bad in (1, 2, 32, 1 << 20):                                                              # ANY_HIT, ROBUST, unknown bits
        assert f(bvh._h, P(dp), P(dq), n, bad, P(counts), None, None, None, None, None) == -2
        assert "flags" in _lib.last_error()
    assert f(bvh._h, None, P(dq), n, 0, P(counts), None, None, None, None, None) == -2
    assert f(bvh._h, P(dp), None, n, 0, P(counts), None, None, None, None, None) == -2
    assert f(None, P(dp), P(dq), n, 0, P(counts), None, None, None, None, None) == -2
    assert f(bvh._h, P(dp), P(dq), n, 0, None, None, None, None, None, None) == -2                # neither counts nor offsets
    assert "d_counts" in _lib.last_error()
    assert f(bvh._h, P(dp), P(dq), n, 0, P(counts), P(offs), None, None, None, None) == -2        # offsets without a list
    assert "d_list_prims" in _lib.last_error()
    assert f(bvh._h, P(dp), P(dq), n, 0, P(counts), None, P(lp), None, None, None) == -2          # a list without offsets
    for args in ((P(dp), P(dq) + 4, n - 1, 0, P(counts), None, None, None, None, None),           # misaligned queries, prims, counts,
                 (P(dp) + 8, P(dq), n, 0, P(counts), None, None, None, None, None),               # offsets, list, distances, counters
                 (P(dp), P(dq), n, 0, P(counts) + 2, None, None, None, None, None),
                 (P(dp), P(dq), n, 0, P(counts), P(offs) + 4, P(lp), None, None, None),
                 (P(dp), P(dq), n, 0, P(counts), P(offs), P(lp) + 2, None, None, None),
                 (P(dp), P(dq), n, 0, P(counts), P(offs), P(lp), P(ld) + 2, None, None),
                 (P(dp), P(dq), n, 0, P(counts), None, None, None, P(ld) + 4, None)):
        assert f(bvh._h, *args) == -2
        assert "aligned" in _lib.last_error()
    assert f(bvh._h, P(dp), P(dq), n, 0, P(counts), P(offs), P(lp) + 4, P(ld) + 4, None, None) == 0   # 4-byte alignment is enough for the lists
    assert lib.bvh_amd_offsets_from_counts(P(counts), n, None, None) == -2
    assert lib.bvh_amd_offsets_from_counts(P(counts), n, P(offs) + 4, None) == -2
    g2 = load_golden("circles2k_2f")
    bb, cc = bvh_amd.sphere_bounds(g2["prims"])
    bvh2 = bvh_amd.DefaultBuilder.build(bb, cc)
    with pytest.raises(TypeError):
        bvh_amd.radius_search(bvh2, g2["prims"], np.zeros((4, 3), np.float32), radius=1.0, leaf="sphere")
    with pytest.raises(TypeError):
        bvh_amd.radius_count(bvh2, g2["prims"], np.zeros((4, 3), np.float32), radius=1.0, leaf="sphere")
    with pytest.raises(TypeError):
        bvh_amd.radius_search(bvh, prims, np.zeros((4, 3), np.float64), radius=1.0)
    with pytest.raises(TypeError):
        bvh_amd.radius_count(bvh, prims.astype(np.float64), np.zeros((4, 3), np.float32), radius=1.0)


def test_cpp_mirror_agrees(tmp_path):
    """tests/cpp/radius_search_amd.cpp (amd::radius_search_batch over the mirror, g++ -Wall -Wextra -Werror) gives the offsets, ids and
    distances bvh_amd.radius_search gives on the same tree."""
    import bvh_amd
    from bvh_amd import build
    build.build()
    lib = os.path.join(ROOT, "bvh_amd", "lib")
    exe = str(tmp_path / "radius_search_amd")
    cmd = ["g++", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "radius_search_amd.cpp"),
           "-L", lib, "-lbvh_amd", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    prim_ids = [int(x) for x in lines[0].split()[1:]]
    cpp_offsets = np.array([int(x) for x in lines[1].split()[1:]], dtype=np.int64)
    side = 12                                                 # the program's mesh, rebuilt here
    h = lambda i, j: np.float32(0.1 * np.sin(0.7 * i) * np.cos(0.4 * j))
    tris, queries = [], []
    for i in range(side):
        for j in range(side):
            a, b = [i, h(i, j), j], [i + 1, h(i + 1, j), j]
            c, d = [i + 1, h(i + 1, j + 1), j + 1], [i, h(i, j + 1), j + 1]
            tris += [a + b + c, a + c + d]
    radii = [np.float32(0.25), np.float32(1.5), np.inf]
    for k in range(200):
        queries.append([np.float32(-1.5 + 15.0 * ((k * 37) % 200) / 200.0), np.float32(-1.0 + 2.0 * ((k * 53) % 200) / 200.0),
                        np.float32(-1.5 + 15.0 * ((k * 91) % 200) / 200.0), radii[2] if k % 50 == 49 else radii[k % 2]])
    tris = np.array(tris, dtype=np.float32)
    bb, cc = bvh_amd.tri_bounds(tris)
    bvh = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.High))
    assert list(bvh.prim_ids) == prim_ids
    offsets, ids, dist = bvh_amd.radius_search(bvh, bvh_amd.precompute_tris(tris, bvh.device_prim_ids()), np.array(queries, np.float32))
    offsets, ids, dist = _np(offsets), _np(ids), _np(dist)
    assert (cpp_offsets == offsets).all() and offsets[-1] > 4 * 288 and len(lines) == 2 + offsets[-1]
    for e, line in enumerate(lines[2:]):
        qk, p, t = line.split()
        assert offsets[int(qk)] <= e < offsets[int(qk) + 1] and int(p) == ids[e] and np.float32(float.fromhex(t)) == dist[e], (line, e)
