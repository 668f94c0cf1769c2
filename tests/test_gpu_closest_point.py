"""MI355X: batched closest-point queries (bvhXX_closest_points_*, bvh_amd.closest_points). The device's records are byte-equal to
the host harness's (the same text compiled by g++, tests/test_closest_point_host.py), counters included; the distances agree with a
float64 brute force over the original vertices; records do not depend on batch order or the reordering flags; trees deeper than 64
levels; flags, errors and the C++ mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from test_closest_point_host import (INVALID, chain_queries, chain_tree, compile_harness, golden_scene, host_brute, host_walk,
                                     precompute, scene_queries)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return compile_harness(tmp_path_factory.mktemp("closest_gpu"))


def _queries(pts, r, dt):
    q = np.zeros((len(pts), 4), dtype=dt)
    q[:, :3] = pts
    q[:, 3] = r
    return q


def _device_vs_host(dll, bvh, dprims, raw_q, leaf, counters=True):
    import bvh_amd
    import torch
    hits, cnt = bvh_amd.closest_points(bvh, dprims, raw_q, leaf="sphere" if leaf else "tri", counters=True)
    torch.cuda.synchronize()
    nodes = bvh.nodes
    h_hits, h_cnt = host_walk(dll, nodes["bounds"], nodes["index"], dprims.cpu().numpy(), raw_q, leaf, threads=8)
    assert bvh_amd.hits_to_numpy(hits).tobytes() == h_hits.tobytes()
    if counters:
        assert (cnt.cpu().numpy().astype(np.uint64) == h_cnt).all(), (cnt, h_cnt)
    return h_hits


@pytest.mark.parametrize("scene", ["cornell", "soup2k", "terrain2k", "soup2k_f64", "spheres2k_f64"])
def test_device_equals_host_golden(dll, orc, scene):
    import bvh_amd
    g = load_golden(scene)
    double = g["prims"].dtype == np.float64
    bvh = bvh_amd.Bvh.deserialize(g["bvh_parallel_high"].tobytes(), dtype=np.float64 if double else np.float32)
    _, _, prims, leaf, raw, _ = golden_scene(scene, "parallel_high", orc)
    import torch
    dprims = torch.from_numpy(prims).cuda()
    pts, diag = scene_queries(raw, 2048, prims.dtype, 3, leaf == 1)
    for r in (np.inf, 0.02 * diag):
        _device_vs_host(dll, bvh, dprims, _queries(pts, r, prims.dtype), leaf)


def test_device_equals_host_float_spheres(dll):
    import bvh_amd
    from bvh_amd import synth
    sph = synth.spheres(20000, dtype=np.float32)
    bb, cc = bvh_amd.sphere_bounds(sph)
    bvh = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.Medium))
    dprims = bvh_amd.gather(sph, bvh.device_prim_ids())
    pts, _ = scene_queries(sph, 8192, np.float32, 4, True)
    _device_vs_host(dll, bvh, dprims, _queries(pts, np.inf, np.float32), 1)


@pytest.fixture(scope="module")
def soup_1m_high():
    import bvh_amd
    from bvh_amd import synth
    tris = synth.soup(1 << 20)
    bb, cc = bvh_amd.tri_bounds(tris)
    bvh = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.High))
    return tris, bvh, bvh_amd.precompute_tris(tris, bvh.device_prim_ids())


def test_device_equals_host_1m_high(dll, soup_1m_high):
    from bvh_amd import synth
    tris, bvh, dprims = soup_1m_high
    lo, hi = synth.scene_bounds(tris)
    pts = np.concatenate([synth.points_uniform(2048, lo, hi, seed=8), synth.points_near_surface(tris, 2048, seed=9, sigma=0.01)])
    _device_vs_host(dll, bvh, dprims, _queries(pts, np.inf, np.float32), 0)


# ---- against a float64 brute force on the GPU -----------------------------------------------------------------------------------

def _dist_f64(torch, q, prim, sphere):
    """float64 distance from q to prim (broadcasting (..., 3) / (..., 9 or 4)): a sphere's max(|q - c| - r, 0); a triangle's plane foot
    where it falls inside the triangle, else the nearest of its three edges (from the original vertices)."""
    if sphere:
        return (torch.linalg.vector_norm(q - prim[..., :3], dim=-1) - prim[..., 3]).clamp_min(0)
    a, b, c = prim[..., 0:3], prim[..., 3:6], prim[..., 6:9]
    ab, ac, bc = b - a, c - a, c - b
    dot = lambda x, y: (x * y).sum(-1)
    one = lambda x: torch.where(x > 0, x, torch.ones_like(x))

    def seg(qa, e):
        ee = dot(e, e)
        t = (dot(qa, e) / one(ee)).clamp(0, 1)
        return dot(qa - t[..., None] * e, qa - t[..., None] * e)

    qa, qb = q - a, q - b
    e2 = torch.minimum(torch.minimum(seg(qa, ab), seg(qa, ac)), seg(qb, bc))
    n = torch.cross(ab.expand_as(qa), ac.expand_as(qa), dim=-1)
    nn = dot(n, n)
    d00, d01, d11, d20, d21 = dot(ab, ab), dot(ab, ac), dot(ac, ac), dot(qa, ab), dot(qa, ac)
    den = d00 * d11 - d01 * d01
    v, w = (d11 * d20 - d01 * d21) / one(den), (d00 * d21 - d01 * d20) / one(den)
    inside = (den > 0) & (nn > 0) & (v >= 0) & (w >= 0) & (v + w <= 1)
    pn = dot(qa, n)
    return torch.where(inside, pn * pn / one(nn), e2).sqrt()


def brute_f64(torch, raw, pts):
    """float64 distance from every point to its nearest primitive, on the GPU, chunked over the points."""
    P = torch.from_numpy(np.ascontiguousarray(raw, dtype=np.float64)).cuda()
    Q = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float64)).cuda()
    sphere = raw.shape[1] == 4
    out = torch.empty(len(pts), dtype=torch.float64, device="cuda")
    chunk = max(1, (1 << 22) // len(raw))
    for s in range(0, len(pts), chunk):
        out[s:s + chunk] = _dist_f64(torch, Q[s:s + chunk, None, :], P[None], sphere).min(dim=1).values
    return out.cpu().numpy()


def pair_f64(torch, prims, pts):
    """float64 distance of pts[k] to prims[k]."""
    P = torch.from_numpy(np.ascontiguousarray(prims, dtype=np.float64)).cuda()
    Q = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float64)).cuda()
    return _dist_f64(torch, Q, P, prims.shape[1] == 4).cpu().numpy()


def _scene(name):
    from bvh_amd import synth
    return {"soup100k": lambda: synth.soup(100_000), "terrain65k": lambda: synth.terrain(65_536),
            "sponza262k": lambda: synth.sponza_proxy(262_144), "spheres100k": lambda: synth.spheres(100_000)}[name]()


@pytest.mark.parametrize("name", ["soup100k", "terrain65k", "sponza262k", "spheres100k"])
def test_against_f64_brute_force(name):
    import bvh_amd
    import torch
    from bvh_amd import synth
    raw = _scene(name)
    sphere = raw.shape[1] == 4
    dt = raw.dtype
    bb, cc = bvh_amd.sphere_bounds(raw) if sphere else bvh_amd.tri_bounds(raw)
    bvh = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.High))
    dprims = bvh_amd.gather(raw, bvh.device_prim_ids()) if sphere else bvh_amd.precompute_tris(raw, bvh.device_prim_ids())
    lo, hi = synth.scene_bounds(raw)
    n = 16384
    verts = raw[:, :3] if sphere else raw.reshape(-1, 3)
    rng = np.random.default_rng(17)
    kinds = [synth.points_uniform(n, lo, hi, seed=21, dtype=np.float64),
             synth.points_near_surface(raw.astype(np.float64), n, seed=22, sigma=0.01 * float(np.max(hi - lo))) if not sphere
             else synth.points_uniform(n, lo, hi, seed=25, scale=0.5, dtype=np.float64),
             synth.points_uniform(n, lo, hi, seed=23, scale=10.0, dtype=np.float64),                      # far outside
             verts[rng.integers(0, len(verts), n)].astype(np.float64)]                                   # exactly on a vertex (a centre for spheres)
    pts = np.concatenate(kinds).astype(dt)
    d_ref = brute_f64(torch, raw, pts)
    ids = bvh.prim_ids.astype(np.int64)
    # Tolerance: the kernel forms q - p0 and the edge dot products in the scalar type; with coordinates of magnitude M (the scene's and
    # the far queries', up to 10x the box) each rounding is at most ulp(M) / 2 and the distance collects a handful of them, so 16 ulps of M.
    M = float(max(np.abs(raw).max(), np.abs(pts).max()))
    tol = 16 * np.finfo(dt).eps * M
    diag = float(np.linalg.norm(hi - lo))
    for r in (np.inf, 0.01 * diag):
        hits = bvh_amd.hits_to_numpy(bvh_amd.closest_points(bvh, dprims, pts, max_distance=r, leaf="sphere" if sphere else "tri"))
        hit = hits["prim"] != INVALID
        clear = np.abs(d_ref - r) > tol
        assert (hit[clear] == (d_ref <= r)[clear]).all(), name
        assert (np.abs(hits["t"][hit].astype(np.float64) - d_ref[hit]) <= tol).all(), (name, np.abs(hits["t"][hit] - d_ref[hit]).max(), tol)
        # the float64 distance of the primitive it returned is within 2 tol of the true minimum
        got = ids[hits["prim"][hit]]
        d_got = pair_f64(torch, raw[got], pts[hit])
        assert (d_got <= d_ref[hit] + 2 * tol).all(), name
        assert (hits["t"][~hit] == np.asarray(r, dtype=dt)).all()



def test_order_invariance(soup_1m_high):
    """A permuted batch, and the forced SORTED / UNSORTED paths, give byte-identical records per query."""
    import bvh_amd
    import torch
    from bvh_amd import synth
    tris, bvh, dprims = soup_1m_high
    lo, hi = synth.scene_bounds(tris)
    pts = np.concatenate([synth.points_uniform(1 << 15, lo, hi, seed=31), synth.points_near_surface(tris, 1 << 15, seed=32, sigma=0.01)])
    q = _queries(pts, 0.02, np.float32)
    q[::7, 3] = np.inf
    base = bvh_amd.hits_to_numpy(bvh_amd.closest_points(bvh, dprims, q, sort_queries=False))
    assert bvh_amd.hits_to_numpy(bvh_amd.closest_points(bvh, dprims, q, sort_queries=True)).tobytes() == base.tobytes()
    assert bvh_amd.hits_to_numpy(bvh_amd.closest_points(bvh, dprims, q)).tobytes() == base.tobytes()
    perm = np.random.default_rng(3).permutation(len(q))
    permuted = bvh_amd.hits_to_numpy(bvh_amd.closest_points(bvh, dprims, torch.from_numpy(q[perm]).cuda(), sort_queries=True))
    assert permuted.tobytes() == base[perm].tobytes()
    sub = bvh_amd.hits_to_numpy(bvh_amd.closest_points(bvh, dprims, q[1000:1100]))   # batch size and position do not matter either
    assert sub.tobytes() == base[1000:1100].tobytes()


@pytest.mark.parametrize("depth", [65, 300, 3000])
def test_trees_deeper_than_64_levels(dll, restatement, depth):
    import bvh_amd
    tris, nodes, ids = chain_tree(depth, restatement.prep_tris)
    bvh = bvh_amd.Bvh.from_nodes(nodes, ids)
    prims = precompute(tris, np.float32)
    q = chain_queries(depth, 4096)
    hits = bvh_amd.hits_to_numpy(bvh_amd.closest_points(bvh, prims, q))
    brute_d2, bi = host_brute(dll, prims, q, 0)
    assert (hits["prim"] == bi).all() and (hits["prim"] == depth).all()
    assert (hits["t"] == np.sqrt(brute_d2)).all()


def test_flags_and_errors(orc):
    import bvh_amd
    import torch
    from bvh_amd import _lib
    g = load_golden("soup2k")
    bvh = bvh_amd.Bvh.deserialize(g["bvh_serial_low"].tobytes())
    _, _, prims, _, raw, ids = golden_scene("soup2k", "serial_low", orc)
    pts = np.random.default_rng(1).random((500, 3)).astype(np.float32)
    h = bvh_amd.hits_to_numpy(bvh_amd.closest_points(bvh, prims, pts))
    ho = bvh_amd.hits_to_numpy(bvh_amd.closest_points(bvh, prims, pts, original_ids=True))
    assert (ho["prim"] == ids[h["prim"]]).all() and (ho["t"] == h["t"]).all()
    q4 = _queries(pts, 0.01, np.float32)
    assert bvh_amd.hits_to_numpy(bvh_amd.closest_points(bvh, prims, q4)).tobytes() == \
        bvh_amd.hits_to_numpy(bvh_amd.closest_points(bvh, prims, pts, max_distance=0.01)).tobytes()
    with pytest.raises(ValueError):
        bvh_amd.closest_points(bvh, prims, q4, max_distance=1.0)
    assert bvh_amd.closest_points(bvh, prims, np.zeros((0, 3), np.float32)).shape == (0, 4)
    lib = _lib.load()
    dp, dq = torch.from_numpy(prims).cuda(), torch.from_numpy(q4).cuda()
    out = torch.empty((len(q4), 4), dtype=torch.float32, device="cuda")
    f = lib.bvh3f_closest_points_tri
    assert f(bvh._h, dp.data_ptr(), dq.data_ptr(), 0, 0, None, None, None) == 0                  # n == 0: no-op
    for bad in (1, 2, 32, 1 << 20):                                                              # ANY_HIT, ROBUST, unknown bits
        assert f(bvh._h, dp.data_ptr(), dq.data_ptr(), len(q4), bad, out.data_ptr(), None, None) == -2
        assert "flags" in _lib.last_error()
    assert f(bvh._h, None, dq.data_ptr(), len(q4), 0, out.data_ptr(), None, None) == -2
    assert f(bvh._h, dp.data_ptr(), dq.data_ptr() + 4, len(q4) - 1, 0, out.data_ptr(), None, None) == -2
    assert "aligned" in _lib.last_error()
    assert f(None, dp.data_ptr(), dq.data_ptr(), len(q4), 0, out.data_ptr(), None, None) == -2
    g2 = load_golden("circles2k_2f")
    bb, cc = bvh_amd.sphere_bounds(g2["prims"])
    bvh2 = bvh_amd.DefaultBuilder.build(bb, cc)
    with pytest.raises(TypeError):
        bvh_amd.closest_points(bvh2, g2["prims"], np.zeros((4, 3), np.float32), leaf="sphere")
    with pytest.raises(TypeError):
        bvh_amd.closest_points(bvh, prims, np.zeros((4, 3), np.float64))


def test_cpp_mirror_agrees(tmp_path):
    """tests/cpp/closest_points_amd.cpp (amd::closest_points_batch over the mirror, g++ -Wall -Wextra -Werror) gives the records
    bvh_amd.closest_points gives on the same tree."""
    import bvh_amd
    from bvh_amd import build
    build.build()
    lib = os.path.join(ROOT, "bvh_amd", "lib")
    exe = str(tmp_path / "closest_points_amd")
    cmd = ["g++", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "closest_points_amd.cpp"),
           "-L", lib, "-lbvh_amd", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    prim_ids = [int(x) for x in lines[0].split()[1:]]
    side = 12                                                 # the program's mesh, rebuilt here
    h = lambda i, j: np.float32(0.1 * np.sin(0.7 * i) * np.cos(0.4 * j))
    tris, queries = [], []
    for i in range(side):
        for j in range(side):
            a, b = [i, h(i, j), j], [i + 1, h(i + 1, j), j]
            c, d = [i + 1, h(i + 1, j + 1), j + 1], [i, h(i, j + 1), j + 1]
            tris += [a + b + c, a + c + d]
    for k in range(200):
        queries.append([np.float32(-1.5 + 15.0 * ((k * 37) % 200) / 200.0), np.float32(-1.0 + 2.0 * ((k * 53) % 200) / 200.0),
                        np.float32(-1.5 + 15.0 * ((k * 91) % 200) / 200.0), np.float32(0.25) if k % 2 else np.inf])
    tris = np.array(tris, dtype=np.float32)
    bb, cc = bvh_amd.tri_bounds(tris)
    bvh = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.High))
    assert list(bvh.prim_ids) == prim_ids
    hits = bvh_amd.hits_to_numpy(bvh_amd.closest_points(bvh, bvh_amd.precompute_tris(tris, bvh.device_prim_ids()), np.array(queries, np.float32)))
    for line, hit in zip(lines[1:], hits):
        p, t, u, v = line.split()
        assert int(p) == hit["prim"] and np.float32(float.fromhex(t)) == hit["t"], (line, hit)
        assert np.float32(float.fromhex(u)) == hit["u"] and np.float32(float.fromhex(v)) == hit["v"], (line, hit)
    assert len(lines) == 201 and (hits["prim"] != INVALID).sum() > 100
