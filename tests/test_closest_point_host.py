"""CPU: the TEXT of the closest-point kernel (bvh_amd/csrc/closest_body.inc + point_walk.inc + trace_device.h) compiled for the host by
tests/cpp/closest_body_host.cpp. The per-primitive distance functions, float and double, against a float64 closest point on crafted
cases (the seven Voronoi regions of a triangle, points on it, degenerate triangles, vertices collinear up to rounding, spheres); the
walk over the golden trees against a brute force over the same function. The device's records must equal this harness's bit for bit (tests/test_gpu_closest_point.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden, parse_stream
from test_kernel_body_host import _aligned, pair_records

HARNESS = os.path.join(ROOT, "tests", "cpp", "closest_body_host.cpp")
INVALID = 0xFFFFFFFF
HITF = np.dtype([("prim", "<u4"), ("t", "<f4"), ("u", "<f4"), ("v", "<f4")])
HITD = np.dtype([("prim", "<u4"), ("pad", "<u4"), ("t", "<f8"), ("u", "<f8"), ("v", "<f8")])


def compile_harness(out_dir):
    out = os.path.join(str(out_dir), "libclosest_body_host.so")
    cmd = ["g++", "-std=c++20", "-O1", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-strict-aliasing", "-Wall", "-Wextra", "-Wno-unused-parameter",
           "-Wno-unknown-pragmas", "-Werror", "-shared", "-fPIC", "-pthread", HARNESS, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    dll = C.CDLL(out)
    P, Z, I, U = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32
    dll.closest_host_tri.argtypes = [I, P, P, P]
    dll.closest_host_sphere.argtypes = [I, P, P, P]
    dll.closest_host_walk.restype = I
    dll.closest_host_walk.argtypes = [I, I, P, U, P, P, Z, P, P, U, I, P, P]
    dll.closest_host_eval.argtypes = [I, I, P, P, Z, P, P, P, P]
    dll.closest_host_brute.argtypes = [I, I, P, Z, P, Z, P, P, I]
    return dll


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_walk(dll, bounds6, index, prims, queries, leaf, order=None, prim_ids=None, deep_cap=0, threads=1):
    """The kernel's walk for every query ({x, y, z, max_distance} rows): (hit records, counters {pairs, tests, leaves})."""
    double = bounds6.dtype == np.float64
    pairs = _aligned(pair_records(bounds6, index))
    prims = _aligned(np.ascontiguousarray(prims))
    queries = _aligned(np.ascontiguousarray(queries))
    hits = np.zeros(len(queries), dtype=HITD if double else HITF)
    cnt = np.zeros(3, dtype=np.uint64)
    order = None if order is None else np.ascontiguousarray(order, dtype=np.uint32)
    prim_ids = None if prim_ids is None else np.ascontiguousarray(prim_ids, dtype=np.uint32)
    assert dll.closest_host_walk(int(double), leaf, _p(pairs), int(index[0]) & 0xFFFFFFFF, _p(prims), _p(queries), len(queries), _p(order),
                                 _p(prim_ids), deep_cap, threads, _p(hits), _p(cnt)) == 0
    return hits, cnt


def host_eval(dll, prims, queries, prim, leaf):
    dt = prims.dtype
    d2 = np.zeros(len(queries), dtype=dt)
    pr = np.ascontiguousarray(prim, dtype=np.uint32)
    dll.closest_host_eval(int(dt == np.float64), leaf, _p(np.ascontiguousarray(prims)), _p(np.ascontiguousarray(queries)), len(queries), _p(pr), _p(d2), None, None)
    return d2


def host_brute(dll, prims, queries, leaf, threads=4):
    dt = prims.dtype
    d2 = np.zeros(len(queries), dtype=dt)
    idx = np.zeros(len(queries), dtype=np.uint32)
    dll.closest_host_brute(int(dt == np.float64), leaf, _p(np.ascontiguousarray(prims)), len(prims), _p(np.ascontiguousarray(queries)), len(queries),
                           _p(d2), _p(idx), threads)
    return d2, idx


def precompute(tris9, dtype):
    """PrecomputedTri {p0, e1 = p0 - p1, e2 = p2 - p0, n = cross(e1, e2)} (tri.h:35-37), each operation rounded in `dtype`."""
    t = np.asarray(tris9, dtype=dtype).reshape(-1, 3, 3)
    p0, p1, p2 = t[:, 0], t[:, 1], t[:, 2]
    e1, e2 = p0 - p1, p2 - p0
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    return np.concatenate([p0, e1, e2, n], axis=1).astype(dtype)


def _seg(q, a, b):
    ab = b - a
    den = ab @ ab
    t = 0.0 if den == 0 else min(1.0, max(0.0, (q - a) @ ab / den))
    return np.linalg.norm(q - (a + t * ab))


def ref_tri_distance(tri9, q):
    """float64 distance from q to the solid triangle (plane projection when it falls inside, else the nearest edge)."""
    a, b, c = (np.asarray(tri9, np.float64).reshape(3, 3))
    q = np.asarray(q, np.float64)
    n = np.cross(b - a, c - a)
    nn = n @ n
    best = min(_seg(q, a, b), _seg(q, a, c), _seg(q, b, c))
    if nn > 0:
        p = q - ((q - a) @ n / nn) * n
        m = np.array([b - a, c - a]).T
        uv, *_ = np.linalg.lstsq(m, p - a, rcond=None)
        if uv[0] >= 0 and uv[1] >= 0 and uv[0] + uv[1] <= 1:
            best = min(best, np.linalg.norm(q - p))
    return best


TRI = np.array([0.2, -0.1, 0.3, 1.7, 0.4, -0.2, -0.3, 1.5, 0.6])     # a tilted, scalene triangle
A, B, Cv = TRI[0:3], TRI[3:6], TRI[6:9]
NRM = np.cross(B - A, Cv - A) / np.linalg.norm(np.cross(B - A, Cv - A))
CEN = (A + B + Cv) / 3
# one query in each of the seven Voronoi regions, and points ON the triangle (distance 0)
REGION_QUERIES = {
    "vertex_a": A + 0.7 * (A - CEN) + 0.3 * NRM, "vertex_b": B + 0.5 * (B - CEN) - 0.4 * NRM, "vertex_c": Cv + 0.6 * (Cv - CEN) + 0.2 * NRM,
    "edge_ab": (A + B) / 2 + 0.8 * ((A + B) / 2 - Cv) + 0.3 * NRM, "edge_ac": (A + Cv) / 2 + 0.5 * ((A + Cv) / 2 - B) - 0.5 * NRM,
    "edge_bc": 0.3 * B + 0.7 * Cv + 0.4 * (0.3 * B + 0.7 * Cv - A) + 0.1 * NRM, "interior": 0.2 * A + 0.5 * B + 0.3 * Cv + 0.9 * NRM,
    "on_vertex": B.copy(), "on_edge": 0.25 * A + 0.75 * Cv, "on_interior": 0.4 * A + 0.35 * B + 0.25 * Cv,
}
DEGENERATE = {
    "collinear": [0, 0, 0, 1, 1, 1, 3, 3, 3], "collinear_middle": [0, 0, 0, 2, 0, 0, 1, 0, 0],
    "two_coincident": [0, 0, 0, 0, 0, 0, 1, 0.5, 0], "two_coincident_bc": [0, 0, 0, 1, 0, 0, 1, 0, 0], "three_coincident": [1, 2, 3, 1, 2, 3, 1, 2, 3],
}
DEGENERATE_QUERIES = [[0.5, 1.0, 0.0], [-1, -1, -1], [5, 4, 3], [1.0, 0.0, 0.0], [0.5, 0.25, 0.0], [0.3, -2, 1.1], [1, 2, 3]]


def _tol(dtype, *mags):
    return 16 * np.finfo(dtype).eps * (1.0 + max(float(np.max(np.abs(m))) for m in mags))


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return compile_harness(tmp_path_factory.mktemp("closest"))


def _tri_query(dll, tri9, q, dtype):
    pre = np.ascontiguousarray(precompute(np.asarray(tri9).reshape(1, 9), dtype)[0])
    qq = np.ascontiguousarray(np.asarray(q, dtype=dtype))
    out = np.zeros(3, dtype=dtype)
    dll.closest_host_tri(int(dtype == np.float64), _p(pre), _p(qq), _p(out))
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", list(REGION_QUERIES))
def test_triangle_regions(dll, dtype, name):
    tri = TRI.astype(dtype).astype(np.float64)
    q = REGION_QUERIES[name].astype(dtype).astype(np.float64)
    d2, u, v = (float(x) for x in _tri_query(dll, tri, q, dtype))
    ref = ref_tri_distance(tri, q)
    tol = _tol(dtype, tri, q)
    assert np.isfinite(d2) and abs(np.sqrt(d2) - ref) <= tol, (name, np.sqrt(d2), ref)
    if name.startswith("on_"):
        assert np.sqrt(d2) <= tol
    p0, p1, p2 = tri.reshape(3, 3)
    point = p0 + u * (p1 - p0) + v * (p2 - p0)             # the ray record's barycentric convention
    assert abs(np.linalg.norm(q - point) - np.sqrt(d2)) <= 4 * tol, (name, u, v)
    assert -tol <= u <= 1 + tol and -tol <= v <= 1 + tol and u + v <= 1 + tol


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", list(DEGENERATE))
def test_degenerate_triangles(dll, dtype, name):
    tri = np.asarray(DEGENERATE[name], np.float64).astype(dtype).astype(np.float64)
    for q in DEGENERATE_QUERIES:
        q = np.asarray(q, np.float64).astype(dtype).astype(np.float64)
        d2, u, v = (float(x) for x in _tri_query(dll, tri, q, dtype))
        assert np.isfinite(d2) and np.isfinite(u) and np.isfinite(v), (name, q)
        ref = ref_tri_distance(tri, q)
        tol = _tol(dtype, tri, q)
        assert abs(np.sqrt(d2) - ref) <= tol, (name, q, np.sqrt(d2), ref)
        p0, p1, p2 = tri.reshape(3, 3)
        assert abs(np.linalg.norm(q - (p0 + u * (p1 - p0) + v * (p2 - p0))) - np.sqrt(d2)) <= 4 * tol, (name, q, u, v)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_collinear_triangles_after_rounding(dll, dtype):
    """Three points of a random line rounded to the scalar type: the vertices are collinear up to rounding, so the normal is almost
    never exactly zero and the plane foot's determinant is noise. The distance must be that of the nearest edge (the minimum of the
    three segment distances in float64 is an upper bound on the true distance, and for such a sliver within rounding of it), and
    (u, v) must rebuild a point at that distance."""
    rng = np.random.default_rng(41)
    nonzero_normals = 0
    for _ in range(3000):
        a, d, s = rng.normal(size=3), rng.normal(size=3), rng.normal(size=3) * 2
        tri = np.concatenate([a + s[0] * d, a + s[1] * d, a + s[2] * d]).astype(dtype)
        q = (a + rng.normal(size=3) * rng.choice([1e-3, 0.1, 1.0, 10.0])).astype(dtype)
        t64, q64 = tri.astype(np.float64), q.astype(np.float64)
        p0, p1, p2 = t64.reshape(3, 3)
        nonzero_normals += bool(np.any(precompute(tri.reshape(1, 9), dtype)[0, 9:] != 0))
        seg_min = min(_seg(q64, p0, p1), _seg(q64, p0, p2), _seg(q64, p1, p2))
        d2, u, v = (float(x) for x in _tri_query(dll, tri, q, dtype))
        tol = _tol(dtype, t64, q64)
        assert np.isfinite(d2) and np.isfinite(u) and np.isfinite(v)
        assert np.sqrt(d2) <= seg_min + tol, (tri, q, np.sqrt(d2), seg_min)
        assert np.sqrt(d2) >= ref_tri_distance(t64, q64) - tol, (tri, q, np.sqrt(d2))
        assert abs(np.linalg.norm(q64 - (p0 + u * (p1 - p0) + v * (p2 - p0))) - np.sqrt(d2)) <= 4 * tol, (tri, q, u, v)
    assert nonzero_normals > 1000                             # the case that needs the fallback: a normal of rounding noise


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_sphere_distance(dll, dtype):
    s = np.array([0.5, -1.0, 2.0, 0.75], dtype=dtype)
    cases = {"inside": ([0.6, -0.9, 2.1], 0.0), "center": ([0.5, -1.0, 2.0], 0.0), "surface": ([1.25, -1.0, 2.0], 0.0),
             "outside": ([0.5, 2.0, 6.0], 5.0 - 0.75)}
    for name, (q, ref) in cases.items():
        qq = np.ascontiguousarray(np.asarray(q, dtype=dtype))
        out = np.zeros(1, dtype=dtype)
        dll.closest_host_sphere(int(dtype == np.float64), _p(s), _p(qq), _p(out))
        assert abs(np.sqrt(float(out[0])) - ref) <= _tol(dtype, s, qq), (name, out[0])


def golden_scene(name, mode, orc):
    """(bounds6, index, BVH-order prims, leaf, raw primitives) of a golden tree."""
    g = load_golden(name)
    double = g["prims"].dtype == np.float64
    nodes, ids = parse_stream(g[f"bvh_{mode}"].tobytes(), double)
    sphere = "spheres" in name
    prims = g["prims"][ids.astype(np.int64)] if sphere else orc.precompute_tris(g["prims"], ids)
    return nodes["bounds"], nodes["index"], np.ascontiguousarray(prims), 1 if sphere else 0, g["prims"], ids


def scene_queries(raw, n, dtype, seed, sphere):
    from bvh_amd import synth
    lo, hi = synth.scene_bounds(raw)
    pts = [synth.points_uniform(n, lo, hi, seed=seed, scale=1.3, dtype=np.float64)]
    if not sphere:
        pts.append(synth.points_near_surface(raw.astype(np.float64), n, seed=seed + 1, sigma=0.01 * float(np.max(hi - lo))))
    return np.concatenate(pts).astype(dtype), float(np.linalg.norm(hi - lo))


GOLDEN_SCENES = ["cornell", "soup2k", "terrain2k", "soup2k_f64", "spheres2k_f64"]


@pytest.mark.parametrize("scene", GOLDEN_SCENES)
@pytest.mark.parametrize("mode", ["serial_low", "parallel_high"])
def test_walk_equals_brute_force(dll, orc, scene, mode):
    bounds, index, prims, leaf, raw, _ = golden_scene(scene, mode, orc)
    dt = prims.dtype
    pts, diag = scene_queries(raw, 1024, dt, 11, leaf == 1)
    q = np.zeros((len(pts), 4), dtype=dt)
    q[:, :3] = pts
    q[:, 3] = np.inf
    hits, cnt = host_walk(dll, bounds, index, prims, q, leaf)
    assert (hits["prim"] != INVALID).all() and cnt[0] > 0 and cnt[1] > 0 and cnt[2] > 0
    brute_d2, _ = host_brute(dll, prims, q, leaf)
    walk_d2 = host_eval(dll, prims, q, hits["prim"], leaf)
    tol = 8 * np.finfo(dt).eps * (1.0 + float(np.abs(raw).max()) + diag)
    assert (walk_d2 >= brute_d2).all()                       # the walk tests a subset of what the brute force tests, with the same function
    assert (np.sqrt(walk_d2.astype(np.float64)) - np.sqrt(brute_d2.astype(np.float64)) <= tol).all()
    assert (hits["t"] == np.sqrt(walk_d2)).all()             # t = sqrt(d2), correctly rounded
    # a finite radius: hit / miss agree with the brute force away from the boundary; misses report the radius
    r = np.asarray(0.05 * diag, dtype=dt)
    q[:, 3] = r
    hr, _ = host_walk(dll, bounds, index, prims, q, leaf)
    bd = np.sqrt(brute_d2.astype(np.float64))
    clear = np.abs(bd - float(r)) > tol
    assert ((hr["prim"] != INVALID)[clear] == (bd <= float(r))[clear]).all()
    assert (hr["t"][hr["prim"] == INVALID] == r).all()
    assert (hr["u"][hr["prim"] == INVALID] == 0).all()
    # the record of a query does not depend on the order the batch is read in
    perm = np.random.default_rng(5).permutation(len(q)).astype(np.uint32)
    hp, cp = host_walk(dll, bounds, index, prims, q, leaf, order=perm)
    assert hp.tobytes() == hr.tobytes()


def test_misses_and_invalid_queries(dll, orc):
    bounds, index, prims, leaf, raw, ids = golden_scene("soup2k", "serial_low", orc)
    q = np.array([[0.5, 0.5, 0.5, np.inf], [np.nan, 0.5, 0.5, np.inf], [0.5, 0.5, 0.5, -1.0], [0.5, 0.5, 0.5, np.nan],
                  [50, 50, 50, 1.0], [0.5, 0.5, 0.5, 0.0], [0.5, 0.5, 0.5, 1e30]], dtype=np.float32)
    hits, _ = host_walk(dll, bounds, index, prims, q, leaf)
    assert hits["prim"][0] != INVALID and hits["prim"][6] == hits["prim"][0]
    for k in (1, 2, 3, 4):
        assert hits["prim"][k] == INVALID and hits["u"][k] == 0 and hits["v"][k] == 0
    assert hits["t"][2] == -1.0 and np.isnan(hits["t"][3]) and hits["t"][4] == 1.0
    assert hits["prim"][5] == INVALID or hits["t"][5] == 0
    # original ids: the same walk, prim = prim_ids[BVH-order index]
    ho, _ = host_walk(dll, bounds, index, prims, q, leaf, prim_ids=ids.astype(np.uint32))
    assert ho["prim"][0] == ids[hits["prim"][0]] and ho["t"][0] == hits["t"][0]


def chain_tree(depth, prep_tris):
    """The chain-shaped tree of test_gpu_traverse.py's deep-stack test: n = depth + 1 triangles at x = 4000 - k, every inner node's
    inner child nearer to a query in front of them than its leaf sibling, so the walk stacks one entry per level."""
    from oracle import NODEF
    n = depth + 1
    tris = np.zeros((n, 9), dtype=np.float32)
    for k in range(n):
        x = np.float32(4000 - k)
        tris[k] = [x, -1, -1, x, 1, -1, x, 0, 1]
    bb, _ = prep_tris(tris)
    nodes = np.zeros(2 * n - 1, dtype=NODEF)
    suffix = bb.copy()
    for k in range(n - 2, -1, -1):
        suffix[k, :3] = np.minimum(bb[k, :3], suffix[k + 1, :3])
        suffix[k, 3:] = np.maximum(bb[k, 3:], suffix[k + 1, 3:])
    box = lambda b: [b[0], b[3], b[1], b[4], b[2], b[5]]
    nodes[0]["bounds"], nodes[0]["index"] = box(suffix[0]), 1 << 4
    for k in range(n - 1):
        leaf, rest = 2 * k + 1, 2 * k + 2
        nodes[leaf]["bounds"], nodes[leaf]["index"] = box(bb[k]), (k << 4) | 1
        if k == n - 2:
            nodes[rest]["bounds"], nodes[rest]["index"] = box(bb[n - 1]), ((n - 1) << 4) | 1
        else:
            nodes[rest]["bounds"], nodes[rest]["index"] = box(suffix[k + 1]), (2 * k + 3) << 4
    return tris, nodes, np.arange(n, dtype=np.uint64)


def chain_queries(depth, n):
    rng = np.random.default_rng(depth)
    q = np.zeros((n, 4), dtype=np.float32)
    q[:, 0] = rng.random(n) * 100                            # in front of the stack of triangles: the deepest leaf is nearest
    q[:, 1:3] = (rng.random((n, 2)) - 0.5) * 1.5
    q[:, 3] = np.inf
    return q


@pytest.mark.parametrize("depth", [65, 300])
def test_deep_chain(dll, orc, depth):
    tris, nodes, ids = chain_tree(depth, orc.prep_tris)
    prims = precompute(tris, np.float32)
    q = chain_queries(depth, 64)
    hits, _ = host_walk(dll, nodes["bounds"], nodes["index"], prims, q, 0, deep_cap=depth - 64 + 1)
    brute_d2, bi = host_brute(dll, prims, q, 0)
    assert (hits["prim"] == bi).all() and (hits["prim"] == depth).all()
    assert (hits["t"] == np.sqrt(brute_d2)).all()


def test_deep_chain_fills_the_spill(dll, orc):
    """70 levels, one push per level: the stack crosses LDS -> scratch (entry 8), scratch -> HBM (entry 64) and ends on the last of
    the 6 HBM entries it is given."""
    depth = 70
    tris, nodes, ids = chain_tree(depth, orc.prep_tris)
    prims = precompute(tris, np.float32)
    q = chain_queries(depth, 48)
    hits, cnt = host_walk(dll, nodes["bounds"], nodes["index"], prims, q, 0, deep_cap=depth - 64)
    brute_d2, bi = host_brute(dll, prims, q, 0)
    assert (hits["prim"] == bi).all() and (hits["prim"] == depth).all()
    assert (hits["t"] == np.sqrt(brute_d2)).all()
    assert cnt[0] == depth * len(q)                          # every level's record fetched once: nothing popped was walked again


def test_tie_across_leaves_entry_at_the_limit_is_kept(dll):
    """Two triangles in two leaves, both at distance exactly 2 from the query. The right leaf's box reaches nearer (1) than its
    triangle, so the walk goes right, stacks the left leaf with key 4 and finds primitive 1 at d2 = 4 = the stacked key. Primitive 0
    wins the tie by its index, which only a pop that keeps an entry AT the limit (key <= best, not <) gets to see."""
    from oracle import NODEF
    tris = np.array([[-2, -1, -1, -2, 1, -1, -2, 0, 1], [2, -1, -1, 2, 1, -1, 2, 0, 1]], dtype=np.float32)
    nodes = np.zeros(3, dtype=NODEF)
    nodes[0]["bounds"], nodes[0]["index"] = [-2, 2, -1, 1, -1, 1], 1 << 4
    nodes[1]["bounds"], nodes[1]["index"] = [-2, -2, -1, 1, -1, 1], (0 << 4) | 1
    nodes[2]["bounds"], nodes[2]["index"] = [1, 2, -1, 1, -1, 1], (1 << 4) | 1
    prims = precompute(tris, np.float32)
    q = np.array([[0, 0, 0, np.inf]], dtype=np.float32)
    d2, bi = host_brute(dll, prims, q, 0)
    assert d2[0] == 4 and bi[0] == 0
    assert (host_eval(dll, prims, np.repeat(q, 2, axis=0), [0, 1], 0) == 4).all()
    hits, cnt = host_walk(dll, nodes["bounds"], nodes["index"], prims, q, 0)
    assert hits["prim"][0] == 0 and hits["t"][0] == 2
    assert list(cnt) == [1, 2, 2]                             # one record, both leaves, both triangles
