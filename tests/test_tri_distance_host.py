"""CPU: the TEXT of the triangle-distance kernel (bvh_amd/csrc/tri_distance_body.inc + nearest_walk.inc + tri_intersect_body.inc +
trace_device.h) compiled for the host by tests/cpp/tri_distance_body_host.cpp. The pair distance, float and double, on hand cases
(vertex / face, skew and parallel edges, coplanar pairs, an edge through a face's interior, touching and identical triangles,
segments and points on either side) and on 4,000 random pairs against a float64 restatement in numpy; its agreement with the pair
test of the intersection query; the walk over the golden trees against a brute force over the same function; a scene on which the
arithmetic is exact; point queries against the closest-point harness; invalid queries; finite max_distance. The device's records must
equal this harness's bit for bit (tests/test_gpu_tri_distance.py).

The float64 restatement (ref_dist64) shares no step with the kernel: the distance of two triangles is the smallest of the 9 segment /
segment distances (each the smaller of the interior critical point of its 2 x 2 system and the four end / segment distances), the 6
vertex / triangle distances (the full point-to-solid-triangle distance), and, for every edge whose ends lie strictly on both sides
of the other triangle's plane, the distance from the crossing point to that triangle (0 when the edge goes through it, continuous
when it passes beside).

TOL is 4 x the largest |t - t64| / scale measured over the 4,000 random pairs of random_pairs() (scale = the largest absolute
coordinate of the pair): float32 2.52e-6 -> 1.01e-5, float64 2.11e-14 -> 8.5e-14. The random set holds generic pairs, pairs of unit
size ~4,000 units from the origin, thin triangles, segments, points, and pairs moved into contact. The largest residuals (20 and 95
eps) are all of one kind: a SEGMENT through a triangle's interior, where the pair test does not apply and the 0 is rebuilt from the
crossing point of the segment with the triangle's computed plane, whose normal carries the cancellation of a cross product; the
99.9th percentile is 5.2e-7 / 3.7e-15 and a pair with area on both sides stays below 1.6e-7 / 4.4e-15.
Triangles collinear UP TO ROUNDING (a normal of rounding noise, yet not zero) are kept out of that set and have a test of their
own: the pair test of the intersection query answers for them from the signs its roundings give (include/bvh_amd.h says so), and
where it accepts such a pair the distance is 0 by contract, whatever the float64 distance of the two slivers is."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tri_intersect_ref as R
from conftest import ROOT
from test_closest_point_host import HITD, HITF, INVALID, _p, precompute
from test_closest_point_host import compile_harness as compile_closest, host_walk as closest_walk
from test_sphere_cast_host import _dot, _seg_dist, dist64

HARNESS = os.path.join(ROOT, "tests", "cpp", "tri_distance_body_host.cpp")
TOL = {np.float32: 1.01e-5, np.float64: 8.5e-14}                # 4 x the measured |t - t64| / scale (module docstring)
DTYPES = [np.float32, np.float64]
SCENES = ["cornell", "soup2k", "terrain2k", "soup2k_f64"]


def compile_harness(out_dir):
    out = os.path.join(str(out_dir), "libtri_distance_body_host.so")
    cmd = ["g++", "-std=c++20", "-O1", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-strict-aliasing", "-Wall", "-Wextra", "-Wno-unused-parameter",
           "-Wno-unknown-pragmas", "-Werror", "-shared", "-fPIC", "-pthread", HARNESS, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    dll = C.CDLL(out)
    P, Z, I, U, D = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_double
    dll.tri_distance_host_pairs.restype = None
    dll.tri_distance_host_pairs.argtypes = [I, P, P, Z, P]
    dll.tri_distance_host_walk.restype = I
    dll.tri_distance_host_walk.argtypes = [I, P, U, P, P, P, Z, D, P, P, I, U, I, P, P, P]
    dll.tri_distance_host_brute.restype = None
    dll.tri_distance_host_brute.argtypes = [I, P, P, Z, P, Z, D, P, P, P, P, I]
    return dll


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return compile_harness(tmp_path_factory.mktemp("tri_distance"))


def host_pairs(dll, queries, tris):
    """The pair distance on row k of each (n, 9) array: (t, u, v, s, w, the pair test's verdict)."""
    dt = queries.dtype
    queries, tris = np.ascontiguousarray(queries).reshape(-1, 9), np.ascontiguousarray(tris, dtype=dt).reshape(-1, 9)
    out = np.zeros((len(queries), 6), dtype=dt)
    dll.tri_distance_host_pairs(int(dt == np.float64), _p(queries), _p(tris), len(queries), _p(out))
    return np.sqrt(out[:, 0]), out[:, 1], out[:, 2], out[:, 3], out[:, 4], out[:, 5] == 1


def _limits(tree, max_distance):
    return None if np.isscalar(max_distance) else np.ascontiguousarray(max_distance, dtype=tree.dtype)


def host_walk(dll, tree, queries, max_distance=np.inf, order=None, original_ids=False, deep_cap=0, threads=4):
    """The kernel's walk over a tri_intersect_ref.TriTree: (hit records, (n, 2) query barycentrics, counters {pairs, triangles, leaves}).
    max_distance: a float, or one per query."""
    q = R._aligned(np.ascontiguousarray(np.asarray(queries).reshape(-1, 9), dtype=tree.dtype))
    lim = _limits(tree, max_distance)
    hits = np.zeros(len(q), dtype=HITD if tree.double else HITF)
    uv = np.full((len(q), 2), 7, dtype=tree.dtype)
    cnt = np.zeros(3, dtype=np.uint64)
    order = None if order is None else np.ascontiguousarray(order, dtype=np.uint32)
    assert dll.tri_distance_host_walk(int(tree.double), _p(tree.pairs), tree.root, _p(tree.tris), _p(tree.ids), _p(q), len(q),
                                      float(max_distance) if lim is None else 0.0, _p(lim), _p(order), int(original_ids), deep_cap, threads, _p(hits), _p(uv),
                                      _p(cnt)) == 0
    return hits, uv, cnt


def host_brute(dll, tree, queries, max_distance=np.inf, threads=8):
    """Every query against every triangle with the same pair distance: (records, query barycentrics, the runner-up's distance)."""
    q = np.ascontiguousarray(np.asarray(queries).reshape(-1, 9), dtype=tree.dtype)
    lim = _limits(tree, max_distance)
    hits = np.zeros(len(q), dtype=HITD if tree.double else HITF)
    uv = np.zeros((len(q), 2), dtype=tree.dtype)
    second = np.zeros(len(q), dtype=tree.dtype)
    dll.tri_distance_host_brute(int(tree.double), _p(tree.tris), _p(tree.ids), tree.n, _p(q), len(q), float(max_distance) if lim is None else 0.0, _p(lim),
                                _p(hits), _p(uv), _p(second), threads)
    return hits, uv, np.sqrt(second.astype(np.float64))


# ---- float64 restatement, vectorised over N (query triangle, tree triangle) rows ------------------------------------------------------
def _seg_seg64(p1, q1, p2, q2):
    d1, d2, r = q1 - p1, q2 - p2, p1 - p2
    a, e, b, c, f = _dot(d1, d1), _dot(d2, d2), _dot(d1, d2), _dot(d1, r), _dot(d2, r)
    den = a * e - b * b
    ok = den > 1e-12 * a * e
    sden = np.where(ok, den, 1.0)
    s, t = (b * f - c * e) / sden, (a * f - b * c) / sden
    ok &= (s >= 0) & (s <= 1) & (t >= 0) & (t <= 1)
    inner = np.linalg.norm(r + s[:, None] * d1 - t[:, None] * d2, axis=1)
    ends = np.minimum(np.minimum(_seg_dist(p1, p2, q2), _seg_dist(q1, p2, q2)), np.minimum(_seg_dist(p2, p1, q1), _seg_dist(q2, p1, q1)))
    return np.where(ok, np.minimum(inner, ends), ends)


def _crossing64(a, b, tri):
    """Distance from the point where segment a b crosses the plane of `tri` to the triangle (inf where its ends are not strictly on
    both sides)."""
    n = np.cross(tri[:, 3:6] - tri[:, 0:3], tri[:, 6:9] - tri[:, 0:3])
    ha, hb = _dot(a - tri[:, 0:3], n), _dot(b - tri[:, 0:3], n)
    through = ha * hb < 0
    x = np.where(through, ha / np.where(through, ha - hb, 1.0), 0.0)
    return np.where(through, dist64(tri, a + x[:, None] * (b - a)), np.inf)


def ref_dist64(q, t):
    """float64 distance between the triangles q and t, (N, 9) each (module docstring)."""
    q, t = np.asarray(q, np.float64).reshape(-1, 9), np.asarray(t, np.float64).reshape(-1, 9)
    best = np.full(len(q), np.inf)
    for i in range(3):
        qa, qb = q[:, 3 * i:3 * i + 3], q[:, 3 * ((i + 1) % 3):3 * ((i + 1) % 3) + 3]
        best = np.minimum(best, dist64(t, qa))
        best = np.minimum(best, _crossing64(qa, qb, t))
        ta, tb = t[:, 3 * i:3 * i + 3], t[:, 3 * ((i + 1) % 3):3 * ((i + 1) % 3) + 3]
        best = np.minimum(best, dist64(q, ta))
        best = np.minimum(best, _crossing64(ta, tb, q))
        for j in range(3):
            ta, tb = t[:, 3 * j:3 * j + 3], t[:, 3 * ((j + 1) % 3):3 * ((j + 1) % 3) + 3]
            best = np.minimum(best, _seg_seg64(qa, qb, ta, tb))
    return best


def points64(q, t, u, v, s, w):
    """The two points the barycentrics name, float64."""
    q, t = np.asarray(q, np.float64).reshape(-1, 9), np.asarray(t, np.float64).reshape(-1, 9)
    u, v, s, w = (np.asarray(x, np.float64)[:, None] for x in (u, v, s, w))
    pt = t[:, 0:3] + u * (t[:, 3:6] - t[:, 0:3]) + v * (t[:, 6:9] - t[:, 0:3])
    pq = q[:, 0:3] + s * (q[:, 3:6] - q[:, 0:3]) + w * (q[:, 6:9] - q[:, 0:3])
    return pt, pq


def pair_scale(q, t):
    return np.maximum(np.abs(np.asarray(q, np.float64).reshape(-1, 9)).max(axis=1), np.abs(np.asarray(t, np.float64).reshape(-1, 9)).max(axis=1))


def check_pairs(dll, q, t, dtype, what):
    """The harness on rows of (query, tree triangle), cast to dtype: distance against ref_dist64, rebuilt points, barycentric ranges,
    t == 0 wherever the pair test accepts. Returns (t, u, v, s, w, accepted, largest |t - t64| / scale)."""
    q, t = np.asarray(q, dtype=dtype).reshape(-1, 9), np.asarray(t, dtype=dtype).reshape(-1, 9)
    d, u, v, s, w, hit = host_pairs(dll, q, t)
    tol, scale = TOL[dtype], pair_scale(q, t)
    assert np.isfinite(d).all() and all(np.isfinite(x).all() for x in (u, v, s, w))
    ref = ref_dist64(q, t)
    err = np.abs(d.astype(np.float64) - ref) / scale
    pt, pq = points64(q, t, u, v, s, w)
    gap = np.abs(np.linalg.norm(pt - pq, axis=1) - d.astype(np.float64)) / scale
    print(f"{what} {np.dtype(dtype).name}: {len(q)} pairs, {int(hit.sum())} intersecting, max |t - t64|/scale {err.max():.3e}, max | |Pt - Pq| - t |/scale {gap.max():.3e}")
    assert (err <= tol).all(), (what, int(np.argmax(err)), err.max())
    assert (gap <= tol).all(), (what, int(np.argmax(gap)), gap.max())
    for a, b in ((u, v), (s, w)):
        assert (a >= -tol).all() and (b >= -tol).all() and (a + b <= 1 + tol).all()
    assert (d[hit] == 0).all()
    return d, u, v, s, w, hit, float(err.max())


def random_pairs(n, dtype, seed=2025, line=False):
    """The random set: query and tree triangles with vertices uniform in a unit cube around centres up to 1.5 apart; every 4th pair
    ~4,000 units from the origin; every 7th triangle thin (c = a + lambda (b - a) + 1e-3 noise), every 13th a segment {a, b, b},
    every 17th a point; every 5th pair pushed together so that it intersects or nearly does. line=True: every 11th triangle
    collinear up to rounding instead (c = a + lambda (b - a), rounded: its normal is rounding noise)."""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    q = rng.uniform(-0.5, 0.5, (n, 3, 3))
    t = rng.uniform(-0.5, 0.5, (n, 3, 3)) + rng.uniform(-1.5, 1.5, (n, 1, 3)) * rng.choice([0.0, 0.3, 1.0], (n, 1, 1))
    for arr, off in ((q, 0), (t, 3)):
        lam = rng.uniform(-0.5, 1.5, (n, 1))
        thin = (k + off) % 7 == 0
        arr[thin, 2] = arr[thin, 0] + lam[thin] * (arr[thin, 1] - arr[thin, 0]) + 1e-3 * rng.uniform(-1, 1, (int(thin.sum()), 3))
        if line:
            on = (k + off) % 11 == 0
            arr[on, 2] = arr[on, 0] + lam[on] * (arr[on, 1] - arr[on, 0])
        seg, point = (k + off) % 13 == 0, (k + off) % 17 == 0
        arr[seg, 2] = arr[seg, 1]
        arr[point, 1], arr[point, 2] = arr[point, 0], arr[point, 0]
    close = k % 5 == 0
    t[close] += (q[close].mean(axis=1) - t[close].mean(axis=1))[:, None, :] * rng.uniform(0.7, 1.0, (int(close.sum()), 1, 1))
    far = k % 4 == 0
    shift = rng.uniform(-4000, 4000, (n, 1, 3))
    q[far] += shift[far]
    t[far] += shift[far]
    return q.reshape(n, 9).astype(dtype), t.reshape(n, 9).astype(dtype)


# ---- the pair distance ---------------------------------------------------------------------------------------------------------------
T0 = [0, 0, 0, 4, 0, 0, 0, 4, 0]                                # the tree triangle of the hand cases, in z = 0
HAND = {   # name: (query, tree triangle, expected distance)
    "vertex_face": ([1, 1, 2, 3, 1, 5, 1, 3, 6], T0, 2.0),
    "face_vertex": (T0, [1, 1, -3, 2, 1, -7, 1, 2, -9], 3.0),
    "edge_edge_skew": ([1, -3, 1, 1, 7, 1, 1, 2, 9], [-5, 1, 0, 9, 1, 0, 2, 1, -8], 1.0),
    "edge_edge_parallel": ([0, -2, 0, 4, -2, 0, 2, -6, 3], T0, 2.0),
    "coplanar_disjoint": ([5, 5, 0, 7, 5, 0, 5, 7, 0], T0, np.sqrt(18.0)),
    "coplanar_overlapping": ([1, 1, 0, 5, 1, 0, 1, 5, 0], T0, 0.0),
    "coplanar_contained": ([1, 1, 0, 2, 1, 0, 1, 2, 0], T0, 0.0),
    "piercing": ([1, 1, -1, 1, 1, 1, 5, 5, 0], T0, 0.0),
    "touching_at_a_vertex": ([0, 0, 0, -2, 0, 1, 0, -2, 1], T0, 0.0),
    "vertex_on_face": ([1, 1, 0, 1, 1, 3, 2, 2, 3], T0, 0.0),
    "identical": (T0, T0, 0.0),
    "segment_query_above": ([1, 1, 2, 2, 1, 3, 2, 1, 3], T0, 2.0),
    "segment_query_through": ([1, 1, -1, 1, 1, 1, 1, 1, 1], T0, 0.0),
    "segment_tree_through": (T0, [1, 1, -1, 1, 1, 1, 1, 1, -1], 0.0),
    "segment_segment": ([0, 0, 1, 2, 0, 1, 2, 0, 1], [1, -1, 0, 1, 1, 0, 1, 1, 0], 1.0),
    "point_query": ([1, 1, 5, 1, 1, 5, 1, 1, 5], T0, 5.0),
    "point_query_beside": ([7, 0, 4, 7, 0, 4, 7, 0, 4], T0, 5.0),
    "point_tree": (T0, [1, 1, -2, 1, 1, -2, 1, 1, -2], 2.0),
    "point_point": ([1, 2, 3, 1, 2, 3, 1, 2, 3], [1, 2, 7, 1, 2, 7, 1, 2, 7], 4.0),
    "collinear_query": ([0, 0, 3, 1, 1, 3, 3, 3, 3], T0, 3.0),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(HAND))
def test_hand_cases(dll, dtype, name):
    q, t, want = HAND[name]
    # each case also with the vertices of both triangles rotated and reversed: the answer does not depend on the labelling
    perms = [[0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1], [2, 1, 0], [1, 0, 2]]
    qq = np.array([np.asarray(q, np.float64).reshape(3, 3)[p].reshape(9) for p in perms for _ in perms])
    tt = np.array([np.asarray(t, np.float64).reshape(3, 3)[p].reshape(9) for _ in perms for p in perms])
    d, u, v, s, w, hit, _ = check_pairs(dll, qq, tt, dtype, name)
    assert (np.abs(d - want) <= 8 * np.finfo(dtype).eps * 8).all(), (name, d)
    assert abs(ref_dist64(qq[:1], tt[:1])[0] - want) <= 1e-12
    if want == 0 and not name.startswith("segment"):
        assert hit.all() and (d == 0).all()                    # the pair test decides: exactly 0
    if name.startswith("segment") and want == 0:
        assert not hit.any()                                   # a segment through a face: the pair test refuses it, the crossing candidate finds it


@pytest.mark.parametrize("dtype", DTYPES)
def test_random_pairs(dll, dtype):
    q, t = random_pairs(4000, dtype)
    d, u, v, s, w, hit, worst = check_pairs(dll, q, t, dtype, "random")
    assert 100 < hit.sum() < 2000 and (d > 0).sum() > 2000
    assert worst >= TOL[dtype] / 16                            # the tolerance is the measured one, not a loose guess
    # symmetric in its arguments up to the tolerance (the roles differ in the local frame's origin only), barycentrics swapped
    d2, u2, v2, s2, w2, hit2 = host_pairs(dll, t, q)
    assert (np.abs(d2.astype(np.float64) - d) <= TOL[dtype] * pair_scale(q, t))[~hit & ~hit2].all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_collinear_after_rounding(dll, dtype):
    """Every 11th triangle of either side collinear up to rounding: where the pair test accepts the pair the distance is 0 (the
    contract: the two queries agree), everywhere else it is the float64 distance within the tolerance; never a NaN."""
    q, t = random_pairs(4000, dtype, seed=2026, line=True)
    d, u, v, s, w, hit = host_pairs(dll, q, t)
    assert np.isfinite(d).all() and all(np.isfinite(x).all() for x in (u, v, s, w)) and (d[hit] == 0).all()
    err = np.abs(d.astype(np.float64) - ref_dist64(q, t)) / pair_scale(q, t)
    k = np.arange(len(q))
    sliver = (k % 11 == 0) | ((k + 3) % 11 == 0)
    print(f"collinear {np.dtype(dtype).name}: accepted sliver pairs {int((hit & sliver).sum())}, of them off by more than the tolerance {int((hit & sliver & (err > TOL[dtype])).sum())}")
    assert (err <= TOL[dtype])[~(hit & sliver)].all(), err[~(hit & sliver)].max()


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_exactly_where_the_pair_test_intersects_on_the_lattice(dll, dtype):
    """Quarter-integer lattice coordinates: the pair test's determinants are exact, so it IS the exact answer for triangles with area;
    the distance is 0 for exactly those pairs (a pair that is apart is apart by far more than the arithmetic's error)."""
    lat = R.lattice_tris()
    n = np.cross(lat[:, 1] - lat[:, 0], lat[:, 2] - lat[:, 0])
    lat = lat[(n != 0).any(axis=1)]                            # (a triangle without area intersects nothing in the pair test, yet can touch)
    ref = R.sat_matrix(lat, lat)
    t = (lat.reshape(-1, 9) / 4.0).astype(dtype)
    i, j = np.meshgrid(np.arange(len(t)), np.arange(len(t)), indexing="ij")
    d, u, v, s, w, hit = host_pairs(dll, t[i.ravel()], t[j.ravel()])
    assert (hit.reshape(ref.shape) == ref).all()
    assert ((d == 0).reshape(ref.shape) == ref).all()
    assert ref.sum() > 2000 and (~ref).sum() > 50000
    pt, pq = points64(t[i.ravel()], t[j.ravel()], u, v, s, w)
    assert (np.linalg.norm(pt - pq, axis=1)[hit] <= TOL[dtype] * 2.0).all()      # a common point (|coordinate| <= 2)


# ---- the walk --------------------------------------------------------------------------------------------------------------------------
def scene_queries(tris9, n, seed):
    """n query triangles for a scene, each made from one of its triangles T: a copy shrunk about a point well inside T (barycentric
    weights >= 0.15) to 2 .. 20 % of its size, turned by a random rotation and lifted off T's plane by up to 10 % of T's size, either
    way; so most are nearest to T's interior, a good part cross it, and few sit over an edge or vertex that several triangles share
    (an exact tie, which the brute-force comparison has to excuse: so T is never a triangle whose inner 70 % comes within a
    quarter of T's size of another triangle of the scene that shares no vertex with it, by ref_dist64 - cornell has four coincident twins, boxes standing on its
    floor and a light 0.01 below its ceiling - and the kinds that nearly always tie on a mesh are few). Every 256th is 1.5 x T's size and moved by up to
    30 % of the scene's diagonal, every 512th far outside; every 10th is a segment, every 50th a point."""
    t = np.asarray(tris9).reshape(-1, 3, 3).astype(np.float64)
    rng = np.random.default_rng(seed)
    diag = float(np.linalg.norm(t.max(axis=(0, 1)) - t.min(axis=(0, 1))))
    inner = t.mean(axis=1, keepdims=True) + 0.7 * (t - t.mean(axis=1, keepdims=True))
    room = 0.25 * np.linalg.norm(t.max(axis=1) - t.min(axis=1), axis=1)
    near = ((inner.min(axis=1)[:, None, :] - room[:, None, None] <= t.max(axis=1)[None, :, :]) &
            (t.min(axis=1)[None, :, :] <= inner.max(axis=1)[:, None, :] + room[:, None, None])).all(axis=2)
    np.fill_diagonal(near, False)
    i, j = np.nonzero(near)
    apart = ~(t[i][:, :, None, :] == t[j][:, None, :, :]).all(axis=3).any(axis=(1, 2))        # (a mesh neighbour is not a crowd)
    i, j = i[apart], j[apart]
    crowded = np.unique(i[ref_dist64(inner[i].reshape(-1, 9), t[j].reshape(-1, 9)) <= room[i]])
    pick = rng.choice(np.setdiff1d(np.arange(len(t)), crowded), n)
    diag = float(np.linalg.norm(t.max(axis=(0, 1)) - t.min(axis=(0, 1))))
    T = t[pick]
    wgt = 0.15 + 0.55 * rng.dirichlet([1, 1, 1], n)
    anchor = np.einsum("nk,nkc->nc", wgt, T)[:, None, :]
    size = np.linalg.norm(T.max(axis=1) - T.min(axis=1), axis=1)[:, None, None]
    rot = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
    shape = np.einsum("nvc,ndc->nvd", T - T.mean(axis=1, keepdims=True), rot)
    nrm = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    q = anchor + shape * rng.uniform(0.02, 0.2, (n, 1, 1)) + (nrm * rng.uniform(-0.1, 0.1, (n, 1)))[:, None, :] * size
    big = np.arange(n) % 256 == 3
    q[big] = (T[big] - T[big].mean(axis=1, keepdims=True)) * 1.5 + anchor[big] + 0.3 * diag * rng.uniform(-1, 1, (int(big.sum()), 1, 3))
    q[5::512] += 10 * diag
    q[::10, 2] = q[::10, 1]
    q[::50, 1], q[::50, 2] = q[::50, 0], q[::50, 0]
    return np.ascontiguousarray(q.reshape(n, 9).astype(np.asarray(tris9).dtype))


def record_tris(tree, hits):
    """The tree triangle each record names (BVH-order prim; row 0 for a miss)."""
    hit = hits["prim"] != INVALID
    return tree.ordered_tris()[np.where(hit, hits["prim"], 0).astype(np.int64)], hit


@pytest.fixture(scope="module")
def golden(dll):
    """Per golden scene, once: (tree, queries, walk records, walk query barycentrics, counters, brute records, brute barycentrics,
    runner-up distance)."""
    out = {}
    for scene in SCENES:
        tree = R.golden_tree(scene, "parallel_high")
        q = scene_queries(tree.tris, 2048, 31)
        hits, uv, cnt = host_walk(dll, tree, q, threads=8)
        brute, buv, second = host_brute(dll, tree, q)
        for a in (q, hits, uv, brute, buv, second):
            a.setflags(write=False)
        out[scene] = (tree, q, hits, uv, cnt, brute, buv, second)
    return out


@pytest.mark.parametrize("scene", SCENES)
def test_walk_against_brute_force(dll, golden, scene):
    tree, q, hits, uv, cnt, brute, buv, second = golden[scene]
    dt = tree.dtype.type
    tris, hit = record_tris(tree, hits)
    assert hit.all() and (brute["prim"] != INVALID).all()      # max_distance = inf: every query finds something
    scale = np.maximum(pair_scale(q, tris), pair_scale(q, record_tris(tree, brute)[0]))
    tol = TOL[dt] * scale
    gap = np.abs(hits["t"].astype(np.float64) - brute["t"].astype(np.float64))
    excused = second - brute["t"].astype(np.float64) <= tol    # the runner-up is no farther than the tolerance: either may be reported
    same = hits["prim"] == brute["prim"]
    print(f"{scene}: zero distances {int((hits['t'] == 0).sum())}/{len(q)}, records equal {int(same.sum())}, excused {int(excused.sum())}, "
          f"max |t - t_brute|/scale {(gap / scale).max():.3e}, triangles fetched {int(cnt[1])} of {len(q) * tree.n}")
    assert (gap <= tol).all()
    assert excused.mean() <= 0.02, excused.mean()
    assert (same | excused).all(), np.flatnonzero(~same & ~excused)[:8]
    assert 50 < (hits["t"] == 0).sum() < len(q) - 200 and cnt[0] > 0 and 0 < cnt[1] < len(q) * tree.n / 4 and cnt[2] > 0
    # the record's distance is that of the two points it names, which lie in their triangles; and it is the f64 distance of ITS pair
    pt, pq = points64(q, tris, hits["u"], hits["v"], uv[:, 0], uv[:, 1])
    assert (np.abs(np.linalg.norm(pt - pq, axis=1) - hits["t"]) <= tol).all()
    assert (np.abs(ref_dist64(q, tris) - hits["t"]) <= tol).all()
    for a, b in ((hits["u"], hits["v"]), (uv[:, 0], uv[:, 1])):
        assert (a >= -TOL[dt]).all() and (b >= -TOL[dt]).all() and (a + b <= 1 + TOL[dt]).all()
    # the reading order changes nothing; original ids map prim only
    perm = np.random.default_rng(9).permutation(len(q)).astype(np.uint32)
    hp, up, cp = host_walk(dll, tree, q, order=perm)
    assert hp.tobytes() == hits.tobytes() and up.tobytes() == uv.tobytes() and (cp == cnt).all()
    ho, uo, _ = host_walk(dll, tree, q, original_ids=True)
    assert (ho["prim"] == tree.ids[hits["prim"]]).all() and uo.tobytes() == uv.tobytes()
    for f in ("t", "u", "v"):
        assert ho[f].tobytes() == hits[f].tobytes()


@pytest.mark.parametrize("scene", ["soup2k", "soup2k_f64"])
def test_zero_for_every_intersecting_pair(dll, golden, scene):
    """t == 0 for every query whose triangle intersects some triangle of the tree by the intersection query's own pair test."""
    tree, q, hits, *_ = golden[scene]
    tdll = R.compile_harness(os.path.dirname(dll._name))
    crossing = R.pair_matrix(tdll, q, tree.ordered_tris()).any(axis=1)
    assert crossing.sum() > 50 and (hits["t"][crossing] == 0).all()


@pytest.mark.parametrize("scene", ["soup2k", "terrain2k"])
def test_finite_max_distance(dll, golden, scene):
    """A finite max_distance keeps a subset of the unbounded hits, with identical records; the others are the miss record. A scalar
    is the array of that scalar."""
    tree, q, hits, uv, *_ = golden[scene]
    dt = tree.dtype.type
    lim = dt(np.median(hits["t"][hits["t"] > 0]))
    h1, u1, c1 = host_walk(dll, tree, q, float(lim))
    h2, u2, c2 = host_walk(dll, tree, q, np.full(len(q), lim, dtype=dt))
    assert h1.tobytes() == h2.tobytes() and u1.tobytes() == u2.tobytes() and (c1 == c2).all()
    # (the walk compares SQUARED distances with lim^2, the record holds the rounded root: a t within an ulp of lim may fall either way)
    keep, drop = hits["t"] < lim * dt(1 - 1e-6), hits["t"] > lim * dt(1 + 1e-6)
    assert 200 < keep.sum() and 200 < drop.sum() and keep.sum() + drop.sum() >= len(q) - 4
    assert h1[keep].tobytes() == hits[keep].tobytes() and u1[keep].tobytes() == uv[keep].tobytes()
    miss = h1[drop]
    assert (miss["prim"] == INVALID).all() and (miss["t"] == lim).all() and (miss["u"] == 0).all() and (miss["v"] == 0).all() and (u1[drop] == 0).all()
    either = ~keep & ~drop
    assert all(h1[k:k + 1].tobytes() == hits[k:k + 1].tobytes() or h1["prim"][k] == INVALID for k in np.flatnonzero(either))
    # one max_distance per query
    per = np.where(np.arange(len(q)) % 2 == 0, lim, dt(np.inf)).astype(dt)
    h3, u3, _ = host_walk(dll, tree, q, per)
    odd = np.arange(len(q)) % 2 == 1
    assert h3[odd].tobytes() == hits[odd].tobytes() and h3[~odd].tobytes() == h1[~odd].tobytes() and u3[~odd].tobytes() == u1[~odd].tobytes()


def test_invalid_queries(dll, golden):
    tree, q, hits, uv, *_ = golden["soup2k"]
    q = q[:12].copy()
    lim = np.full(12, np.inf, dtype=np.float32)
    q[1, 4], q[2, 0], q[3, 8] = np.nan, np.nan, np.nan
    lim[4], lim[5], lim[6] = np.nan, -1.0, -np.inf
    lim[7] = 0.0                                               # max_distance 0 is legal: only intersecting triangles
    h, u, cnt = host_walk(dll, tree, q, lim, threads=1)
    bad = np.array([1, 2, 3, 4, 5, 6])
    assert (h["prim"][bad] == INVALID).all() and (h["u"][bad] == 0).all() and (h["v"][bad] == 0).all() and (u[bad] == 0).all()
    assert h["t"][bad].tobytes() == lim[bad].tobytes()         # the max_distance's bits, NaN included
    good = np.array([0, 8, 9, 10, 11])
    assert h[good].tobytes() == hits[good].tobytes()
    assert (h["prim"][7] == INVALID and h["t"][7] == 0) or h[7:8].tobytes() == hits[7:8].tobytes()
    hb, ub, _ = host_brute(dll, tree, q, lim)
    assert (hb["prim"][bad] == INVALID).all() and hb["t"][bad].tobytes() == lim[bad].tobytes()


def exact_scene(orc):
    """Unit squares (two triangles each) on an 8 x 8 grid in the planes z = 0, 2, 4, 6, and 2,048 axis-aligned right triangles with
    legs of 1/4, 1/2 or 1 in planes z = k / 4, every coordinate a multiple of 1/4 in [-3, 11] (every 9th a segment along an axis):
    every edge vector, Gram determinant and its reciprocal is a power of two or a small multiple, every parameter a dyadic rational
    and every squared distance a multiple of 1/16 below 2^10, so the pair distance is computed without rounding. Queries over the grid
    tie between the two triangles of a square, or among up to eight triangles around a grid point."""
    tris = []
    for z in (0.0, 2.0, 4.0, 6.0):
        for x in range(8):
            for y in range(8):
                tris.append([x, y, z, x + 1, y, z, x + 1, y + 1, z])
                tris.append([x, y, z, x + 1, y + 1, z, x, y + 1, z])
    tree = R.built_tree(orc, np.array(tris, dtype=np.float32), np.float32)
    rng = np.random.default_rng(41)
    n = 2048
    o = rng.integers(-12, 45, (n, 3)) / 4.0
    o[:, 2] = rng.integers(-8, 33, n) / 4.0
    leg = rng.choice([0.25, 0.5, 1.0], (n, 1))
    q = np.concatenate([o, o + leg * [1, 0, 0], o + leg * [0, 1, 0]], axis=1)
    q[::9, 6:9] = q[::9, 3:6]
    return tree, q.astype(np.float32)


def test_walk_equals_brute_force_exactly_on_exact_scene(dll, orc):
    tree, q = exact_scene(orc)
    hits, uv, cnt = host_walk(dll, tree, q)
    brute, buv, second = host_brute(dll, tree, q)
    assert hits.tobytes() == brute.tobytes() and uv.tobytes() == buv.tobytes()          # argmin by (d2, index), ties included
    ties = second == brute["t"]
    assert ties.sum() > 300 and (hits["t"] == 0).sum() > 50 and cnt[1] < len(q) * tree.n / 8
    d64 = ref_dist64(q, record_tris(tree, hits)[0])
    assert (np.abs(d64 - hits["t"]) <= TOL[np.float32] * 11).all()          # (the square root is the one rounding; |coordinate| <= 11)


@pytest.mark.parametrize("scene", ["cornell", "soup2k_f64"])
def test_point_queries_agree_with_closest_points(dll, golden, scene, tmp_path_factory):
    """{p, p, p}: the distance is closest_points' within the tolerance (two different evaluation orders of one distance)."""
    tree = golden[scene][0]
    dt = tree.dtype.type
    cdll = compile_closest(tmp_path_factory.mktemp("closest_for_tri_distance"))
    rng = np.random.default_rng(6)
    pts = tree.tris.reshape(-1, 3)
    lo, hi = pts.min(axis=0).astype(np.float64), pts.max(axis=0).astype(np.float64)
    p = (lo + rng.uniform(-0.2, 1.2, (1024, 3)) * (hi - lo)).astype(dt)
    hits, uv, _ = host_walk(dll, tree, np.tile(p, (1, 3)))
    queries4 = np.concatenate([p, np.full((len(p), 1), np.inf, dtype=dt)], axis=1)
    chits, _ = closest_walk(cdll, tree.bounds, tree.index, precompute(tree.ordered_tris(), dt), queries4, 0, threads=4)
    scale = np.maximum(np.abs(p).max(axis=1), np.abs(pts).max())
    assert (np.abs(hits["t"].astype(np.float64) - chits["t"].astype(np.float64)) <= TOL[dt] * scale).all()
    # (a point over an edge two triangles share ties; the two functions round such a tie differently)
    assert (hits["prim"] == chits["prim"]).mean() > 0.9 and (uv == 0).all()


@pytest.mark.parametrize("depth", [65, 300])
def test_deep_chain(dll, depth):
    """A chain tree deeper than 64 levels: the Deep walk's HBM spill; the walk equals the brute force byte for byte."""
    tree = R.chain_tree(depth, stacked=True)
    q = chain_queries(depth, 64)
    hits, uv, cnt = host_walk(dll, tree, q, deep_cap=depth - 64 + 1)
    brute, buv, _ = host_brute(dll, tree, q)
    assert hits.tobytes() == brute.tobytes() and uv.tobytes() == buv.tobytes()
    assert (hits["t"][::4] == 0).all() and (hits["t"] > 0).sum() > 16 and len(set(hits["prim"].tolist())) > 8


def chain_queries(depth, n):
    """Over tri_intersect_ref.chain_tree: every 4th query the sliver that crosses every level (distance 0, the lowest index wins), the
    others small triangles beside the chain at quarter coordinates, spread along it."""
    import query_slices as qs
    rng = np.random.default_rng(depth)
    q = R.chain_queries(depth, n)
    cx = qs.chain_base(depth) - rng.integers(0, 4 * depth, n) / 4.0
    cy = rng.choice([-3.0, -2.5, 2.25, 3.5], n)
    small = np.stack([cx, cy, np.zeros(n), cx + 0.25, cy, np.zeros(n), cx, cy + 0.25, 0.25 + np.zeros(n)], axis=1).astype(np.float32)
    keep = np.arange(n) % 4 == 0
    return np.ascontiguousarray(np.where(keep[:, None], q, small))


def test_one_triangle_tree(dll):
    from oracle import NODEF
    tri = np.array([T0], dtype=np.float32)
    nodes = np.zeros(1, dtype=NODEF)
    nodes[0]["bounds"], nodes[0]["index"] = [0, 4, 0, 4, 0, 0], (0 << 4) | 1
    tree = R.TriTree(nodes["bounds"], nodes["index"], tri, np.zeros(1, dtype=np.uint32))
    q = np.array([HAND["vertex_face"][0], HAND["piercing"][0], HAND["point_query"][0]], dtype=np.float32)
    hits, uv, cnt = host_walk(dll, tree, q, threads=1)
    assert (hits["prim"] == 0).all() and hits["t"].tolist() == [2.0, 0.0, 5.0] and cnt[1] == 3 and cnt[0] == 0
    h, u, _ = host_walk(dll, tree, q, 1.0, threads=1)
    assert h["prim"].tolist() == [INVALID, 0, INVALID] and h["t"].tolist() == [1.0, 0.0, 1.0]


def test_symbols_are_declared_and_exported():
    import re
    from bvh_amd import _lib, build
    build.build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "bvh_amd.h")).read()
    declared = set(re.findall(r"BVH_AMD_API[^;]*?\b(bvh\w+)\s*\(", header))
    want = {"bvh3f_tri_distance", "bvh3d_tri_distance"}
    assert {n for n in declared if "tri_distance" in n} == want and want <= set(_lib.exported_symbols())
    for s in ("2f", "2d"):
        assert not hasattr(lib, f"bvh{s}_tri_distance")
    import bvh_amd
    assert callable(bvh_amd.tri_distance)
