"""CPU: the TEXT of the sphere-cast kernel (bvh_amd/csrc/sphere_cast_body.inc + nearest_walk.inc + trace_device.h) compiled for the
host by tests/cpp/sphere_cast_body_host.cpp. The sweep test, float and double, on crafted cases (head-on contact with the face, each
edge and each vertex; a start inside the plane slab; initial overlap; dir = 0; r = 0; tmax around the contact; dir parallel to an
edge; degenerate triangles; triangles collinear up to rounding; sphere leaves) and on 4,000 random pairs against a float64
restatement in numpy, itself checked against bisection of the convex function t -> dist(c(t), triangle); the walk over the golden
trees against a brute force over the same function. The device's records must equal this harness's bit for bit
(tests/test_gpu_sphere_cast.py).

What is asserted of a reported hit is its RESIDUAL, not its t (a grazing root moves by sqrt(eps) under rounding):
|dist64(c(t), prim) - r| <= TOL * scale, or dist64 <= r + TOL * scale when t == tmin, and no penetration deeper than TOL * scale
before t (so an exit from the grown triangle can never pass for a contact); scale = the largest coordinate magnitude involved.
TOL is 4 x the largest residual measured over the random set below (float32 2.66e-7 -> 1.07e-6, float64 4.75e-16 -> 1.9e-15:
about two roundings of a coordinate).

Mutants, each made once by hand in sphere_cast_body.inc and run against this file:
  * the face accepted without the distance guard (`<= rs * rs` made always true): test_random_pairs and
    test_collinear_after_rounding fail in both types (contacts with the noise plane of a triangle collinear up to rounding);
  * the boxes grown by 0 instead of r: every test_walk_golden case and test_walk_equals_brute_force_exactly_on_dyadic_scene fail;
  * the face tested without the approach condition s (n.dir) < 0: NOTHING fails, and nothing can. The root then offered is where
    a centre inside the slab leaves it over the triangle; below that height over the triangle it is inside the grown triangle, so it
    either started inside (the start candidate, t = tmin) or came in through an edge cylinder or a vertex ball at an earlier t, and
    the minimum over the candidates takes that one. In this decomposition the condition saves the face's arithmetic and decides no
    record; test_inside_slab_moving_away pins the behaviour (the exit is never reported), not the condition."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_kernel_body_host import _aligned, pair_records
from test_closest_point_host import (DEGENERATE, GOLDEN_SCENES, HITD, HITF, INVALID, TRI, A, B, Cv, NRM, CEN, _p, chain_tree, golden_scene,
                                     precompute)

HARNESS = os.path.join(ROOT, "tests", "cpp", "sphere_cast_body_host.cpp")
TOL = {np.float32: 1.07e-6, np.float64: 1.9e-15}               # 4 x the measured residual / scale (module docstring)


def compile_harness(out_dir):
    out = os.path.join(str(out_dir), "libsphere_cast_body_host.so")
    cmd = ["g++", "-std=c++20", "-O1", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-strict-aliasing", "-Wall", "-Wextra", "-Wno-unused-parameter",
           "-Wno-unknown-pragmas", "-Werror", "-shared", "-fPIC", "-pthread", HARNESS, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    dll = C.CDLL(out)
    P, Z, I, U, D = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_double
    dll.sphere_cast_host_pairs.argtypes = [I, I, P, P, P, Z, P]
    dll.sphere_cast_host_walk.restype = I
    dll.sphere_cast_host_walk.argtypes = [I, I, I, P, U, P, P, Z, D, P, P, P, U, I, P, P]
    dll.sphere_cast_host_brute.argtypes = [I, I, P, Z, P, Z, D, P, P, I, P]
    return dll


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return compile_harness(tmp_path_factory.mktemp("sphere_cast"))


def host_pairs(dll, prims, rays, radii, leaf=0):
    """The sweep test on row k of each array: (hit mask, t, u, v)."""
    dt = prims.dtype
    prims, rays, radii = (np.ascontiguousarray(x, dtype=dt) for x in (prims, rays, radii))
    out = np.zeros((len(rays), 4), dtype=dt)
    dll.sphere_cast_host_pairs(int(dt == np.float64), leaf, _p(prims), _p(rays), _p(radii), len(rays), _p(out))
    return out[:, 0] == 1, out[:, 1], out[:, 2], out[:, 3]


def host_walk(dll, bounds6, index, prims, rays, radius, leaf, robust=False, order=None, prim_ids=None, deep_cap=0, threads=2):
    """The kernel's walk for every ray: (hit records, counters {pairs, tests, leaves}). radius: a float, or one per ray."""
    double = bounds6.dtype == np.float64
    pairs = _aligned(pair_records(bounds6, index))
    prims = _aligned(np.ascontiguousarray(prims))
    rays = _aligned(np.ascontiguousarray(rays))
    radii = None if np.isscalar(radius) else np.ascontiguousarray(radius, dtype=prims.dtype)
    hits = np.zeros(len(rays), dtype=HITD if double else HITF)
    cnt = np.zeros(3, dtype=np.uint64)
    order = None if order is None else np.ascontiguousarray(order, dtype=np.uint32)
    prim_ids = None if prim_ids is None else np.ascontiguousarray(prim_ids, dtype=np.uint32)
    assert dll.sphere_cast_host_walk(int(double), leaf, int(robust), _p(pairs), int(index[0]) & 0xFFFFFFFF, _p(prims), _p(rays), len(rays),
                                     float(radius) if radii is None else 0.0, _p(radii), _p(order), _p(prim_ids), deep_cap, threads, _p(hits), _p(cnt)) == 0
    return hits, cnt


def host_brute(dll, prims, rays, radius, leaf, threads=4):
    double = prims.dtype == np.float64
    prims, rays = np.ascontiguousarray(prims), np.ascontiguousarray(rays)
    radii = None if np.isscalar(radius) else np.ascontiguousarray(radius, dtype=prims.dtype)
    hits = np.zeros(len(rays), dtype=HITD if double else HITF)
    tests = C.c_ulonglong(0)
    dll.sphere_cast_host_brute(int(double), leaf, _p(prims), len(prims), _p(rays), len(rays), float(radius) if radii is None else 0.0, _p(radii),
                               _p(hits), threads, C.byref(tests))
    return hits, int(tests.value)


# ---- float64 reference, vectorised over N (triangle, ray, radius) rows ---------------------------------------------------------------
def _dot(a, b):
    return np.einsum("ij,ij->i", a, b)


def _seg_dist(q, a, b):
    ab = b - a
    den = _dot(ab, ab)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(den > 0, _dot(q - a, ab) / np.where(den > 0, den, 1), 0.0)
    w = np.clip(w, 0.0, 1.0)
    return np.linalg.norm(q - (a + w[:, None] * ab), axis=1)


def degenerate64(tri):
    """|n|^2 <= 1e-20 |ab|^2 |ac|^2: such a triangle is its three edges."""
    a, b, c = tri[:, 0:3], tri[:, 3:6], tri[:, 6:9]
    n = np.cross(b - a, c - a)
    return _dot(n, n) <= 1e-20 * _dot(b - a, b - a) * _dot(c - a, c - a)


def dist64(tri, q):
    """float64 distance from q (N, 3) to the solid triangles tri (N, 9): the plane foot when it falls inside, else the nearest edge."""
    tri, q = np.asarray(tri, np.float64), np.asarray(q, np.float64)
    a, b, c = tri[:, 0:3], tri[:, 3:6], tri[:, 6:9]
    best = np.minimum(np.minimum(_seg_dist(q, a, b), _seg_dist(q, a, c)), _seg_dist(q, b, c))
    ab, ac, ap = b - a, c - a, q - a
    abab, acac, abac, apab, apac = _dot(ab, ab), _dot(ac, ac), _dot(ab, ac), _dot(ap, ab), _dot(ap, ac)
    det = abab * acac - abac * abac
    ok = ~degenerate64(tri) & (det > 0)
    sdet = np.where(ok, det, 1.0)
    u, v = (acac * apab - abac * apac) / sdet, (abab * apac - abac * apab) / sdet
    inside = ok & (u >= 0) & (v >= 0) & (u + v <= 1)
    foot = np.linalg.norm(ap - u[:, None] * ab - v[:, None] * ac, axis=1)
    return np.where(inside, np.minimum(best, foot), best)


def _first_root(A_, B_, C_):
    """The smaller root of A t^2 + 2 B t + C = 0 where a centre outside (C > 0) approaches (B < 0), else inf."""
    with np.errstate(all="ignore"):
        disc = B_ * B_ - A_ * C_
        ok = (A_ > 0) & (B_ < 0) & (C_ > 0) & (disc >= 0)
        return np.where(ok, C_ / (np.sqrt(np.where(ok, disc, 0.0)) - B_), np.inf)


def ref_cast(tri, rays, r):
    """The decomposition restated in float64 from the ORIGINAL vertices: first contact t per row (inf: none)."""
    tri, rays, r = np.asarray(tri, np.float64), np.asarray(rays, np.float64), np.asarray(r, np.float64)
    a, b, c = tri[:, 0:3], tri[:, 3:6], tri[:, 6:9]
    org, d, tmin, tmax = rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7]
    c0 = org + tmin[:, None] * d
    best = np.full(len(tri), np.inf)
    with np.errstate(all="ignore"):
        n = np.cross(b - a, c - a)
        nl = np.linalg.norm(n, axis=1)
        g0, nd = _dot(n, c0 - a), _dot(n, d)
        s = np.sign(g0)
        tau = (s * r * nl - g0) / nd
        face = ~degenerate64(tri) & (s * nd < 0) & (tau >= 0)
        cf = c0 + np.where(face, tau, 0.0)[:, None] * d
        ab, ac, ap = b - a, c - a, cf - a
        abab, acac, abac, apab, apac = _dot(ab, ab), _dot(ac, ac), _dot(ab, ac), _dot(ap, ab), _dot(ap, ac)
        det = np.where(face, abab * acac - abac * abac, 1.0)
        u, v = (acac * apab - abac * apac) / det, (abab * apac - abac * apab) / det
        face &= (u >= 0) & (v >= 0) & (u + v <= 1)
        best = np.where(face, tau, best)
        dd = _dot(d, d)
        for p0, p1 in ((a, b), (a, c), (b, c)):
            e, m = p1 - p0, c0 - p0
            ee, me, de = _dot(e, e), _dot(m, e), _dot(d, e)
            t = _first_root(ee * dd - de * de, ee * _dot(m, d) - de * me, ee * (_dot(m, m) - r * r) - me * me)
            w = (me + np.where(np.isfinite(t), t, 0.0) * de) / np.where(ee > 0, ee, 1.0)
            best = np.minimum(best, np.where((ee > 0) & (w >= 0) & (w <= 1), t, np.inf))
        for p0 in (a, b, c):
            m = c0 - p0
            best = np.minimum(best, _first_root(dd, _dot(m, d), _dot(m, m) - r * r))
    t = np.where(dist64(tri, c0) <= r, tmin, tmin + best)
    return np.where(t <= tmax, t, np.inf)


def min_clearance(tri, rays, lo=None, hi=None, iters=90):
    """min over t in [lo, hi] (default [tmin, tmax]) of dist64(c(t)), and its argmin: golden-section search of a convex function."""
    tri, rays = np.asarray(tri, np.float64), np.asarray(rays, np.float64)
    org, d = rays[:, 0:3], rays[:, 3:6]
    lo = rays[:, 6].copy() if lo is None else np.array(lo, np.float64)
    hi = rays[:, 7].copy() if hi is None else np.array(hi, np.float64)
    hi = np.where(np.isfinite(hi), hi, 1e3)                   # (an unbounded ray: far beyond every scene of this file)
    lo0, hi0 = lo.copy(), hi.copy()
    f = lambda t: dist64(tri, org + t[:, None] * d)
    g = (np.sqrt(5.0) - 1) / 2
    for _ in range(iters):
        x1, x2 = hi - g * (hi - lo), lo + g * (hi - lo)
        left = f(x1) <= f(x2)
        hi, lo = np.where(left, x2, hi), np.where(left, lo, x1)
    t = (lo + hi) / 2
    vals, ts = np.stack([f(t), f(lo0), f(hi0)]), np.stack([t, lo0, hi0])
    k = vals.argmin(axis=0)
    return vals.min(axis=0), ts[k, np.arange(len(t))]


def bisect_cast(tri, rays, r):
    """First t in [tmin, tmax] with dist64(c(t)) <= r by bisection between tmin and the argmin of the convex distance (inf: none)."""
    tri, rays, r = np.asarray(tri, np.float64), np.asarray(rays, np.float64), np.asarray(r, np.float64)
    org, d, tmin = rays[:, 0:3], rays[:, 3:6], rays[:, 6]
    f = lambda t: dist64(tri, org + t[:, None] * d)
    fmin, targ = min_clearance(tri, rays)
    lo, hi = tmin.copy(), targ.copy()
    for _ in range(80):
        mid = (lo + hi) / 2
        inside = f(mid) <= r
        hi, lo = np.where(inside, mid, hi), np.where(inside, lo, mid)
    return np.where(f(tmin) <= r, tmin, np.where(fmin <= r, hi, np.inf))


def _scale(tri, rays, t):
    org, d = rays[:, 0:3].astype(np.float64), rays[:, 3:6].astype(np.float64)
    ct = org + np.where(np.isfinite(t), t, 0.0)[:, None] * d
    return np.maximum(np.maximum(np.abs(np.asarray(tri, np.float64)).max(axis=1), np.abs(org).max(axis=1)), np.abs(ct).max(axis=1))


def residuals(tri, rays, r, hit, t):
    """Per row: (residual / scale of a reported hit (0 where none), deepest penetration before t / scale). tri, rays, r as the harness
    got them; everything computed in float64."""
    tri64, rays64, r = np.asarray(tri, np.float64), np.asarray(rays, np.float64), np.asarray(r, np.float64)
    t = np.asarray(t, np.float64)
    tt = np.where(hit, t, rays64[:, 6])
    scale = _scale(tri64, rays64, tt)
    dist = dist64(tri64, rays64[:, 0:3] + tt[:, None] * rays64[:, 3:6])
    at_start = tt == rays64[:, 6]
    res = np.where(at_start, np.maximum(dist - r, 0.0), np.abs(dist - r)) / scale
    before, _ = min_clearance(tri64, rays64, lo=rays64[:, 6], hi=tt, iters=60)
    pen = np.where(at_start, 0.0, np.maximum(r - before, 0.0)) / scale
    return np.where(hit, res, 0.0), np.where(hit, pen, 0.0)


def check_pairs(dll, tri, rays, r, dtype, what, band_cap=0.02):
    """The harness on rows of (original vertices, ray, radius), all already representable in dtype: residuals of the hits, hit / miss
    against ref_cast outside the grazing band. Returns (hit, t, u, v, largest residual / scale)."""
    tri, rays, r = (np.asarray(x, dtype=dtype) for x in (tri, rays, r))
    hit, t, u, v = host_pairs(dll, precompute(tri, dtype), rays, r)
    tol = TOL[dtype]
    res, pen = residuals(tri, rays, r, hit, t)
    print(f"{what} {np.dtype(dtype).name}: hits {int(hit.sum())}/{len(hit)}, max residual/scale {res.max():.3e}, max early penetration/scale {pen.max():.3e}")
    assert (res <= tol).all(), (what, int(np.argmax(res)), res.max())
    assert (pen <= tol).all(), (what, int(np.argmax(pen)), pen.max())
    outside = hit & ((t < rays[:, 6]) | (t > rays[:, 7]))
    assert not outside.any()
    ref_t = ref_cast(tri, rays, r)
    clear, _ = min_clearance(tri, rays)
    band = np.abs(clear - r.astype(np.float64)) <= tol * _scale(tri, rays, np.where(hit, t, rays[:, 6]).astype(np.float64))
    print(f"{what} {np.dtype(dtype).name}: grazing band {int(band.sum())}/{len(band)}, flips outside it {int(((hit != np.isfinite(ref_t)) & ~band).sum())}")
    assert band.mean() <= band_cap, (what, band.mean())
    assert ((hit == np.isfinite(ref_t)) | band).all(), (what, np.flatnonzero((hit != np.isfinite(ref_t)) & ~band)[:8])
    return hit, t, u, v, float(res.max())


def random_pairs(n, dtype, seed=2024):
    """The random set: vertices uniform in [-1, 1]^3, every 7th triangle collinear up to rounding (c = a + lambda (b - a), rounded),
    origins uniform in [-3, 3]^3 aimed at a point of [-1.3, 1.3]^3, |dir| scaled by a factor in [0.2, 2], r and tmax from short lists."""
    rng = np.random.default_rng(seed)
    tri = rng.uniform(-1, 1, (n, 9))
    lam = rng.uniform(-0.5, 1.5, n)
    thin = np.arange(n) % 7 == 0
    tri[thin, 6:9] = tri[thin, 0:3] + lam[thin, None] * (tri[thin, 3:6] - tri[thin, 0:3])
    org = rng.uniform(-3, 3, (n, 3))
    aim = rng.uniform(-1.3, 1.3, (n, 3))
    d = (aim - org) * rng.uniform(0.2, 2.0, (n, 1))
    rays = np.concatenate([org, d, np.zeros((n, 1)), rng.choice([0.5, 1.0, 3.0], (n, 1))], axis=1)
    r = rng.choice([0.0, 0.003, 0.01, 0.1, 0.5], n)
    return tri.astype(dtype), rays.astype(dtype), r.astype(dtype)


def _unit(x):
    return x / np.linalg.norm(x)


def _ray(org, d, tmin=0.0, tmax=10.0):
    return np.concatenate([org, d, [tmin, tmax]])


INTERIOR = 0.2 * A + 0.5 * B + 0.3 * Cv
EDGES = {"ab": (A, B, Cv), "ac": (A, Cv, B), "bc": (B, Cv, A)}
VERTS = {"a": (A, (0.0, 0.0)), "b": (B, (1.0, 0.0)), "c": (Cv, (0.0, 1.0))}


def _out(p0, p1, opp):
    """In the triangle's plane, perpendicular to the edge p0 p1, pointing away from the opposite vertex."""
    e = _unit(p1 - p0)
    w = (p0 + p1) / 2 - opp
    return _unit(w - (w @ e) * e)


def _one(dll, dtype, ray, r, tri=TRI):
    tri = np.asarray(tri, np.float64).astype(dtype)[None]
    ray = np.asarray(ray, np.float64).astype(dtype)[None]
    rr = np.asarray([r], dtype=dtype)
    hit, t, u, v = host_pairs(dll, precompute(tri, dtype), ray, rr)
    ref_t, bis_t = ref_cast(tri, ray, rr)[0], bisect_cast(tri, ray, rr)[0]
    # the restatement against bisection of the convex distance (both float64), unless the path only grazes the grown triangle (r = 0
    # always does: bisection cannot see a set without interior)
    grazes = abs(min_clearance(tri, ray)[0][0] - r) <= 1e-7
    assert grazes or np.isfinite(ref_t) == np.isfinite(bis_t) and (not np.isfinite(ref_t) or abs(ref_t - bis_t) <= 1e-9 * (1 + abs(bis_t))), (ref_t, bis_t)
    if hit[0]:
        res, pen = residuals(tri, ray, rr, hit, t)
        assert res[0] <= TOL[dtype] and pen[0] <= TOL[dtype], (res, pen)
    return bool(hit[0]), float(t[0]), float(u[0]), float(v[0]), float(ref_t)


def _close(dtype, t, ref_t):
    return abs(t - ref_t) <= (2e-5 if dtype == np.float32 else 1e-11) * (1 + abs(ref_t))


DTYPES = [np.float32, np.float64]


@pytest.mark.parametrize("dtype", DTYPES)
def test_head_on_face(dll, dtype):
    hit, t, u, v, ref_t = _one(dll, dtype, _ray(INTERIOR + 2.0 * NRM, -NRM), 0.25)
    assert hit and _close(dtype, t, 1.75) and _close(dtype, ref_t, 1.75)
    assert abs(u - 0.5) <= 1e-5 and abs(v - 0.3) <= 1e-5      # the contact point is INTERIOR = A + 0.5 (B - A) + 0.3 (C - A)
    # from the other side of the plane
    hit, t, u, v, ref_t = _one(dll, dtype, _ray(INTERIOR - 2.0 * NRM, 0.5 * NRM), 0.25)
    assert hit and _close(dtype, t, 3.5) and abs(u - 0.5) <= 1e-5 and abs(v - 0.3) <= 1e-5


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("edge", list(EDGES))
def test_head_on_edge(dll, dtype, edge):
    p0, p1, opp = EDGES[edge]
    mid, out = 0.4 * p0 + 0.6 * p1, _out(p0, p1, opp)
    hit, t, u, v, ref_t = _one(dll, dtype, _ray(mid + 2.0 * out + 0.05 * NRM, -out), 0.25)
    assert hit and _close(dtype, t, ref_t) and 1.7 < t < 1.8
    point = A + u * (B - A) + v * (Cv - A)
    assert np.linalg.norm(point - mid) <= 1e-5                # the contact point is on the edge, at its parameter 0.6
    assert {"ab": v == 0, "ac": u == 0, "bc": abs(u + v - 1) <= 1e-6}[edge]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("vert", list(VERTS))
def test_head_on_vertex(dll, dtype, vert):
    p, uv = VERTS[vert]
    away = _unit(p - CEN)
    hit, t, u, v, ref_t = _one(dll, dtype, _ray(p + 2.0 * away + 0.02 * NRM, -away), 0.25)
    assert hit and _close(dtype, t, ref_t) and (u, v) == uv


@pytest.mark.parametrize("dtype", DTYPES)
def test_inside_slab_moving_away(dll, dtype):
    """A centre that starts inside the slab |n.(c - p0)| <= r beside the triangle and moves away from the plane: it misses, or it
    meets an edge on its way over the triangle. The t at which it LEAVES the slab over the triangle is never reported."""
    r = 0.25
    out = _out(A, B, Cv)
    start = (A + B) / 2 + (r + 0.3) * out + 0.5 * r * NRM
    hit, t, u, v, ref_t = _one(dll, dtype, _ray(start, NRM), r)
    assert not hit and not np.isfinite(ref_t)
    # up and over the triangle: the exit of the slab is at t = 0.5 r / 0.3 over the interior; the edge AB comes first
    d = 0.3 * NRM - 1.5 * out
    hit, t, u, v, ref_t = _one(dll, dtype, _ray(start, d), r)
    t_exit = 0.5 * r / 0.3
    foot = start + t_exit * d
    assert dist64(TRI[None], foot[None])[0] < r + 1e-9 and hit and v == 0 and 0 < u < 1 and t < t_exit - 0.05 and _close(dtype, t, ref_t)
    # along the plane inside the slab, past the triangle: nothing
    hit, *_ = _one(dll, dtype, _ray(start, _unit(B - A) + 0.01 * NRM), r)
    assert not hit


@pytest.mark.parametrize("dtype", DTYPES)
def test_initial_overlap_dir0_r0(dll, dtype):
    for tmin in (0.0, 0.5):
        hit, t, u, v, _ = _one(dll, dtype, _ray(INTERIOR + 0.1 * NRM - tmin * NRM, NRM, tmin, 10.0), 0.25)
        assert hit and t == dtype(tmin) and abs(u - 0.5) <= 1e-5 and abs(v - 0.3) <= 1e-5
    # dir = 0: an overlap test at c(tmin)
    hit, t, *_ = _one(dll, dtype, _ray(INTERIOR + 0.1 * NRM, np.zeros(3), 0.25, 10.0), 0.25)
    assert hit and t == 0.25
    hit, *_ = _one(dll, dtype, _ray(INTERIOR + 0.3 * NRM, np.zeros(3), 0.25, 10.0), 0.25)
    assert not hit
    # r = 0: a ray cast against the closed triangle
    hit, t, u, v, ref_t = _one(dll, dtype, _ray(INTERIOR + 2.0 * NRM, -NRM), 0.0)
    assert hit and _close(dtype, t, 2.0) and abs(u - 0.5) <= 1e-5 and abs(v - 0.3) <= 1e-5
    hit, *_ = _one(dll, dtype, _ray((A + B) / 2 + 0.1 * _out(A, B, Cv) + 2.0 * NRM, -NRM), 0.0)
    assert not hit
    # a negative or NaN radius never touches anything
    for bad in (-0.5, np.nan):
        tri = TRI.astype(dtype)[None]
        hit, *_ = host_pairs(dll, precompute(tri, dtype), _ray(INTERIOR + 0.1 * NRM, NRM).astype(dtype)[None], np.asarray([bad], dtype=dtype))
        assert not hit[0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_tmax_around_contact(dll, dtype):
    ray = _ray(INTERIOR + 2.0 * NRM, -NRM)
    for tmax, want in ((1.7499, False), (1.7501, True), (1.0, False), (np.inf, True)):
        ray[7] = tmax
        hit, t, *_ = _one(dll, dtype, ray, 0.25)
        assert hit == want and (not hit or _close(dtype, t, 1.75))


@pytest.mark.parametrize("dtype", DTYPES)
def test_dir_parallel_to_edge(dll, dtype):
    """Along the line of AB, 0.1 beside it: the cylinder of AB has no root (its leading coefficient is 0 up to rounding), the ball of
    the vertex A is met first."""
    e, out = _unit(B - A), _out(A, B, Cv)
    hit, t, u, v, ref_t = _one(dll, dtype, _ray(A - 2.0 * e + 0.1 * out, e), 0.25)
    assert hit and _close(dtype, t, 2.0 - np.sqrt(0.25 ** 2 - 0.1 ** 2)) and abs(u) <= 1e-5 and v == 0
    tri_axis = np.array([0, 0, 0, 2, 0, 0, 0, 2, 0], np.float64)                          # dir EXACTLY parallel to AB
    hit, t, u, v, ref_t = _one(dll, dtype, _ray(np.array([-3, -0.125, 0.0]), np.array([1.0, 0, 0])), 0.25, tri=tri_axis)
    assert hit and (u, v) == (0.0, 0.0) and _close(dtype, t, ref_t)


DEGENERATE_RAYS = [([0.5, 4.0, 0.25], [0.0, -1.0, 0.0]), ([-3.0, -3.0, -2.5], [1.0, 1.0, 1.0]), ([4.0, 0.5, 0.125], [-1.0, 0.0, 0.0]),
                   ([1.0, 2.0, 7.0], [0.0, 0.0, -1.0]), ([0.5, 0.25, 3.0], [0.0, 0.0, -1.0]), ([5.0, 5.0, 5.0], [1.0, 0.0, 0.0])]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(DEGENERATE))
def test_degenerate_triangles(dll, dtype, name):
    """Coincident or collinear vertices in dyadic coordinates: the triangle behaves as its edges (and their end balls)."""
    rays = np.array([_ray(np.array(org), np.array(d), 0.0, 20.0) for org, d in DEGENERATE_RAYS for _ in range(3)], dtype=dtype)
    r = np.array([0.0, 0.25, 1.0] * len(DEGENERATE_RAYS), dtype=dtype)
    tri = np.repeat(np.asarray(DEGENERATE[name], dtype=dtype)[None], len(rays), axis=0)
    hit, t, u, v = host_pairs(dll, precompute(tri, dtype), rays, r)
    assert np.isfinite(t).all() and np.isfinite(u).all() and np.isfinite(v).all() and hit.any()
    ref_t, bis_t = ref_cast(tri, rays, r), bisect_cast(tri, rays, r)
    grazing = np.abs(min_clearance(tri, rays)[0] - r) <= 1e-5
    assert (np.isfinite(ref_t) == np.isfinite(bis_t))[~grazing].all()
    assert (grazing | (hit == np.isfinite(ref_t))).all(), (name, np.flatnonzero(~grazing & (hit != np.isfinite(ref_t))))
    both = ~grazing & hit
    assert (np.abs(t[both] - ref_t[both]) <= (2e-5 if dtype == np.float32 else 1e-11) * (1 + np.abs(ref_t[both]))).all()
    assert (np.abs(bis_t[both] - ref_t[both]) <= 1e-9 * (1 + np.abs(ref_t[both]))).all()
    res, pen = residuals(tri, rays, r, hit, t)
    assert (res <= TOL[dtype]).all() and (pen <= TOL[dtype]).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_collinear_after_rounding(dll, dtype):
    """c = a + lambda (b - a) rounded to the scalar type: the normal and the face's barycentrics are rounding noise. Every hit must be
    a real contact (residual), and hit / miss must be the three edges' (ref_cast treats such a triangle as its edges)."""
    rng = np.random.default_rng(77)
    n = 1200
    tri = rng.uniform(-1, 1, (n, 9))
    tri[:, 6:9] = tri[:, 0:3] + rng.uniform(-0.5, 1.5, (n, 1)) * (tri[:, 3:6] - tri[:, 0:3])
    tri = tri.astype(dtype)
    _, rays, r = random_pairs(n, dtype, seed=78)
    assert (precompute(tri, dtype)[:, 9:] != 0).any(axis=1).mean() > 0.5      # the case that needs the guard: a normal of rounding noise
    hit, *_ = check_pairs(dll, tri, rays, r, dtype, "collinear")
    assert 50 < hit.sum() < n


@pytest.mark.parametrize("dtype", DTYPES)
def test_random_pairs(dll, dtype):
    tri, rays, r = random_pairs(4000, dtype)
    hit, t, u, v, _ = check_pairs(dll, tri, rays, r, dtype, "random")
    assert 200 < hit.sum() < 3600
    # the restatement against bisection where neither grazes
    ref_t, bis_t = ref_cast(tri, rays, r), bisect_cast(tri, rays, r)
    clear, _ = min_clearance(tri, rays)
    far = np.abs(clear - r) > 1e-6
    assert (np.isfinite(ref_t) == np.isfinite(bis_t))[far].all()
    both = far & np.isfinite(ref_t)
    assert (np.abs(ref_t[both] - bis_t[both]) <= 1e-7).all()
    # (u, v) rebuild a point of the triangle at distance r from c(t) (the contact normal's foot)
    tri64, rays64 = tri.astype(np.float64), rays.astype(np.float64)
    point = tri64[:, 0:3] + u[:, None] * (tri64[:, 3:6] - tri64[:, 0:3]) + v[:, None] * (tri64[:, 6:9] - tri64[:, 0:3])
    ct = rays64[:, 0:3] + t.astype(np.float64)[:, None] * rays64[:, 3:6]
    moving = hit & (t > rays[:, 6])
    gap = np.abs(np.linalg.norm(ct - point, axis=1) - r) / _scale(tri64, rays64, t.astype(np.float64))
    assert (gap[moving] <= 4 * TOL[dtype]).all(), gap[moving].max()
    assert ((u >= 0) & (v >= 0) & (u + v <= 1 + 4 * np.finfo(dtype).eps))[hit].all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_sphere_leaves(dll, dtype):
    s = np.array([[0.5, -1.0, 2.0, 0.75]], dtype=dtype)
    cases = [(_ray(np.array([0.5, -1.0, 7.0]), np.array([0, 0, -2.0])), 0.25, 2.0),                # head on: (5 - 0.75 - 0.25) / 2
             (_ray(np.array([0.5, -1.0, 7.0]), np.array([0, 0, -2.0]), 0.0, 1.99), 0.25, None),   # tmax just short
             (_ray(np.array([0.5, -1.0, 7.0]), np.array([0, 0, 2.0])), 0.25, None),               # moving away
             (_ray(np.array([0.5, 0.2, 2.0]), np.array([0.25, 0, 0]), 0.5, 9.0), 0.5, 0.5),        # overlap at tmin
             (_ray(np.array([0.5, 0.5, 2.0]), np.zeros(3), 0.5, 9.0), 0.5, None),                  # dir = 0, apart
             (_ray(np.array([0.5, -1.0, 7.0]), np.array([0, 0, -2.0])), 0.0, 2.125),               # r = 0: the ray against the sphere
             (_ray(np.array([1.5, -1.0, 7.0]), np.array([0, 0, -1.0])), 0.2, None)]                # passes 0.05 clear
    for ray, r, want in cases:
        hit, t, u, v = host_pairs(dll, s, ray.astype(dtype)[None], np.asarray([r], dtype=dtype), leaf=1)
        assert bool(hit[0]) == (want is not None), (ray, r)
        if want is not None:
            assert _close(dtype, float(t[0]), want) and u[0] == 0 and v[0] == 0


# ---- the walk --------------------------------------------------------------------------------------------------------------------------
def scene_rays(raw, n, dtype, seed, sphere):
    """n rays into a scene: origins in its box blown up by 1.5, aimed at points of the box, |dir| = the aim's distance times a factor in
    [0.5, 2], tmax in {0.5, 1, inf}; radii in {0, 0.1 %, 1 %, 5 %} of the diagonal. Returns (rays, radii, diagonal)."""
    rng = np.random.default_rng(seed)
    pts = raw[:, :3].reshape(-1, 3) if sphere else raw.reshape(-1, 3)
    lo, hi = pts.min(axis=0).astype(np.float64), pts.max(axis=0).astype(np.float64)
    diag = float(np.linalg.norm(hi - lo))
    mid, half = (lo + hi) / 2, (hi - lo) / 2 + 1e-3 * diag
    org = mid + rng.uniform(-1.5, 1.5, (n, 3)) * half
    aim = mid + rng.uniform(-1.0, 1.0, (n, 3)) * half
    d = (aim - org) * rng.uniform(0.5, 2.0, (n, 1))
    rays = np.concatenate([org, d, np.zeros((n, 1)), rng.choice([0.5, 1.0, np.inf], (n, 1))], axis=1).astype(dtype)
    radii = (rng.choice([0.0, 0.001, 0.01, 0.05], n) * diag).astype(dtype)
    return rays, radii, diag


def prim_residuals(raw, ids, rays, radii, hits, sphere):
    """residual / scale of every record of a walk against ITS primitive (original vertices / spheres by BVH order), float64."""
    hit = hits["prim"] != INVALID
    prim = np.where(hit, hits["prim"], 0).astype(np.int64)
    src = raw[ids.astype(np.int64)][prim].astype(np.float64)
    rays64, r = rays.astype(np.float64), radii.astype(np.float64)
    t = np.where(hit, hits["t"].astype(np.float64), 0.0)
    ct = rays64[:, 0:3] + t[:, None] * rays64[:, 3:6]
    if sphere:
        dist = np.maximum(np.linalg.norm(ct - src[:, :3], axis=1) - src[:, 3], 0.0)
        scale = np.maximum(np.abs(src).max(axis=1), np.maximum(np.abs(rays64[:, :3]).max(axis=1), np.abs(ct).max(axis=1)))
    else:
        dist = dist64(src.reshape(-1, 9), ct)
        scale = _scale(src.reshape(-1, 9), rays64, t)
    res = np.where(t == rays64[:, 6], np.maximum(dist - r, 0.0), np.abs(dist - r)) / scale
    return np.where(hit, res, 0.0)


@pytest.mark.parametrize("scene", GOLDEN_SCENES)
@pytest.mark.parametrize("robust", [False, True])
def test_walk_golden(dll, orc, scene, robust):
    bounds, index, prims, leaf, raw, ids = golden_scene(scene, "serial_low" if robust else "parallel_high", orc)
    dt = prims.dtype.type
    rays, radii, diag = scene_rays(raw, 512, dt, 5, leaf == 1)
    hits, cnt = host_walk(dll, bounds, index, prims, rays, radii, leaf, robust=robust)
    brute, tests = host_brute(dll, prims, rays, radii, leaf)
    hit, bhit = hits["prim"] != INVALID, brute["prim"] != INVALID
    assert 50 < hit.sum() and cnt[0] > 0 and 0 < cnt[1] < tests and cnt[2] > 0        # fewer primitives tested than the brute force
    assert (hits["t"] >= brute["t"]).all()                    # the walk tests a subset of what the brute force tests, with the same function
    res = prim_residuals(raw, ids, rays, radii, hits, leaf == 1)
    print(f"{scene} robust={robust}: hits {int(hit.sum())}, brute hits {int(bhit.sum())}, same record {int((hits.tobytes() == brute.tobytes()))}, "
          f"max residual/scale {res.max():.3e}, prim tests {int(cnt[1])} of {tests}")
    assert (res <= TOL[dt]).all(), res.max()
    # where the walk and the brute force differ at all, they differ by a rounding of t, never by a missed contact
    differ = (hits["prim"] != brute["prim"]) | (hits["t"] != brute["t"])
    assert differ.mean() <= 0.02
    both = differ & hit & bhit
    gap = np.abs(hits["t"][both].astype(np.float64) - brute["t"][both].astype(np.float64))
    assert (gap <= 64 * np.sqrt(np.finfo(dt).eps)).all()
    # misses: the miss record
    miss = ~hit
    assert (hits["t"][miss].tobytes() == rays[miss, 7].tobytes()) and (hits["u"][miss] == 0).all() and (hits["v"][miss] == 0).all()
    # a scalar radius is the array of that radius; the reading order changes nothing; original ids map prim only
    h1, c1 = host_walk(dll, bounds, index, prims, rays, float(radii[3]), leaf, robust=robust)
    h2, c2 = host_walk(dll, bounds, index, prims, rays, np.full(len(rays), radii[3], dtype=dt), leaf, robust=robust)
    assert h1.tobytes() == h2.tobytes() and (c1 == c2).all()
    perm = np.random.default_rng(9).permutation(len(rays)).astype(np.uint32)
    hp, cp = host_walk(dll, bounds, index, prims, rays, radii, leaf, robust=robust, order=perm)
    assert hp.tobytes() == hits.tobytes() and (cp == cnt).all()
    ho, _ = host_walk(dll, bounds, index, prims, rays, radii, leaf, robust=robust, prim_ids=ids.astype(np.uint32))
    assert (ho["prim"][hit] == ids[hits["prim"][hit]]).all() and (ho["prim"][miss] == INVALID).all()
    for f in ("t", "u", "v"):
        assert ho[f].tobytes() == hits[f].tobytes()


def dyadic_scene(orc):
    """Axis-aligned unit squares (two triangles each) on an 8 x 8 grid in four planes z = 0, 2, 4, 6, every coordinate an integer;
    rays along the axes from origins at ODD multiples of 1/16, |dir| a power of two, radii in {0, 1/8, 1/4, 1/2}: every plane, slab and
    clearance is exact in float32, and no path grazes a grown box, edge or vertex (an odd multiple of 1/16 is no multiple of 1/8, and
    a^2 + b^2 = 4 c^2 has no odd a, b), so neither the slab test's closed ends nor a zero discriminant decides anything."""
    tris = []
    for z in (0.0, 2.0, 4.0, 6.0):
        for x in range(0, 8):
            for y in range(0, 8):
                tris.append([x, y, z, x + 1, y, z, x + 1, y + 1, z])
                tris.append([x, y, z, x + 1, y + 1, z, x, y + 1, z])
    tris = np.array(tris, dtype=np.float32)
    bb, cc = orc.prep_tris(tris)
    bvh = orc.build(bb, cc, max_leaf=4)
    nodes, ids = bvh.nodes(), bvh.prim_ids()
    rng = np.random.default_rng(12)
    n = 512
    org = (2 * rng.integers(-8, 72, (n, 3)) + 1) / 16.0
    axis, sign = rng.integers(0, 3, n), rng.choice([-1.0, 1.0], n)
    d = np.zeros((n, 3))
    d[np.arange(n), axis] = sign * rng.choice([0.5, 1.0, 2.0, 4.0], n)
    rays = np.concatenate([org, d, np.zeros((n, 1)), rng.choice([2.0, 8.0, 64.0], (n, 1))], axis=1).astype(np.float32)
    radii = rng.choice([0.0, 0.125, 0.25, 0.5], n).astype(np.float32)
    return tris, nodes, ids, rays, radii


def test_walk_equals_brute_force_exactly_on_dyadic_scene(dll, orc):
    """The robust box test: the fast one is the ray walks' (ray_constants, slab_pair), whose -org / dir overflows for a direction
    component of exactly 0 beside |org| > 1, as in intersect: axis-parallel sweeps want robust=True."""
    tris, nodes, ids, rays, radii = dyadic_scene(orc)
    prims = orc.precompute_tris(tris, ids)
    hits, cnt = host_walk(dll, nodes["bounds"], nodes["index"], prims, rays, radii, 0, robust=True)
    brute, tests = host_brute(dll, prims, rays, radii, 0)
    assert hits.tobytes() == brute.tobytes()                  # (t, index), and (u, v) with them
    assert 100 < (hits["prim"] != INVALID).sum() < len(rays) and cnt[1] < tests / 4
    assert ((hits["t"] == 0) & (hits["prim"] != INVALID)).sum() > 5          # initial overlaps among them


@pytest.mark.parametrize("depth", [65, 300])
def test_deep_chain(dll, orc, depth):
    """A chain tree deeper than 64 levels: the Deep walk's HBM spill. Balls flying along +x towards the stack of triangles."""
    tris, nodes, ids = chain_tree(depth, orc.prep_tris)
    prims = precompute(tris, np.float32)
    rng = np.random.default_rng(depth)
    n = 64
    rays = np.zeros((n, 8), dtype=np.float32)
    rays[:, 0] = rng.integers(0, 100, n)
    rays[:, 1:3] = rng.integers(-2, 3, (n, 2)) / 4.0
    rays[:, 3] = 1.0
    rays[:, 7] = np.inf
    hits, cnt = host_walk(dll, nodes["bounds"], nodes["index"], prims, rays, 0.25, 0, deep_cap=depth - 64 + 1)
    brute, _ = host_brute(dll, prims, rays, 0.25, 0)
    assert hits.tobytes() == brute.tobytes() and (hits["prim"] == depth).all()     # the deepest leaf is the first one met


def test_one_primitive_tree_and_invalid_queries(dll):
    """A tree that is one leaf (no box test at all), and the queries that are not walked."""
    from oracle import NODEF
    tri = TRI.astype(np.float32)[None]
    nodes = np.zeros(1, dtype=NODEF)
    nodes[0]["bounds"], nodes[0]["index"] = [tri[0, 0::3].min(), tri[0, 0::3].max(), tri[0, 1::3].min(), tri[0, 1::3].max(), tri[0, 2::3].min(), tri[0, 2::3].max()], (0 << 4) | 1
    prims = precompute(tri, np.float32)
    base = _ray(INTERIOR + 2.0 * NRM, -NRM, 0.0, 10.0)
    rays = np.stack([base, _ray(INTERIOR + 2.0 * NRM, -NRM, np.nan, 10.0), _ray(INTERIOR + 2.0 * NRM, -NRM, 0.0, np.nan),
                     _ray(INTERIOR + 2.0 * NRM, -NRM, 3.0, 1.0), _ray(INTERIOR + 2.0 * NRM, NRM, 0.0, 10.0), base, base]).astype(np.float32)
    radii = np.array([0.25, 0.25, 0.25, 0.25, 0.25, -1.0, np.nan], dtype=np.float32)
    hits, cnt = host_walk(dll, nodes["bounds"], nodes["index"], prims, rays, radii, 0)
    assert hits["prim"][0] == 0 and abs(hits["t"][0] - 1.75) <= 1e-5
    assert (hits["prim"][1:] == INVALID).all() and (hits["u"][1:] == 0).all() and (hits["v"][1:] == 0).all()
    assert hits["t"][1:].tobytes() == rays[1:, 7].tobytes()  # the ray's tmax bits, NaN included
    assert cnt[1] == 3                                        # NaN tmin / tmax, a negative or NaN radius: not walked
