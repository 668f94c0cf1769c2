"""CPU: the TEXT of the winding-number kernels (bvh_amd/csrc/winding_body.inc over point_walk.inc + trace_device.h) compiled for the
host by tests/cpp/winding_body_host.cpp. atan2 against libm, single-triangle solid angles against the float64 formula, the per-node
moments against a float64 restatement (and their bytes under reordered and concurrent climbs), the walk against a float64 brute-force
sum over all triangles, and the classification of points against closed surfaces whose inside is known analytically. The device's
moments, winding numbers and counters must equal this harness's bit for bit (tests/test_gpu_winding.py).

Measured on the CPU (this file prints the figures; DESIGN.md, "Winding numbers" has the tables):
  atan2, largest |error| against float64 / libm over the grid below: float 2.49e-07 (0.67 eps pi), double 4.44e-16 (0.64 eps pi);
  walk, largest |w - w64| per scene at beta = 2 / 3: WALK_MEASURED below (the shell's 0.111 at beta = 2 is the largest)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import winding_scenes as ws
from conftest import ROOT
from test_closest_point_host import HITD, HITF, chain_tree, precompute
from test_kernel_body_host import _aligned, pair_records

HARNESS = os.path.join(ROOT, "tests", "cpp", "winding_body_host.cpp")
BETAS = [2.0, 3.0, math.inf]
DTYPES = [np.float32, np.float64]

# largest |atan2 - reference| measured over atan2_grid(), and the ceiling the issue sets for it: 4 eps pi
ATAN2_MEASURED = {np.float32: 2.50e-07, np.float64: 4.45e-16}
# largest |w - w64| measured per scene over its 2048 queries (float and double trees, Low and High quality: the larger figure), beta = 2 / 3
WALK_MEASURED = {
    "sphere": (0.0448, 0.0162), "torus": (0.0690, 0.0237), "shell": (0.1109, 0.0187), "doubled": (0.0718, 0.0320), "hemisphere": (0.0342, 0.0175),
    "holed": (0.0401, 0.0153), "soup2k": (0.00763, 0.00344),
}


def compile_harness(out_dir):
    out = os.path.join(str(out_dir), "libwinding_body_host.so")
    cmd = ["g++", "-std=c++20", "-O1", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-strict-aliasing", "-Wall", "-Wextra", "-Wno-unused-parameter",
           "-Wno-unknown-pragmas", "-Werror", "-shared", "-fPIC", "-pthread", HARNESS, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    dll = C.CDLL(out)
    P, Z, I, U, D = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_double
    dll.winding_host_atan2.argtypes = [I, P, P, Z, P]
    dll.winding_host_solid_angle.argtypes = [I, P, P, Z, P]
    dll.winding_host_prepare.restype = I
    dll.winding_host_prepare.argtypes = [I, P, U, U, P, Z, P, I, P, P]
    dll.winding_host_walk.restype = I
    dll.winding_host_walk.argtypes = [I, P, U, P, P, P, Z, P, D, U, I, P, P, P]
    return dll


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return compile_harness(tmp_path_factory.mktemp("winding"))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_atan2(dll, y, x):
    y, x = np.ascontiguousarray(y), np.ascontiguousarray(x)
    out = np.empty_like(y)
    dll.winding_host_atan2(int(y.dtype == np.float64), _p(y), _p(x), len(y), _p(out))
    return out


def host_solid_angle(dll, tris9, q, dtype):
    pre = np.ascontiguousarray(precompute(np.asarray(tris9).reshape(-1, 9), dtype))
    qq = np.ascontiguousarray(np.asarray(q, dtype=dtype).reshape(-1, 3))
    assert len(pre) == len(qq)
    out = np.empty(len(pre), dtype=dtype)
    dll.winding_host_solid_angle(int(dtype == np.float64), _p(pre), _p(qq), len(pre), _p(out))
    return out


def host_prepare(dll, bounds6, index, prims, lanes=None, threads=1, with_sums=False):
    """The moments of the tree, (node_count + 1, 8) (and the per-node s, (node_count, 4))."""
    dt = bounds6.dtype
    n = len(index)
    pairs = _aligned(pair_records(bounds6, index))
    prims = _aligned(np.ascontiguousarray(prims, dtype=dt))
    mom = _aligned(np.full((n + 1, 8), 7, dtype=dt))
    sums = np.zeros((n, 4), dtype=dt) if with_sums else None
    lanes = None if lanes is None else np.ascontiguousarray(lanes, dtype=np.uint32)
    assert dll.winding_host_prepare(int(dt == np.float64), _p(pairs), int(index[0]) & 0xFFFFFFFF, n, _p(prims), len(prims), _p(lanes), threads, _p(mom),
                                    _p(sums)) == 0
    return (mom, sums) if with_sums else mom


def host_walk(dll, bounds6, index, prims, moments, queries4, beta=2.0, order=None, deep_cap=0, threads=4, hits=None):
    """The kernel's walk for every query: (w, counters {pair records opened, triangles summed exactly, far terms added})."""
    dt = bounds6.dtype
    pairs = _aligned(pair_records(bounds6, index))
    prims = _aligned(np.ascontiguousarray(prims, dtype=dt))
    moments = _aligned(np.ascontiguousarray(moments, dtype=dt))
    q = _aligned(np.ascontiguousarray(queries4, dtype=dt))
    w = np.full(len(q), 7, dtype=dt)
    cnt = np.zeros(3, dtype=np.uint64)
    order = None if order is None else np.ascontiguousarray(order, dtype=np.uint32)
    assert dll.winding_host_walk(int(dt == np.float64), _p(pairs), int(index[0]) & 0xFFFFFFFF, _p(prims), _p(moments), _p(q), len(q), _p(order), beta,
                                 deep_cap, threads, _p(w), _p(hits), _p(cnt)) == 0
    return w, cnt


def queries4(points, dtype, fourth=0.0):
    q = np.full((len(points), 4), fourth, dtype=dtype)
    q[:, :3] = points
    return q


_TREES = {}


def scene_tree(orc, name, dtype, quality):
    """(raw tris in dtype (n, 9), node bounds, node index words, BVH-order PrecomputedTri, prim ids) of a scene under DefaultBuilder."""
    key = (name, np.dtype(dtype).name, quality)
    if key not in _TREES:
        import oracle
        tris = np.ascontiguousarray(ws.SCENES[name][0]().astype(dtype))
        bb, cc = orc.prep_tris(tris)
        bvh = orc.build(bb, cc, builder=oracle.BUILDER_DEFAULT_SERIAL, quality=quality)
        nodes, ids = bvh.nodes(), bvh.prim_ids()
        _TREES[key] = (tris, nodes["bounds"].copy(), nodes["index"].copy(), np.ascontiguousarray(orc.precompute_tris(tris, ids)), ids)
    return _TREES[key]


_QUERIES = {}


def scene_queries(name):
    """(points float64, expected winding numbers or None): for a classified scene only the points clear of the surface."""
    if name not in _QUERIES:
        tris = ws.SCENES[name][0]()
        q, expect = ws.queries(tris, rule=ws.SCENES[name][1])
        _QUERIES[name] = (q, expect)
    return _QUERIES[name]


_BRUTE = {}


def scene_brute(name, dtype):
    """float64 brute-force w over the scene and queries as rounded to dtype."""
    key = (name, np.dtype(dtype).name)
    if key not in _BRUTE:
        tris = ws.SCENES[name][0]().astype(dtype)
        q, _ = scene_queries(name)
        _BRUTE[key] = ws.brute_winding64(tris, q.astype(dtype))[0]
    return _BRUTE[key]


def tree_depth(index):
    depth, stack = 0, [(0, 0)]
    while stack:
        c, d = stack.pop()
        depth = max(depth, d)
        if int(index[c]) & 15 == 0:
            f = int(index[c]) >> 4
            stack += [(f, d + 1), (f + 1, d + 1)]
    return depth


# ---- atan2 ------------------------------------------------------------------------------------------------------------------------------

def atan2_grid(dtype):
    """(y, x): every octant and both axes, signed zeros, equal magnitudes, tiny and huge ratios, the reduction's cut, pairs of two huge or
    two tiny magnitudes at moderate ratios, random pairs."""
    fi = np.finfo(dtype)
    mags = np.concatenate([[0.0, float(fi.tiny), 1e-30 if dtype == np.float32 else 1e-300, 1e-7, 1e-3, 0.1, 0.41421, 0.41422, 0.5, 0.99999, 1.0, 1.00001,
                            2.0, 2.41421, 2.41422, 10.0, 1e3, 1e7, 1e30 if dtype == np.float32 else 1e300, float(fi.max), np.inf],
                           np.tan(np.linspace(0.0, np.pi / 2, 97)[1:-1])]).astype(dtype)
    ym, xm = [a.ravel() for a in np.meshgrid(mags, mags)]
    y = np.concatenate([s * ym for s in (1, -1) for _ in (0, 1)])
    x = np.concatenate([s * xm for _ in (0, 1) for s in (1, -1)])
    # two magnitudes near the type's largest (and smallest) at ratios on either side of the cut: the reduction's sum must not overflow
    ratios = np.linspace(0.3, 1.0, 41)
    big = np.concatenate([ratios * (f * float(fi.max)) for f in (1.0, 0.7, 0.3)] + [ratios * (f * float(fi.tiny)) for f in (1.0, 64.0)])
    base = np.concatenate([np.full(41, f * float(fi.max)) for f in (1.0, 0.7, 0.3)] + [np.full(41, f * float(fi.tiny)) for f in (1.0, 64.0)])
    for sy in (1, -1):
        for sx in (1, -1):
            y = np.concatenate([y, (sy * big).astype(dtype), (sy * base).astype(dtype)])
            x = np.concatenate([x, (sx * base).astype(dtype), (sx * big).astype(dtype)])
    rng = np.random.default_rng(3)
    ang = rng.random(200000) * 2 * np.pi - np.pi
    rad = np.exp(rng.normal(size=len(ang)) * 5)
    y = np.concatenate([y, (rad * np.sin(ang))]).astype(dtype)
    x = np.concatenate([x, (rad * np.cos(ang))]).astype(dtype)
    return y, x


@pytest.mark.parametrize("dtype", DTYPES)
def test_atan2_accuracy(dll, dtype):
    y, x = atan2_grid(dtype)
    got = host_atan2(dll, y, x)
    if dtype == np.float32:
        ref = np.arctan2(y.astype(np.float64), x.astype(np.float64))
    else:
        ref = np.array([math.atan2(a, b) for a, b in zip(y.tolist(), x.tolist())])
    assert np.isfinite(got).all()
    worst = float(np.max(np.abs(got.astype(np.float64) - ref)))
    eps_pi = float(np.finfo(dtype).eps) * math.pi
    print(f"atan2 {np.dtype(dtype).name}: largest |error| = {worst:.3e} = {worst / eps_pi:.2f} eps pi over {len(y)} pairs")
    assert ATAN2_MEASURED[dtype] <= 4 * eps_pi
    assert worst <= 2 * ATAN2_MEASURED[dtype]
    assert (np.signbit(got) == np.signbit(y)).all()           # the sign is y's, zeros included


@pytest.mark.parametrize("dtype", DTYPES)
def test_atan2_axes_and_specials(dll, dtype):
    pi = dtype(math.pi)
    z, one, inf = dtype(0.0), dtype(1.0), dtype(np.inf)
    cases = [(z, one), (-z, one), (z, -one), (-z, -one), (z, z), (-z, z), (z, -z), (-z, -z), (one, z), (-one, z), (one, -z), (-one, -z),
             (one, one), (-one, one), (one, -one), (-one, -one), (inf, inf), (-inf, inf), (inf, -inf), (one, inf), (one, -inf), (inf, one),
             (dtype(3.0), z), (z, dtype(5.0)), (dtype(1e-20), dtype(-1e20)), (dtype(1e20), dtype(1e-20))]
    y = np.array([c[0] for c in cases], dtype=dtype)
    x = np.array([c[1] for c in cases], dtype=dtype)
    got = host_atan2(dll, y, x)
    ref = np.arctan2(y, x)                                     # in dtype: the axis values are the type's roundings of k pi / 4
    axis = (y == 0) | (x == 0) | (np.isinf(y) ^ np.isinf(x))
    assert got[axis].tobytes() == ref[axis].tobytes(), (got[axis], ref[axis])
    assert (np.signbit(got) == np.signbit(ref)).all()
    assert np.max(np.abs(got.astype(np.float64) - ref.astype(np.float64))) <= 2 * np.finfo(dtype).eps * math.pi
    assert got[12] == pi / 4 and got[13] == -pi / 4          # equal magnitudes: exactly the type's pi / 4
    nan = host_atan2(dll, np.array([np.nan, 1, np.nan], dtype=dtype), np.array([1, np.nan, np.nan], dtype=dtype))
    assert np.isnan(nan).all()


# ---- one triangle -----------------------------------------------------------------------------------------------------------------------

TRI = np.array([0.2, -0.1, 0.3, 1.7, 0.4, -0.2, -0.3, 1.5, 0.6])
A, B, Cv = TRI[0:3], TRI[3:6], TRI[6:9]
NRM = np.cross(B - A, Cv - A) / np.linalg.norm(np.cross(B - A, Cv - A))
CEN = (A + B + Cv) / 3


@pytest.mark.parametrize("dtype", DTYPES)
def test_single_triangle_solid_angles(dll, dtype):
    eps = float(np.finfo(dtype).eps)
    tri = TRI.astype(dtype).astype(np.float64)
    rng = np.random.default_rng(19)
    around = [CEN + s * h * NRM + 0.8 * rng.normal(size=3) * (1, 1, 0.2) for h in (0.01, 0.3, 2.0) for s in (1, -1) for _ in range(20)]
    far = [CEN + 1e3 * v / np.linalg.norm(v) for v in rng.normal(size=(10, 3))]
    q = np.array(around + far).astype(dtype)
    got = host_solid_angle(dll, np.tile(tri, (len(q), 1)), q, dtype).astype(np.float64)
    ref = np.array([ws.solid_angles64(tri, p[None].astype(np.float64))[0, 0] for p in q])
    # a rounding of the vertices' differences (eps of the coordinates) moves the angle by about eps / distance
    dist = np.array([np.linalg.norm(p - CEN) for p in q.astype(np.float64)])
    assert (np.abs(got - ref) <= 64 * eps * (1 + 1 / np.minimum(dist, 1.0))).all(), np.max(np.abs(got - ref))
    assert (np.sign(got) == np.sign(ref)).all() and np.abs(got).max() < 2 * math.pi
    # the other orientation: the sign flips exactly
    flipped = np.concatenate([tri[0:3], tri[6:9], tri[3:6]])
    got_f = host_solid_angle(dll, np.tile(flipped, (len(q), 1)), q, dtype).astype(np.float64)
    assert (np.sign(got_f) == -np.sign(got)).all()             # the sign flips exactly
    # ... and the magnitude is the same but for the order of the factors of |a||b||c| (b and c change places): a few eps, in the type
    assert np.abs(got_f + got).max() <= 16 * eps, np.abs(got_f + got).max()
    # in the triangle's plane outside it, and at a vertex: exactly 0 (an exactly representable triangle in the plane z = 0.5)
    flat = np.array([0, 0, 0.5, 2, 0, 0.5, 0, 2, 0.5], dtype=np.float64)
    zero_q = np.array([[3, 3, 0.5], [-1, 0.5, 0.5], [1.5, 1.5, 0.5], [0, 0, 0.5], [2, 0, 0.5], [0, 2, 0.5]], dtype=np.float64)
    z = host_solid_angle(dll, np.tile(flat, (len(zero_q), 1)), zero_q, dtype)
    assert (z == 0).all(), z


@pytest.mark.parametrize("dtype", DTYPES)
def test_degenerate_triangles_add_nothing(dll, dtype):
    from test_closest_point_host import DEGENERATE, DEGENERATE_QUERIES
    for name, tri in DEGENERATE.items():
        q = np.asarray(DEGENERATE_QUERIES, dtype=np.float64)
        got = host_solid_angle(dll, np.tile(np.asarray(tri, np.float64), (len(q), 1)), q, dtype)
        assert (got == 0).all(), (name, got)


# ---- the moments ------------------------------------------------------------------------------------------------------------------------

def moments64(index, prims, bounds6):
    """float64 restatement (centroids from extended precision) over the dtype-rounded PrecomputedTri: per node N (3), area, s (3), the sums of |terms| of N and s (3 + 3),
    and the BVH-order triangle indices below it."""
    p = prims.astype(np.longdouble)                         # (the centroid in extended precision: p0 + (e2 - e1) / 3 cancels where a triangle
    area_vec = (-0.5 * p[:, 9:12]).astype(np.float64)       #  lies across a coordinate plane, and a float64 tree is checked against this too)
    length = np.linalg.norm(area_vec, axis=1)
    cen = (p[:, 0:3] + (p[:, 6:9] - p[:, 3:6]) / 3).astype(np.float64)
    n = len(index)
    N, area, s = np.zeros((n, 3)), np.zeros(n), np.zeros((n, 3))
    absN, abss = np.zeros((n, 3)), np.zeros((n, 3))
    below = [None] * n
    order, stack = [], [0]
    while stack:
        c = stack.pop()
        order.append(c)
        if int(index[c]) & 15 == 0:
            f = int(index[c]) >> 4
            stack += [f, f + 1]
    for c in reversed(order):
        w = int(index[c])
        if w & 15:
            r = np.arange(w >> 4, (w >> 4) + (w & 15))
            below[c] = r
            N[c], area[c], s[c] = area_vec[r].sum(axis=0), length[r].sum(), (length[r, None] * cen[r]).sum(axis=0)
            absN[c], abss[c] = np.abs(area_vec[r]).sum(axis=0), np.abs(length[r, None] * cen[r]).sum(axis=0)
        else:
            f = w >> 4
            below[c] = np.concatenate([below[f], below[f + 1]])
            N[c], area[c], s[c] = N[f] + N[f + 1], area[f] + area[f + 1], s[f] + s[f + 1]
            absN[c], abss[c] = absN[f] + absN[f + 1], abss[f] + abss[f + 1]
    return N, area, s, absN, abss, below, order


def check_moments(dll, tris, bounds, index, prims, ids, closed):
    dt = bounds.dtype
    eps = float(np.finfo(dt).eps)
    mom, sums = host_prepare(dll, bounds, index, prims, with_sums=True)
    assert (mom[0] == 0).all()
    N, area, s, absN, abss, below, reach = moments64(index, prims, bounds)
    rows = mom[1:].astype(np.float64)
    k = (tree_depth(index) + int((index & 15).max()) + 8) * eps            # (depth + largest leaf + 8) eps
    reach = np.asarray(reach)
    assert (np.abs(rows[reach, 4:7] - N[reach]) <= k * absN[reach]).all()
    assert (np.abs(rows[reach, 7] - area[reach]) <= k * area[reach]).all()
    assert (np.abs(sums[reach, :3].astype(np.float64) - s[reach]) <= k * abss[reach]).all()
    if closed:
        assert (np.abs(rows[0, 4:7]) <= k * absN[0]).all(), rows[0]           # a closed surface: the area vectors cancel
    verts = tris.astype(np.float64).reshape(-1, 3, 3)[ids.astype(np.int64)]  # BVH order
    for c in reach:
        v = verts[below[c]].reshape(-1, 3)
        d = np.linalg.norm(v - rows[c, 0:3], axis=1).max()
        assert d <= math.sqrt(rows[c, 3]) * (1 + 4 * eps), (c, d, rows[c])
        if area[c] > 0:
            assert np.abs(rows[c, 0:3] - s[c] / area[c]).max() <= 4 * k * abss[c].max() / area[c]
    return mom


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(ws.SCENES))
def test_moments_on_scene_trees(dll, orc, name, dtype):
    import oracle
    for quality in (oracle.QUALITY_LOW, oracle.QUALITY_HIGH):
        tris, bounds, index, prims, ids = scene_tree(orc, name, dtype, quality)
        mom = check_moments(dll, tris, bounds, index, prims, ids, name in ws.CLOSED)
        # the bytes do not depend on the order the lanes start in, nor on lanes climbing at the same time
        n = len(index)
        shuffled = np.random.default_rng(n).permutation(n)
        assert host_prepare(dll, bounds, index, prims, lanes=shuffled).tobytes() == mom.tobytes()
        assert host_prepare(dll, bounds, index, prims, lanes=np.arange(n)[::-1]).tobytes() == mom.tobytes()
        assert host_prepare(dll, bounds, index, prims, threads=8).tobytes() == mom.tobytes()
        assert host_prepare(dll, bounds, index, prims, lanes=shuffled, threads=8).tobytes() == mom.tobytes()


@pytest.mark.parametrize("scene", ["cornell", "soup2k", "terrain2k", "soup2k_f64"])
@pytest.mark.parametrize("mode", ["serial_low", "parallel_high"])
def test_moments_on_golden_trees(dll, orc, scene, mode):
    from test_closest_point_host import golden_scene
    bounds, index, prims, leaf, raw, ids = golden_scene(scene, mode, orc)
    mom = check_moments(dll, np.ascontiguousarray(raw).reshape(-1, 9), bounds, index, prims, ids, False)
    assert host_prepare(dll, bounds, index, prims, threads=8, lanes=np.random.default_rng(1).permutation(len(index))).tobytes() == mom.tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_degenerate_node_takes_the_box_centre(dll, dtype):
    from oracle import NODED, NODEF
    tris = np.array([[0, 0, 0, 1, 1, 1, 3, 3, 3], [1, 2, 3, 1, 2, 3, 1, 2, 3], [5, 0, 0, 6, 0, 0, 5, 1, 0]], dtype=dtype)
    nodes = np.zeros(3, dtype=NODEF if dtype == np.float32 else NODED)
    nodes[0]["bounds"], nodes[0]["index"] = [0, 6, 0, 3, 0, 3], 1 << 4
    nodes[1]["bounds"], nodes[1]["index"] = [0, 3, 0, 3, 0, 3], (0 << 4) | 2
    nodes[2]["bounds"], nodes[2]["index"] = [5, 6, 0, 1, 0, 0], (2 << 4) | 1
    mom = host_prepare(dll, nodes["bounds"], nodes["index"], precompute(tris, dtype))
    assert mom[2].tolist() == [1.5, 1.5, 1.5, 3 * 1.5 ** 2, 0, 0, 0, 0]                 # node 1: no area, the centre of its box
    assert mom[3, 7] == 0.5 and mom[3, 6] == 0.5 and mom[3, 3] > 0                       # node 2: one right triangle of area 1/2, facing +z
    assert np.allclose(mom[3, 0:3], [16 / 3, 1 / 3, 0], rtol=4 * np.finfo(dtype).eps)
    assert mom[1, 7] == 0.5 and np.allclose(mom[1, 0:3], mom[3, 0:3]) and mom[1, 3] > mom[3, 3]   # the root: the same centre, its own box


def test_single_leaf_root(dll):
    from oracle import NODEF
    tris = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1, 1, 0, 1, 0, 1, 1]], dtype=np.float32)
    nodes = np.zeros(1, dtype=NODEF)
    nodes[0]["bounds"], nodes[0]["index"] = [0, 1, 0, 1, 0, 1], (0 << 4) | 2
    prims = precompute(tris, np.float32)
    mom = host_prepare(dll, nodes["bounds"], nodes["index"], prims)
    assert mom[1, 7] == 1.0 and mom[1, 6] == 1.0 and mom[1, 3] > 0
    q = queries4(np.array([[0.2, 0.2, 0.5], [0.2, 0.2, 30.0]]), np.float32)
    w, cnt = host_walk(dll, nodes["bounds"], nodes["index"], prims, mom, q, beta=2.0, threads=1)
    assert list(cnt) == [0, 2, 1] and abs(w[0]) < 1e-6 and w[1] < 0


# ---- the walk ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(ws.SCENES))
def test_walk_against_brute_force(dll, orc, name, dtype):
    import oracle
    eps = float(np.finfo(dtype).eps)
    pts, expect = scene_queries(name)
    w64 = scene_brute(name, dtype)
    q = queries4(pts, dtype)
    for quality in (oracle.QUALITY_LOW, oracle.QUALITY_HIGH):
        tris, bounds, index, prims, ids = scene_tree(orc, name, dtype, quality)
        mom = host_prepare(dll, bounds, index, prims)
        for beta, measured in zip(BETAS, WALK_MEASURED[name] + (None,)):
            w, cnt = host_walk(dll, bounds, index, prims, mom, q, beta=beta)
            assert np.isfinite(w).all()
            err = float(np.max(np.abs(w.astype(np.float64) - w64)))
            per_query = [int(c) / len(q) for c in cnt]
            print(f"winding {name} {np.dtype(dtype).name} quality {quality} beta {beta}: largest |w - w64| = {err:.3e}; per query "
                  f"{per_query[0]:.1f} pair records, {per_query[1]:.1f} triangles, {per_query[2]:.1f} far terms")
            if math.isinf(beta):
                assert cnt[2] == 0 and cnt[1] == len(q) * len(prims)         # every triangle, exactly
                assert err <= 16 * eps * (int(cnt[1]) / len(q))
            else:
                assert cnt[2] > 0 and cnt[1] < len(q) * len(prims)
                assert measured < 0.25 and err <= 2 * measured
            if expect is not None:                                          # a condition, not a measurement
                assert (np.rint(w).astype(np.int64) == expect).all(), (name, beta, np.abs(w - expect).max())


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_queries_order_and_position(dll, orc, dtype):
    import oracle
    tris, bounds, index, prims, ids = scene_tree(orc, "sphere", dtype, oracle.QUALITY_HIGH)
    mom = host_prepare(dll, bounds, index, prims)
    pts, _ = scene_queries("sphere")
    q = queries4(pts[:512], dtype, fourth=np.nan)              # the fourth slot is not read
    w, cnt = host_walk(dll, bounds, index, prims, mom, q)
    assert np.isfinite(w).all()
    w0, _ = host_walk(dll, bounds, index, prims, mom, queries4(pts[:512], dtype, fourth=1.0))
    assert w0.tobytes() == w.tobytes()
    perm = np.random.default_rng(5).permutation(len(q)).astype(np.uint32)
    wp, cp = host_walk(dll, bounds, index, prims, mom, q, order=perm)
    assert wp.tobytes() == w.tobytes() and list(cp) == list(cnt)
    ws_, _ = host_walk(dll, bounds, index, prims, mom, q[perm])                        # another position in another batch
    assert ws_.tobytes() == w[perm].tobytes()
    w1, _ = host_walk(dll, bounds, index, prims, mom, q[100:101], threads=1)
    assert w1[0].tobytes() == w[100].tobytes()
    # NaN and infinite coordinates: w = NaN, the hit record untouched; an inside query's t is negated, an outside one's is not
    bad = queries4(np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [0.1, 0.2, 0.3], [3, 3, 3]]), dtype)
    hits = np.zeros(5, dtype=HITD if dtype == np.float64 else HITF)
    hits["prim"], hits["t"], hits["u"], hits["v"] = 11, 2.5, 0.25, 0.5
    before = hits.copy()
    wb, _ = host_walk(dll, bounds, index, prims, mom, bad, threads=1, hits=hits)
    assert np.isnan(wb[:3]).all() and round(float(wb[3])) == 1 and round(float(wb[4])) == 0
    assert hits[:3].tobytes() == before[:3].tobytes() and hits[4].tobytes() == before[4].tobytes()
    assert hits["t"][3] == -2.5
    hits["t"][3] = 2.5
    assert hits.tobytes() == before.tobytes()                 # nothing else was touched


def mirror_siblings(nodes):
    """Every pair of siblings swapped (the index words name the pair, so they stay valid)."""
    out = nodes.copy()
    out[1::2], out[2::2] = nodes[2::2], nodes[1::2]
    return out


@pytest.mark.parametrize("depth", [65, 300])
@pytest.mark.parametrize("mirrored", [False, True])
def test_deep_chain(dll, orc, depth, mirrored):
    """The chain tree of the closest-point tests, deeper than 64 levels, through the Deep path. As it stands its inner child is the
    right one, which this walk pops before it descends: the stack never holds more than one entry. Mirrored (siblings swapped, the
    inner child on the left) the walk stacks one entry per level: LDS, scratch, then the spill beyond 64."""
    tris, nodes, ids = chain_tree(depth, orc.prep_tris)
    if mirrored:
        nodes = mirror_siblings(nodes)
    prims = precompute(tris, np.float32)
    mom = host_prepare(dll, nodes["bounds"], nodes["index"], prims)
    rng = np.random.default_rng(depth)
    pts = np.stack([4000 - depth + rng.random(64) * depth, (rng.random(64) - 0.5) * 1.5, (rng.random(64) - 0.5) * 1.5], axis=1)
    q = queries4(pts, np.float32)
    w64 = ws.brute_winding64(tris.astype(np.float64), q[:, :3].astype(np.float64))[0]
    w, cnt = host_walk(dll, nodes["bounds"], nodes["index"], prims, mom, q, beta=math.inf, deep_cap=depth - 64 + 1, threads=1)
    assert cnt[0] == depth * len(q) and cnt[1] == (depth + 1) * len(q)
    assert np.abs(w - w64).max() <= 16 * np.finfo(np.float32).eps * (depth + 1)
    w2, cnt2 = host_walk(dll, nodes["bounds"], nodes["index"], prims, mom, q, beta=2.0, deep_cap=depth - 64 + 1, threads=1)
    assert cnt2[2] > 0 and np.abs(w2 - w64).max() < 0.05
