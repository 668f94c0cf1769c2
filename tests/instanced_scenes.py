"""TEST INFRASTRUCTURE shared by tests/test_instanced_host.py and tests/test_gpu_instanced.py: the host harness of the instanced ray
kernels (tests/cpp/instanced_body_host.cpp = bvh_amd/csrc/instanced_body.inc compiled by g++), the two-level scenes the tests trace,
and the expected results as a sequential composition of the CPU checker's own single-level `intersect_tri`."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle
from conftest import ROOT
from test_kernel_body_host import _aligned, pair_records

HARNESS = os.path.join(ROOT, "tests", "cpp", "instanced_body_host.cpp")
INVALID = 0xFFFFFFFF
MODES4 = [(a, r) for a in (False, True) for r in (False, True)]


def compile_harness(out_dir):
    """g++ with the flags of test_closest_point_host.compile_harness."""
    out = os.path.join(str(out_dir), "libinstanced_body_host.so")
    cmd = ["g++", "-std=c++20", "-O1", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-strict-aliasing", "-Wall", "-Wextra", "-Wno-unused-parameter",
           "-Wno-unknown-pragmas", "-Werror", "-shared", "-fPIC", "-pthread", HARNESS, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    dll = C.CDLL(out)
    P, Z, I, U = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32
    dll.instanced_host_walk.restype = I
    dll.instanced_host_walk.argtypes = [I, P, U, P, U, P, P, P, P, P, P, P, Z, I, I, I, U, I, P, P, P]
    dll.instanced_host_prepare.restype = I
    dll.instanced_host_prepare.argtypes = [I, U, P, P, P, Z, P, P, P]
    return dll


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _ptr_array(arrays):
    return (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


class Geometry:
    """One mesh: its tree as (nodes, prim ids), the BVH-order PrecomputedTri, the checker's own Bvh for the expected results."""

    def __init__(self, orc, tris9, nodes=None, ids=None):
        self.tris9 = np.ascontiguousarray(tris9)
        self.dtype = self.tris9.dtype
        if nodes is None:
            bb, cc = orc.prep_tris(self.tris9)
            self.cpu = orc.build(bb, cc)
            nodes, ids = self.cpu.nodes(), self.cpu.prim_ids()
        else:
            self.cpu = orc.from_arrays(nodes, ids)
        self.nodes, self.ids = nodes, np.ascontiguousarray(ids, dtype=np.uint64)
        self.tris12 = _aligned(np.ascontiguousarray(orc.precompute_tris(self.tris9, self.ids)))
        self.pairs = _aligned(pair_records(nodes["bounds"], nodes["index"]))
        self.ids32 = self.ids.astype(np.uint32)
        self.root_index = int(nodes["index"][0]) & 0xFFFFFFFF
        self.root_box = np.ascontiguousarray(nodes["bounds"][0])


class Scene:
    """Geometries, instances {object-to-world 3 x 4, geometry index} and a top tree over the harness's own instance boxes."""

    def __init__(self, dll, geoms, obj2world, geometry_ids):
        self.dll, self.geoms = dll, geoms
        self.dtype = geoms[0].dtype
        self.double = self.dtype == np.float64
        self.obj2world = _aligned(np.ascontiguousarray(obj2world, dtype=self.dtype).reshape(-1, 12))
        self.gids = None if geometry_ids is None else np.ascontiguousarray(geometry_ids, dtype=np.uint32)
        self.world2obj, self.bboxes, self.centers = host_prepare(dll, [g.root_box for g in geoms], self.obj2world, self.gids)
        self.n = len(self.obj2world)
        self.top_nodes = self.top_ids = None

    def gid(self, i):
        return 0 if self.gids is None else int(self.gids[i])

    def enabled(self, i):
        return self.gid(i) < len(self.geoms) and not np.isnan(self.world2obj[i, 0])

    def single_leaf_top(self, seed=3):
        """One leaf node, index = count with first = 0, prim ids a shuffled permutation: the walk order is the slot order."""
        assert self.n <= 15
        nodes = np.zeros(1, dtype=oracle.NODED if self.double else oracle.NODEF)
        lo, hi = self.bboxes[:, :3].min(axis=0), self.bboxes[:, 3:].max(axis=0)
        nodes[0]["bounds"] = [lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]]
        nodes[0]["index"] = self.n
        self.top_nodes, self.top_ids = nodes, np.random.default_rng(seed).permutation(self.n).astype(np.uint64)
        return self

    def built_top(self, orc):
        """The checker's default builder over the instance boxes."""
        cpu = orc.build(self.bboxes, self.centers)
        self.top_nodes, self.top_ids = cpu.nodes(), cpu.prim_ids()
        return self

    def top_depth(self):
        """Deepest level of the top tree (root = 0)."""
        index = self.top_nodes["index"]
        depth, todo = 0, [(0, 0)]
        while todo:
            node, d = todo.pop()
            depth = max(depth, d)
            if int(index[node]) & 15 == 0:
                first = int(index[node]) >> 4
                todo += [(first, d + 1), (first + 1, d + 1)]
        return depth


def host_prepare(dll, root_boxes, obj2world, gids):
    """The kernel's instance preparation on the host: (world2obj (n, 12), bboxes (n, 6), centers (n, 3))."""
    dt = obj2world.dtype
    n = len(obj2world)
    w, bb, cc = _aligned(np.zeros((n, 12), dtype=dt)), np.zeros((n, 6), dtype=dt), np.zeros((n, 3), dtype=dt)
    boxes = [np.ascontiguousarray(b, dtype=dt) for b in root_boxes]
    assert dll.instanced_host_prepare(int(dt == np.float64), len(boxes), _ptr_array(boxes), _p(obj2world), _p(gids), n, _p(w), _p(bb), _p(cc)) == 0
    return w, bb, cc


def host_walk(scene, rays, any_hit, robust, original_ids=False, deep_cap=0, threads=4):
    """The kernel's two-level walk on the host: (hit records, instance per ray, counters {pairs, tests, leaves})."""
    g = scene.geoms
    rays = _aligned(np.ascontiguousarray(rays, dtype=scene.dtype))
    top_pairs = _aligned(pair_records(scene.top_nodes["bounds"], scene.top_nodes["index"]))
    top_ids = scene.top_ids.astype(np.uint32)
    hits = _aligned(np.zeros(len(rays), dtype=oracle.HITD if scene.double else oracle.HITF))
    inst = np.zeros(len(rays), dtype=np.uint32)
    cnt = np.zeros(3, dtype=np.uint64)
    roots = np.array([x.root_index for x in g], dtype=np.uint32)
    rc = scene.dll.instanced_host_walk(int(scene.double), _p(top_pairs), int(scene.top_nodes["index"][0]) & 0xFFFFFFFF, _p(top_ids), len(g),
                                       _ptr_array([x.pairs for x in g]), _ptr_array([x.tris12 for x in g]), _ptr_array([x.ids32 for x in g]), _p(roots),
                                       _p(scene.world2obj), _p(scene.gids), _p(rays), len(rays), int(any_hit), int(robust), int(original_ids), deep_cap,
                                       threads, _p(hits), _p(inst), _p(cnt))
    assert rc == 0
    return hits, inst, cnt


def transform_rays(w12, rays):
    """org' = W org + w, dir' = W dir in the rays' scalar type, with dot3's operation order: ((0 + a0 b0) + a1 b1) + a2 b2, then + w."""
    out = rays.copy()
    zero = rays.dtype.type(0)
    with np.errstate(invalid="ignore"):                       # (an infinite origin: inf x 0)
        for k in range(3):
            a0, a1, a2, a3 = (w12[4 * k + j] for j in range(4))
            out[:, k] = (((zero + a0 * rays[:, 0]) + a1 * rays[:, 1]) + a2 * rays[:, 2]) + a3
            out[:, 3 + k] = ((zero + a0 * rays[:, 3]) + a1 * rays[:, 4]) + a2 * rays[:, 5]
    return out


def nan_flagged(rays):
    return np.isnan(rays[:, 6]) | np.isnan(rays[:, 7])


def compose(scene, rays, order, any_hit, robust, original_ids=False, tmax=None):
    """The expected result: the checker's single-level intersect_tri, one instance after the other in `order` — the still-live rays
    carried into the instance's object space with their running tmax, the hits it reports taken over. Returns (hit records, instance
    per ray, counters = the sum of the calls' counters; the caller adds the top tree's share)."""
    rays = np.ascontiguousarray(rays, dtype=scene.dtype)
    n = len(rays)
    hits = np.zeros(n, dtype=oracle.HITD if scene.double else oracle.HITF)
    hits["prim"] = INVALID
    t = rays[:, 7].copy() if tmax is None else np.asarray(tmax, dtype=scene.dtype).copy()
    hits["t"] = t
    inst = np.full(n, INVALID, dtype=np.uint32)
    live = ~nan_flagged(rays)
    cnt = np.zeros(3, dtype=np.uint64)
    for i in order:
        i = int(i)
        if not scene.enabled(i):
            continue
        idx = np.nonzero(live)[0]
        if len(idx) == 0:
            break
        geom = scene.geoms[scene.gid(i)]
        local = transform_rays(scene.world2obj[i], rays[idx])
        local[:, 7] = t[idx]
        h, c = geom.cpu.intersect_tri(geom.tris12, local, any_hit, robust, counters=True)
        cnt += c
        got = h["prim"] != INVALID
        sel = idx[got]
        for f in ("t", "u", "v"):
            hits[f][sel] = h[f][got]
        hits["prim"][sel] = geom.ids32[h["prim"][got]] if original_ids else h["prim"][got]
        t[sel] = h["t"][got]
        inst[sel] = i
        if any_hit:
            live[sel] = False
    return hits, inst, cnt


def same_records(a, b):
    """Bit-equal prim, t, u, v (NaN included; the padding word of the double record is not compared)."""
    return all(np.ascontiguousarray(a[f]).tobytes() == np.ascontiguousarray(b[f]).tobytes() for f in ("prim", "t", "u", "v"))


# ---- the scenes -----------------------------------------------------------------------------------------------------------------

def _rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def affine(rng, translation, scale=(0.6, 1.6)):
    """rotation x non-uniform scale x shear, and a translation: a (12,) row-major 3 x 4."""
    shear = np.eye(3)
    shear[0, 1], shear[0, 2], shear[1, 2] = rng.uniform(-0.3, 0.3, size=3)
    m = _rotation(rng) @ np.diag(rng.uniform(*scale, size=3)) @ shear
    return np.concatenate([m, np.asarray(translation, np.float64).reshape(3, 1)], axis=1).reshape(12)


def centred(tris9):
    """The mesh moved and scaled into the cube [-1, 1]^3 around the origin."""
    p = np.asarray(tris9, np.float64).reshape(-1, 3)
    lo, hi = p.min(axis=0), p.max(axis=0)
    return ((p - 0.5 * (lo + hi)) / (0.5 * float((hi - lo).max()))).reshape(-1, 9)


def three_geometries(orc, dtype):
    """A ~300-triangle soup, a 16 x 16-cell terrain, and a single triangle whose root is a leaf."""
    from bvh_amd import synth
    soup = centred(synth.soup(300, seed=21, jitter=0.08, dtype=np.float64)).astype(dtype)
    terrain = centred(synth.terrain(512, dtype=np.float64)).astype(dtype)
    one = np.array([[-1.0, -0.8, 0.1, 1.0, -0.7, -0.2, 0.1, 0.9, 0.15]]).astype(dtype)
    geoms = [Geometry(orc, soup), Geometry(orc, terrain), Geometry(orc, one)]
    assert len(terrain) == 512 and geoms[2].root_index & 15 == 1
    return geoms


def scene12(dll, orc, dtype):
    """H1: 3 geometries, 12 instances (rotation x non-uniform scale x shear), of them one identity, one disabled (singular), one with a
    geometry index outside the table; a single-leaf top tree with shuffled prim ids."""
    rng = np.random.default_rng(1201)
    geoms = three_geometries(orc, dtype)
    cells = [(4.0 * (k % 4), 4.0 * (k // 4), 1.5 * ((k * 7) % 3)) for k in range(12)]
    m = np.array([affine(rng, cells[k]) for k in range(12)])
    gids = np.array([k % 3 for k in range(12)], dtype=np.uint32)
    m[0] = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).reshape(12)          # identity, at the origin cell
    m[5, 4:7] = 0.0                                                                     # a zero row: determinant exactly 0, disabled
    gids[9] = 7                                                                         # outside the table
    scene = Scene(dll, geoms, m.astype(dtype), gids).single_leaf_top()
    assert np.isnan(scene.world2obj[5]).all() and not np.isnan(np.delete(scene.world2obj, 5, axis=0)).any()
    return scene


def scene_rays(scene, n, seed):
    """About 2/3 aimed at instance centres, about 1/6 grazing or missing, some cut by tmax to land between instances, four with NaN /
    +-inf in tmin / tmax / origin. Directions are not normalised and have no component that is exactly zero."""
    rng = np.random.default_rng(seed)
    lo, hi = scene.bboxes[:, :3].min(axis=0).astype(np.float64), scene.bboxes[:, 3:].max(axis=0).astype(np.float64)
    ctr, rad = 0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo))
    d = rng.normal(size=(n, 3))
    org = ctr + 1.6 * rad * d / np.linalg.norm(d, axis=1, keepdims=True)
    which = rng.integers(0, scene.n, size=n)
    target = scene.centers[which].astype(np.float64) + rng.normal(scale=0.15, size=(n, 3))
    graze = rng.random(n) < 1 / 6
    half = 0.5 * (scene.bboxes[which, 3:] - scene.bboxes[which, :3]).astype(np.float64)
    target[graze] += (np.sign(rng.normal(size=(n, 3))) * half * rng.uniform(0.9, 1.6, size=(n, 1)))[graze]
    away = rng.random(n) < 1 / 12
    target[away] = org[away] + rng.normal(size=(n, 3))[away]
    dirs = (target - org) * rng.uniform(0.3, 2.0, size=(n, 1))
    dirs[dirs == 0] = 1e-3
    rays = np.zeros((n, 8), dtype=scene.dtype)
    rays[:, 0:3], rays[:, 3:6] = org, dirs
    rays[:, 6] = 0
    rays[:, 7] = np.inf
    cut = rng.random(n) < 0.2                                                           # t = 1 is at the target: end before, at or behind it
    rays[cut, 7] = rng.uniform(0.3, 1.4, size=n)[cut].astype(scene.dtype)
    rays[rng.random(n) < 0.1, 6] = 0.5
    if n >= 8:
        rays[n // 7, 6] = np.nan
        rays[2 * n // 7, 7] = np.nan
        rays[3 * n // 7, 6], rays[3 * n // 7, 7] = -np.inf, np.inf
        rays[4 * n // 7, 0] = np.nan
        rays[5 * n // 7, 1] = np.inf
    assert not (rays[:, 3:6] == 0).any()
    return rays


def scene200(dll, orc, dtype=np.float32, seed=77):
    """H3: 200 instances of the three geometries scattered in a box, a top tree from the checker's default builder."""
    rng = np.random.default_rng(seed)
    geoms = three_geometries(orc, dtype)
    m = np.array([affine(rng, rng.uniform(-12, 12, size=3)) for _ in range(200)])
    gids = rng.integers(0, 3, size=200).astype(np.uint32)
    return Scene(dll, geoms, m.astype(dtype), gids).built_top(orc)


def chain_scene(dll, orc, depth, n_rays=96):
    """H5: the chain-shaped tree of test_closest_point_host.chain_tree (depth + 1 triangles, one stacked entry per level) as the one
    geometry of three instances under a single-leaf top tree; rays from in front of the stack of triangles. (scene, rays, deep_cap)."""
    from test_closest_point_host import chain_queries, chain_tree
    tris, nodes, ids = chain_tree(depth, orc.prep_tris)
    rng = np.random.default_rng(depth)
    geom = Geometry(orc, tris, nodes, ids)
    m = np.array([np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).reshape(12), affine(rng, (0.0, 30.0, 0.0), (0.9, 1.1)),
                  affine(rng, (0.0, -40.0, 10.0), (0.9, 1.1))])
    scene = Scene(dll, [geom], m.astype(np.float32), None).single_leaf_top()
    q = chain_queries(depth, n_rays).astype(np.float64)
    org = q[:, :3]
    dirs = np.stack([np.full(len(q), 1.0), rng.uniform(-1e-4, 1e-4, len(q)) + 2e-4, rng.uniform(-1e-4, 1e-4, len(q)) - 2e-4], axis=1)
    rays = np.zeros((len(q), 8), dtype=np.float32)
    for k in range(len(q)):                                                             # ray k starts in the object space of instance k % 3
        a = m[k % 3].reshape(3, 4)
        rays[k, 0:3], rays[k, 3:6] = a[:, :3] @ org[k] + a[:, 3], a[:, :3] @ dirs[k]
    rays[:, 7] = np.inf
    assert not (rays[:, 3:6] == 0).any()
    return scene, rays, (scene.top_depth() + 1 + depth) - 64 + 1
