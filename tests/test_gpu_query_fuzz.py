"""MI355X: the point queries (closest_points, radius_count / radius_search, knn) and the box queries (overlap_*, self_overlaps) on the
adversarial scenes and tree shapes of tests/adversarial_queries.py, on trees built by the device builders with the drawn Config: a root
that is a leaf, two leaves of one primitive, leaves of 9 to 15, coincident and degenerate primitives, a root box of zero extent on one
axis (flat) and on all of them (one point repeated) under forced SORTED.

Device == host harness (the kernels' text compiled by g++) byte for byte, counters included, under default flags, ORIGINAL_IDS and
forced SORTED; device == exact numpy on lattice points, without the harness; the rounded tier's property checks on the device's own
output; moving geometry, where the topology comes from other geometry than the one the tree is refitted to. Every output buffer is
written between two guard zones of sentinels. Nothing here needs the compiled reference."""
import numpy as np
import pytest

import adversarial_queries as adv
import test_closest_point_host as closest_host
import test_knn_host as knn_host
import test_overlap_host as overlap_host
import test_radius_search_host as radius_host
from test_gpu_overlap import _cuda, _np, _same, device_overlap, device_walk
from test_radius_search_host import GUARD, SENT_DIST, SENT_PRIM, Tree, dfs_prim_order

pytestmark = pytest.mark.gpu

ORIGINAL_IDS, SORTED = 8, 4
FLAGS = (0, ORIGINAL_IDS, SORTED)
KS = (1, 5, 64)
# the shapes and kinds dealt by the seed, and the degenerate root boxes with n > 1 whatever the deal gives
POINT_CASES = adv.cases(4, adv.EXACT_KINDS + adv.ROUNDED_KINDS, 12) + [
    ("flat", 200, (1, 8), (2, 0), np.float32, 451), ("flat", 65, (1, 1), (0, 2), np.float64, 452),
    ("one_point", 65, (1, 8), (3, 0), np.float32, 453), ("one_point", 200, (9, 15), (1, 2), np.float64, 454), ("one_point", 2, (1, 1), (0, 2), np.float32, 455)]
OVERLAP_CASES = adv.cases(5, ("lattice", "dups", "flat", "scales", "uniform", "points_lattice", "one_point", "spheres"), 8)


@pytest.fixture(scope="module")
def dlls(tmp_path_factory):
    d = tmp_path_factory.mktemp("query_fuzz_gpu")
    return {"closest": closest_host.compile_harness(d), "radius": radius_host.compile_harness(d), "knn": knn_host.compile_harness(d),
            "overlap": overlap_host.compile_harness(d)}


def device_build(bb, cc, lim, bq):
    import bvh_amd
    cfg = bvh_amd.Config(quality=bvh_amd.Quality(bq[1]), min_leaf_size=lim[0], max_leaf_size=lim[1])
    if bq[0] == 2:
        return bvh_amd.BinnedSahBuilder.build(bb, cc, cfg)
    if bq[0] == 3:
        return bvh_amd.SweepSahBuilder.build(bb, cc, cfg)
    return bvh_amd.DefaultBuilder.build(bb, cc, cfg, thread_pool=bvh_amd.ThreadPool() if bq[0] == 1 else None)


def check_shape(nodes, n, lim):
    dfs = dfs_prim_order(nodes["index"])
    assert len(dfs) == n and len(set(dfs.tolist())) == n
    assert int((nodes["index"].astype(np.uint64) & np.uint64(15)).max()) <= lim[1]
    if n == 1:
        assert len(nodes) == 1 and int(nodes["index"][0]) == 1
    return dfs


def _guarded(total, fill, dtype):
    """A device buffer of `total` entries between two guard zones of GUARD sentinels."""
    return _cuda(np.full(total + 2 * GUARD, fill, dtype=dtype))


def _inner(buf, total, fill, dtype):
    """The entries between the guard zones, as numpy; the guards must hold their sentinel."""
    a = _np(buf, dtype)
    assert (a[:GUARD] == fill).all() and (a[GUARD + total:] == fill).all()
    return a[GUARD:GUARD + total].copy()


class Device:
    """The C entry points of the point queries on one tree, every output between guard zones. -> numpy, shaped like the harnesses'."""

    def __init__(self, bvh, dprims, q, leaf):
        from bvh_amd import _lib
        self.lib, self.check = _lib.load(), _lib.last_error
        self.bvh, self.p, self.q, self.n = bvh, dprims, _cuda(q), len(q)
        self.dt, self.size = q.dtype, q.dtype.itemsize
        self.kind = "sphere" if leaf else "tri"

    def _cnt(self):
        import torch
        return torch.zeros(3, dtype=torch.int64, device="cuda")

    def closest(self, flags):
        rec = 4                                                # scalars per record
        out = _guarded(rec * self.n, SENT_DIST, self.dt)
        out[GUARD:GUARD + rec * self.n] = 0                    # (the double record's padding word is not written)
        cnt = self._cnt()
        f = getattr(self.lib, f"bvh{self.bvh._s}_closest_points_{self.kind}")
        assert f(self.bvh._h, self.p.data_ptr(), self.q.data_ptr(), self.n, flags, out.data_ptr() + GUARD * self.size, cnt.data_ptr(), None) == 0, self.check()
        hits = _inner(out, rec * self.n, SENT_DIST, self.dt).view(closest_host.HITD if self.dt == np.float64 else closest_host.HITF).reshape(-1)
        return hits, _np(cnt).astype(np.uint64)

    def radius(self, flags):
        import bvh_amd
        f = getattr(self.lib, f"bvh{self.bvh._s}_radius_search_{self.kind}")
        args = (self.bvh._h, self.p.data_ptr(), self.q.data_ptr(), self.n, flags)
        counts, cnt0 = _guarded(self.n, 0xABABABAB, np.uint32), self._cnt()
        assert f(*args, counts.data_ptr() + 4 * GUARD, None, None, None, cnt0.data_ptr(), None) == 0, self.check()
        c = _inner(counts, self.n, 0xABABABAB, np.uint32)
        offsets = bvh_amd.offsets_from_counts(_cuda(c))
        h_off = _np(offsets, np.uint64)
        total = int(h_off[-1])
        lp, ld, cnt = _guarded(total, SENT_PRIM, np.uint32), _guarded(total, SENT_DIST, self.dt), self._cnt()
        c2 = _guarded(self.n, 0xABABABAB, np.uint32)
        assert f(*args, c2.data_ptr() + 4 * GUARD, offsets.data_ptr(), lp.data_ptr() + 4 * GUARD, ld.data_ptr() + GUARD * self.size, cnt.data_ptr(), None) == 0, self.check()
        assert (_inner(c2, self.n, 0xABABABAB, np.uint32) == c).all() and (_np(cnt) == _np(cnt0)).all()
        return h_off, _inner(lp, total, SENT_PRIM, np.uint32), _inner(ld, total, SENT_DIST, self.dt), c, _np(cnt).astype(np.uint64)

    def knn(self, k, flags):
        f = getattr(self.lib, f"bvh{self.bvh._s}_knn_{self.kind}")
        ids, dist = _guarded(self.n * k, SENT_PRIM, np.uint32), _guarded(self.n * k, SENT_DIST, self.dt)
        counts, cnt = _guarded(self.n, 0xABABABAB, np.uint32), self._cnt()
        assert f(self.bvh._h, self.p.data_ptr(), self.q.data_ptr(), self.n, k, flags, ids.data_ptr() + 4 * GUARD, dist.data_ptr() + GUARD * self.size,
                 counts.data_ptr() + 4 * GUARD, cnt.data_ptr(), None) == 0, self.check()
        return (_inner(ids, self.n * k, SENT_PRIM, np.uint32).reshape(self.n, k), _inner(dist, self.n * k, SENT_DIST, self.dt).reshape(self.n, k),
                _inner(counts, self.n, 0xABABABAB, np.uint32), _np(cnt).astype(np.uint64))


def device_equals_host(dlls, bvh, dprims, q, leaf, lim, what):
    """Every point query under every flag against the harness on the tree read back from the device. -> (nodes, BVH-order prims, dfs,
    the device's results under default flags)."""
    nodes, ids, prims = bvh.nodes, bvh.prim_ids.astype(np.uint32), _np(dprims)
    dfs = check_shape(nodes, len(prims), lim)
    tree = Tree(nodes["bounds"], nodes["index"], prims, leaf)
    dev = Device(bvh, dprims, q, leaf)
    host, base = {}, None
    for original in (False, True):
        pid = ids if original else None
        host[original] = (closest_host.host_walk(dlls["closest"], nodes["bounds"], nodes["index"], prims, q, leaf, prim_ids=pid, threads=8),
                          radius_host.host_radius(dlls["radius"], tree, q, prim_ids=pid, threads=8),
                          {k: knn_host.host_knn(dlls["knn"], tree, q, k, prim_ids=pid, threads=8) for k in KS})
    for flags in FLAGS:
        h_closest, h_radius, h_knn = host[bool(flags & ORIGINAL_IDS)]
        hits, cnt = dev.closest(flags)
        assert hits.tobytes() == h_closest[0].tobytes(), (what, flags, "closest")
        assert (cnt == h_closest[1]).all(), (what, flags, cnt, h_closest[1])
        radius = dev.radius(flags)
        for name, d, h in zip(("offsets", "ids", "dist", "counts", "counters"), radius, h_radius):
            assert d.dtype == h.dtype and d.tobytes() == h.tobytes(), (what, flags, "radius", name)
        rows = {}
        for k in KS:
            rows[k] = dev.knn(k, flags)
            for name, d, h in zip(("ids", "dist", "counts", "counters"), rows[k], h_knn[k]):
                assert d.dtype == h.dtype and d.tobytes() == h.tobytes(), (what, flags, "knn", k, name)
        if flags == 0:
            base = (hits, radius[:4], {k: v[:3] for k, v in rows.items()})
    return nodes, prims, dfs, base


def check_exact(base, nodes, prims, q, dfs, what):
    """The device's results against the exact numpy expectations (lattice points), without the harness. -> adv.exact_witnesses."""
    hits, (offsets, lst, dist, counts), rows = base
    d2 = adv.exact_d2(prims[:, :3], q)
    prim, t, _ = adv.expect_closest(d2, q)
    assert (hits["prim"] == prim).all() and hits["t"].tobytes() == t.tobytes() and (hits["u"] == 0).all() and (hits["v"] == 0).all(), what
    e_off, e_ids, e_dist, e_counts = adv.expect_radius(d2, q, dfs)
    assert (counts == e_counts).all() and (offsets == e_off).all() and lst.tobytes() == e_ids.tobytes() and dist.tobytes() == e_dist.tobytes(), what
    for k, (ki, kd, kc) in rows.items():
        e_ki, e_kd, e_kc = adv.expect_knn(d2, q, k)
        assert ki.tobytes() == e_ki.tobytes() and kd.tobytes() == e_kd.tobytes() and (kc == e_kc).all(), (what, k)
    return adv.exact_witnesses(d2, q, adv.leaf_of_prims(nodes["index"], len(prims)))


def check_rounded(dlls, base, nodes, prims, leaf, raw, q, dfs, what):
    hits, radius, rows = base
    d2 = radius_host.host_brute(dlls["radius"], Tree(nodes["bounds"], nodes["index"], prims, leaf), q, threads=8)
    return adv.check_rounded(hits, radius, rows, d2, q, dfs, adv.host_tol(raw, prims.dtype), what)


@pytest.mark.parametrize("case", POINT_CASES, ids=adv.case_id)
def test_point_queries(dlls, case):
    import bvh_amd
    kind, n, lim, bq, dtype, seed = case
    rng = np.random.default_rng(seed)
    raw = adv.scene(rng, n, kind, dtype)
    exact = kind in adv.EXACT_KINDS
    q = adv.lattice_queries(rng, raw, dtype) if exact else adv.rounded_queries(rng, raw, dtype)
    leaf = 1 if raw.shape[1] == 4 else 0
    bb, cc = bvh_amd.sphere_bounds(raw) if leaf else bvh_amd.tri_bounds(raw)
    bvh = device_build(bb, cc, lim, bq)
    dprims = bvh_amd.gather(raw, bvh.device_prim_ids()) if leaf else bvh_amd.precompute_tris(raw, bvh.device_prim_ids())
    what = adv.case_id(case)
    nodes, prims, dfs, base = device_equals_host(dlls, bvh, dprims, q, leaf, lim, what)
    if kind in ("flat", "one_point"):                          # the degenerate root boxes that query_order scales its keys by
        ext = nodes["bounds"][0][1::2] - nodes["bounds"][0][0::2]
        assert (ext == 0).sum() == (3 if kind == "one_point" else 1)
    if exact:
        witnesses = check_exact(base, nodes, prims, q, dfs, what)
        if kind == "points_lattice" and n >= 17:               # not vacuous: distance exactly r, equal d2 across leaves, r = 0 on a primitive
            assert min(witnesses) > 0, (what, witnesses)
    else:
        check_rounded(dlls, base, nodes, prims, leaf, raw, q, dfs, what)


# ---- overlap ----------------------------------------------------------------------------------------------------------------------

def overlap_device_equals_host_and_numpy(dll, bvh, boxes, q, lim, what):
    """overlap_boxes under default flags, ORIGINAL_IDS and forced SORTED, overlap_self in both id modes: device == harness byte for
    byte, and == the numpy brute force exactly. -> self pairs."""
    nodes = bvh.nodes
    check_shape(nodes, bvh.prim_count, lim)
    tree = overlap_host.Tree(nodes["bounds"], nodes["index"], boxes, bvh.prim_ids)
    bb = _cuda(tree.bboxes)
    host = overlap_host.host_overlap(dll, tree, q, threads=8)
    want_counts, want_ids = overlap_host.expected_lists(overlap_host.brute(tree.ordered_boxes(), q), tree.dfs)
    assert (host[2] == want_counts).all() and host[1].tobytes() == want_ids.tobytes(), what
    _same(device_overlap(bvh, bb, q), host)
    _same(device_overlap(bvh, bb, q, flags=SORTED), host)
    _same(device_overlap(bvh, bb, q, flags=ORIGINAL_IDS), overlap_host.host_overlap(dll, tree, q, threads=8, original_ids=True))
    n, k, base = len(q), 3, 7                                  # k slots per query behind a non-zero base
    fixed = (base + k * np.arange(n + 1)).astype(np.uint64)
    _same(device_walk(bvh, bb, q, offsets=fixed, total=base + k * n + 5), overlap_host.host_walk(dll, tree, q, offsets=fixed, total=base + k * n + 5))
    within, (self_counts, self_ids) = overlap_host.self_expected(tree)
    host = overlap_host.host_overlap(dll, tree, None, threads=8)
    assert (host[2] == self_counts).all() and host[1].tobytes() == self_ids.tobytes(), what
    _same(device_overlap(bvh, bb, None), host)
    _same(device_overlap(bvh, bb, None, flags=ORIGINAL_IDS), overlap_host.host_overlap(dll, tree, None, threads=8, original_ids=True))
    return int(host[0][-1])


@pytest.mark.parametrize("case", OVERLAP_CASES, ids=adv.case_id)
def test_overlap_queries(dlls, case):
    kind, n, lim, bq, dtype, seed = case
    rng = np.random.default_rng(seed)
    boxes, centres = adv.adversarial_boxes(rng, adv.scene(rng, n, kind, dtype))
    bvh = device_build(boxes, centres, lim, bq)
    pairs = overlap_device_equals_host_and_numpy(dlls["overlap"], bvh, boxes, adv.box_queries(rng, boxes), lim, adv.case_id(case))
    print(f"{adv.case_id(case)}: {pairs} self pairs")
    assert n > 1 or pairs == 0
    if kind == "one_point":                                    # all coincident: every pair
        assert pairs == n * (n - 1) // 2


# ---- moving geometry: the topology of one scene, the geometry of another ----------------------------------------------------------

@pytest.mark.parametrize("lim", [(3, 15), (1, 1)], ids=["leaf3_15", "leaf1_1"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_moving_geometry_point_queries(dlls, lim, dtype):
    """Built on `uniform`, refit_tris to lattice points (exact tier on the returned BVH-order primitives), then to `dups` (rounded
    tier); device == harness on the re-read nodes both times."""
    import bvh_amd
    n = 1500
    rng = np.random.default_rng(61 + lim[1])
    first = adv.scene(rng, n, "uniform", dtype)
    bb, cc = bvh_amd.tri_bounds(first)
    bvh = device_build(bb, cc, lim, (0, 2))
    index0 = bvh.nodes["index"].copy()
    lattice = adv.scene(rng, n, "points_lattice", dtype)
    dprims = bvh.refit_tris(lattice)
    assert _np(dprims).tobytes() == _np(bvh_amd.precompute_tris(lattice, bvh.device_prim_ids())).tobytes()
    q = adv.lattice_queries(rng, lattice, dtype)
    nodes, prims, dfs, base = device_equals_host(dlls, bvh, dprims, q, 0, lim, ("lattice", lim))
    assert (nodes["index"] == index0).all()                    # the topology is still the uniform scene's
    assert min(check_exact(base, nodes, prims, q, dfs, ("lattice", lim))) > 0
    dups = adv.scene(rng, n, "dups", dtype)
    dprims = bvh.refit_tris(dups, out=dprims)
    q = adv.rounded_queries(rng, dups, dtype)
    nodes, prims, dfs, base = device_equals_host(dlls, bvh, dprims, q, 0, lim, ("dups", lim))
    check_rounded(dlls, base, nodes, prims, 0, dups, q, dfs, f"moving geometry, dups, leaves {lim}, {np.dtype(dtype).name}")


@pytest.mark.parametrize("lim", [(3, 15), (1, 1)], ids=["leaf3_15", "leaf1_1"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_moving_geometry_overlap(dlls, lim, dtype):
    """Built on `uniform`, tri_bounds + refit_boxes to lattice points and then to the adversarial boxes of `dups`: overlap lists and
    self pairs equal the numpy brute force exactly."""
    import bvh_amd
    n = 1500
    rng = np.random.default_rng(71 + lim[1])
    bb, cc = bvh_amd.tri_bounds(adv.scene(rng, n, "uniform", dtype))
    bvh = device_build(bb, cc, lim, (1, 2))
    lattice = adv.scene(rng, n, "points_lattice", dtype)
    mb, _ = bvh_amd.tri_bounds(lattice)
    bvh.refit_boxes(mb)
    boxes = _np(mb)
    assert (boxes == overlap_host.prim_boxes(lattice)).all()
    pairs = overlap_device_equals_host_and_numpy(dlls["overlap"], bvh, boxes, adv.box_queries(rng, boxes), lim, ("lattice", lim))
    assert pairs > n                                           # 1500 points on 125 lattice sites: coincident ones overlap
    boxes, _ = adv.adversarial_boxes(rng, adv.scene(rng, n, "dups", dtype))
    bvh.refit_boxes(boxes)
    pairs = overlap_device_equals_host_and_numpy(dlls["overlap"], bvh, boxes, adv.box_queries(rng, boxes), lim, ("dups", lim))
    assert pairs > 0
    full = overlap_host.brute(boxes, boxes)                    # by original id, no tree involved
    opairs = _np(bvh_amd.self_overlaps(bvh, boxes))
    want = {(min(a, b), max(a, b)) for a, b in zip(*np.nonzero(np.triu(full, 1)))}
    assert {(min(a, b), max(a, b)) for a, b in opairs.tolist()} == want and len(want) == len(opairs) == pairs
