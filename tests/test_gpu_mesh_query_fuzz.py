"""MI355X: sphere_cast, tri_distance, region_* and winding_* on the adversarial scenes, tree shapes and batches of
tests/adversarial_mesh_queries.py (the cases of tests/test_mesh_query_fuzz_host.py and the degenerate root boxes with n > 1), on trees
built by the device builders with the drawn Config: a root that is a leaf, two leaves of one primitive, leaves of 9 to 15, a root box
of zero extent on one axis (flat) and on all of them (one point repeated) under forced SORTED.

Every query goes through its C entry point with every output (records, query barycentrics, winding values, moments, region counts,
lists and inside bytes, counters) written between two guard zones of sentinels. Device == host harness (the kernels' text compiled by
g++) byte for byte, counters included, under every legal flag set; then, without the harness in between: tri_distance on lattice
points against numpy, region CULL against region_ref.brute_cull, winding's dyadic tier against winding_ref64, and the sphere-cast
residual / no-miss checks on the device's own ROBUST records. One test moves the geometry under a fixed topology. Nothing here needs
the compiled reference."""
import math

import numpy as np
import pytest

import adversarial_mesh_queries as amq
import adversarial_queries as adv
import region_ref as R
import test_sphere_cast_host as cast_host
import test_tri_distance_host as dist_host
import test_winding_host as wind_host
import tri_intersect_ref as TR
from test_closest_point_host import HITD, HITF
from test_gpu_overlap import _cuda, _np
from test_gpu_query_fuzz import _guarded, _inner, check_shape, device_build
from test_mesh_query_fuzz_host import CLEARANCE, ROUNDED_MEASURED
from test_radius_search_host import GUARD, SENT_DIST, SENT_PRIM

pytestmark = pytest.mark.gpu

INVALID = adv.INVALID
ROBUST, SORTED, ORIGINAL_IDS, UNSORTED, EXACT = 2, 4, 8, 16, R.REGION_EXACT
CAST_FLAGS = (0, ROBUST, SORTED, SORTED | ROBUST | ORIGINAL_IDS)
DISTANCE_FLAGS = (0, SORTED, ORIGINAL_IDS)
REGION_FLAGS = (0, EXACT, ORIGINAL_IDS, EXACT | ORIGINAL_IDS)
WINDING_FLAGS = (UNSORTED, SORTED)
COUNTS_FILL, SENT_COUNTER = 0xABABABAB, 0x5A5A5A5A5A5A5A5A
HOST_THREADS = 8

CAST_CASES = amq.CAST_CASES + amq.DEGENERATE_ROOTS
DISTANCE_CASES = amq.DISTANCE_EXACT_CASES + amq.DISTANCE_CASES + amq.DEGENERATE_ROOTS
REGION_CASES = amq.REGION_CASES + amq.DEGENERATE_ROOTS
WINDING_CASES = amq.WINDING_CASES + amq.DEGENERATE_ROOTS


@pytest.fixture(scope="module")
def dlls(tmp_path_factory):
    d = tmp_path_factory.mktemp("mesh_query_fuzz_gpu")
    return {"cast": cast_host.compile_harness(d), "distance": dist_host.compile_harness(d), "region": R.compile_harness(d),
            "winding": wind_host.compile_harness(d)}


class Device:
    """The C entry points of the four queries on one tree, every output between guard zones. -> numpy, shaped like the harnesses'."""

    def __init__(self, bvh, dtype):
        from bvh_amd import _lib
        self.lib, self.check, self.bvh = _lib.load(), _lib.last_error, bvh
        self.dt, self.size = np.dtype(dtype), np.dtype(dtype).itemsize

    def f(self, name):
        return getattr(self.lib, f"bvh{self.bvh._s}_{name}")

    def _counters(self):
        buf = _guarded(3, SENT_COUNTER, np.uint64)
        buf[GUARD:GUARD + 3] = 0
        return buf

    def _records(self, n):
        out = _guarded(4 * n, SENT_DIST, self.dt)
        out[GUARD:GUARD + 4 * n] = 0                           # (the double record's padding word is not written)
        return out

    def _read(self, rec, n, cnt):
        hits = _inner(rec, 4 * n, SENT_DIST, self.dt).view(HITD if self.dt == np.float64 else HITF).reshape(-1)
        return hits, _inner(cnt, 3, SENT_COUNTER, np.uint64)

    def cast(self, dprims, leaf, rays, radii, flags):
        n = len(rays)
        rec, cnt, dr, drad = self._records(n), self._counters(), _cuda(rays), _cuda(radii)
        rc = self.f("sphere_cast_sphere" if leaf else "sphere_cast_tri")(self.bvh._h, dprims.data_ptr(), dr.data_ptr(), n, 0.0, drad.data_ptr(), flags,
                                                                          rec.data_ptr() + GUARD * self.size, cnt.data_ptr() + 8 * GUARD, None)
        assert rc == 0, self.check()
        return self._read(rec, n, cnt)

    def distance(self, dtris, q, lim, flags):
        n = len(q)
        rec, cnt, uv = self._records(n), self._counters(), _guarded(2 * n, SENT_DIST, self.dt)
        dq, dl = _cuda(q), _cuda(lim)
        rc = self.f("tri_distance")(self.bvh._h, dtris.data_ptr(), dtris.shape[0], dq.data_ptr(), n, 0.0, dl.data_ptr(), flags,
                                    rec.data_ptr() + GUARD * self.size, uv.data_ptr() + GUARD * self.size, cnt.data_ptr() + 8 * GUARD, None)
        assert rc == 0, self.check()
        hits, c = self._read(rec, n, cnt)
        return hits, _inner(uv, 2 * n, SENT_DIST, self.dt).reshape(n, 2), c

    def _region_call(self, dprims, leaf, dq, flags, offsets, total, inside):
        n, m = dq.shape[0], dq.shape[1]
        counts, cnt = _guarded(n, COUNTS_FILL, np.uint32), self._counters()
        off = lp = li = None
        if offsets is not None:
            off = _cuda(np.ascontiguousarray(offsets, dtype=np.uint64))
            lp = _guarded(total, SENT_PRIM, np.uint32)
            li = _guarded(total, R.SENT_INSIDE, np.uint8) if inside else None
        P = lambda t, skip=0: None if t is None else t.data_ptr() + skip
        rc = self.f("region_spheres" if leaf else "region_tris")(self.bvh._h, dprims.data_ptr(), dprims.shape[0], dq.data_ptr(), m, n, flags,
                                                                 P(counts, 4 * GUARD), P(off), P(lp, 4 * GUARD), P(li, GUARD), P(cnt, 8 * GUARD), None)
        assert rc == 0, self.check()
        return (_inner(counts, n, COUNTS_FILL, np.uint32), None if lp is None else _inner(lp, total, SENT_PRIM, np.uint32),
                None if li is None else _inner(li, total, R.SENT_INSIDE, np.uint8), _inner(cnt, 3, SENT_COUNTER, np.uint64))

    def region(self, dprims, leaf, planes, flags):
        """The count pass, bvh_amd.offsets_from_counts, the fill pass with inside flags: what region_ref.host_region returns."""
        import bvh_amd
        dq = _cuda(planes)
        counts, _, _, cnt0 = self._region_call(dprims, leaf, dq, flags, None, 0, False)
        offsets = _np(bvh_amd.offsets_from_counts(_cuda(counts)), np.uint64)
        total = int(offsets[-1])
        c2, ids, ins, cnt = self._region_call(dprims, leaf, dq, flags, offsets, total, True)
        assert (c2 == counts).all() and (cnt == cnt0).all()
        return offsets, ids, ins, counts, cnt

    def region_fixed(self, dprims, leaf, planes, flags, k=3, base=7):
        """k slots per query behind a non-zero base. -> (counts, the whole list buffer, the inside bytes, offsets, total)."""
        n = len(planes)
        fixed = (base + k * np.arange(n + 1)).astype(np.uint64)
        total = base + k * n + 5
        counts, lp, li, _ = self._region_call(dprims, leaf, _cuda(planes), flags, fixed, total, True)
        return counts, lp, li, fixed, total

    def prepare(self, dprims):
        rows = self.bvh.node_count + 1
        mom = _guarded(8 * rows, SENT_DIST, self.dt)
        assert self.f("winding_prepare")(self.bvh._h, dprims.data_ptr(), mom.data_ptr() + GUARD * self.size, rows, None) == 0, self.check()
        return mom, _inner(mom, 8 * rows, SENT_DIST, self.dt).reshape(rows, 8)

    def winding(self, dprims, mom, q4, beta, flags):
        n, rows = len(q4), self.bvh.node_count + 1
        w, cnt, dq = _guarded(n, SENT_DIST, self.dt), self._counters(), _cuda(q4)
        rc = self.f("winding_numbers")(self.bvh._h, dprims.data_ptr(), mom.data_ptr() + GUARD * self.size, rows, dq.data_ptr(), n, beta, flags,
                                       w.data_ptr() + GUARD * self.size, None, cnt.data_ptr() + 8 * GUARD, None)
        assert rc == 0, self.check()
        return _inner(w, n, SENT_DIST, self.dt), _inner(cnt, 3, SENT_COUNTER, np.uint64)


def build(case):
    """The scene of a case and its tree from the drawn device builder: (raw, Bvh, nodes, prim ids, leaf)."""
    import bvh_amd
    kind, n, lim, bq, dtype, seed = case
    raw = adv.scene(np.random.default_rng(seed), n, kind, dtype)
    leaf = 1 if raw.shape[1] == 4 else 0
    bb, cc = bvh_amd.sphere_bounds(raw) if leaf else bvh_amd.tri_bounds(raw)
    bvh = device_build(bb, cc, lim, bq)
    nodes = bvh.nodes
    check_shape(nodes, n, lim)
    if kind in ("flat", "one_point"):                          # the degenerate root boxes that query_order scales its keys by
        ext = nodes["bounds"][0][1::2] - nodes["bounds"][0][0::2]
        assert (ext == 0).sum() == (3 if kind == "one_point" else 1)
    return raw, bvh, nodes, bvh.prim_ids.astype(np.uint32), leaf


def _rng(case, salt):
    return np.random.default_rng([case[5], salt])


# ---- sphere_cast ----------------------------------------------------------------------------------------------------------------------------

def cast_checks(dll, bvh, nodes, ids, dprims, leaf, raw, rays, radii, marks, what, cap=0.02):
    """Device == harness under CAST_FLAGS; then the fuzz's property checks on the device's own ROBUST and fast records."""
    prims = _np(dprims)
    dev = Device(bvh, prims.dtype)
    got = {}
    for flags in CAST_FLAGS:
        hits, cnt = dev.cast(dprims, leaf, rays, radii, flags)
        h_hits, h_cnt = cast_host.host_walk(dll, nodes["bounds"], nodes["index"], prims, rays, radii, leaf, robust=bool(flags & ROBUST),
                                            prim_ids=ids if flags & ORIGINAL_IDS else None, threads=HOST_THREADS)
        assert hits.tobytes() == h_hits.tobytes(), (what, flags, np.flatnonzero((hits["prim"] != h_hits["prim"]) | (hits["t"] != h_hits["t"]))[:8])
        assert (cnt == h_cnt).all(), (what, flags, cnt, h_cnt)
        got[flags] = hits
    brute, _ = cast_host.host_brute(dll, prims, rays, radii, leaf)
    tol = cast_host.TOL[prims.dtype.type]
    out = amq.check_cast(raw, ids, rays, radii, marks, got[ROBUST], brute, leaf == 1, ~marks["negative"], tol, (what, "robust"), cap=cap)
    amq.check_cast(raw, ids, rays, radii, marks, got[0], brute, leaf == 1, ~marks["negative"] & ~marks["zero"], tol, (what, "fast"), cap=cap)
    return out


@pytest.mark.parametrize("case", CAST_CASES, ids=adv.case_id)
def test_sphere_cast(dlls, case):
    import bvh_amd
    kind, n, lim, bq, dtype, seed = case
    raw, bvh, nodes, ids, leaf = build(case)
    dprims = bvh_amd.gather(raw, bvh.device_prim_ids()) if leaf else bvh_amd.precompute_tris(raw, bvh.device_prim_ids())
    rays, radii, marks = amq.rays(_rng(case, 1), raw, dtype)
    found, differ, res = cast_checks(dlls["cast"], bvh, nodes, ids, dprims, leaf, raw, rays, radii, marks, adv.case_id(case))
    print(f"{adv.case_id(case)}: ROBUST {found} hits, {differ} records differ from the brute force, residual/scale {res:.3e}")
    assert found > 0
    lo, hi, diag = adv.scene_extent(raw)
    if (hi == lo).any():
        rays, radii, marks = amq.rays(_rng(case, 6), raw, dtype, floor=diag if diag > 0 else 1.0)
        cast_checks(dlls["cast"], bvh, nodes, ids, dprims, leaf, raw, rays, radii, marks, (adv.case_id(case), "from afar"), cap=None)


# ---- tri_distance ---------------------------------------------------------------------------------------------------------------------------

def distance_device_equals_host(dll, bvh, tree, q, lim, what):
    """Device == harness under DISTANCE_FLAGS. -> the device's (records, query barycentrics) under default flags."""
    dev = Device(bvh, tree.dtype)
    dtris = _cuda(tree.tris)
    base = None
    for flags in DISTANCE_FLAGS:
        hits, uv, cnt = dev.distance(dtris, q, lim, flags)
        h_hits, h_uv, h_cnt = dist_host.host_walk(dll, tree, q, lim, original_ids=bool(flags & ORIGINAL_IDS), threads=HOST_THREADS)
        assert hits.tobytes() == h_hits.tobytes(), (what, flags, np.flatnonzero((hits["prim"] != h_hits["prim"]) | (hits["t"] != h_hits["t"]))[:8])
        assert uv.tobytes() == h_uv.tobytes() and (cnt == h_cnt).all(), (what, flags, cnt, h_cnt)
        if flags == 0:
            base = (hits, uv)
    return base


def distance_checks(dll, bvh, nodes, ids, raw, kind, rng, what):
    """Lattice points: the device against numpy, no harness in between. Otherwise amq.check_distance on the device's records."""
    tree = TR.TriTree(nodes["bounds"], nodes["index"], raw, ids)
    dtype = raw.dtype.type
    if kind in adv.EXACT_KINDS:
        q4 = adv.lattice_queries(rng, raw, dtype)
        q, lim = np.ascontiguousarray(np.tile(q4[:, :3], (1, 3))), np.ascontiguousarray(q4[:, 3])
        hits, uv = distance_device_equals_host(dll, bvh, tree, q, lim, what)
        d2 = adv.exact_d2(tree.ordered_tris()[:, :3], q4)
        prim, t, _ = adv.expect_closest(d2, q4)
        assert (hits["prim"] == prim).all() and hits["t"].tobytes() == t.tobytes(), what
        assert (hits["u"] == 0).all() and (hits["v"] == 0).all() and (uv == 0).all(), what
        return adv.exact_witnesses(d2, q4, adv.leaf_of_prims(nodes["index"], len(raw)))
    q, lim, _ = amq.query_tris(rng, raw, dtype)
    hits, uv = distance_device_equals_host(dll, bvh, tree, q, lim, what)
    brute, _, second = dist_host.host_brute(dll, tree, q, lim)
    amq.check_distance(q, lim, tree.ordered_tris(), hits, uv, brute, second, dist_host.TOL[dtype], what)
    return None


@pytest.mark.parametrize("case", DISTANCE_CASES, ids=adv.case_id)
def test_tri_distance(dlls, case):
    kind, n, lim, bq, dtype, seed = case
    raw, bvh, nodes, ids, leaf = build(case)
    witnesses = distance_checks(dlls["distance"], bvh, nodes, ids, raw, kind, _rng(case, 2 if kind in adv.EXACT_KINDS else 3), adv.case_id(case))
    if kind == "points_lattice" and n >= 17:
        assert min(witnesses) > 0, witnesses


# ---- region ---------------------------------------------------------------------------------------------------------------------------------

def region_checks(dll, bvh, tree, planes, what):
    """Device == harness under REGION_FLAGS (count pass, fill pass, k = 3 fixed slots behind a base); CULL against brute_cull."""
    dev = Device(bvh, tree.dtype)
    dprims = _cuda(tree.prims)
    pairs_exact = lambda pr, pl: R.host_pairs(dll, pr, pl, tree.dtype)[1]
    listed = 0
    for flags in REGION_FLAGS:
        if flags & EXACT and tree.leaf == 1:
            continue
        exact, original = bool(flags & EXACT), bool(flags & ORIGINAL_IDS)
        got = dev.region(dprims, tree.leaf, planes, flags)
        host = R.host_region(dll, tree, planes, exact=exact, original_ids=original, threads=HOST_THREADS)
        for name, d, h in zip(("offsets", "ids", "inside", "counts", "counters"), got, host):
            assert d.dtype == h.dtype and d.tobytes() == h.tobytes(), (what, flags, name)
        if not original:
            listed += amq.check_region(tree, planes, got[:4], exact, pairs_exact, (what, flags))[0]
        counts, lp, li, fixed, total = dev.region_fixed(dprims, tree.leaf, planes, flags)
        hc, hlp, hli, _ = R.host_walk(dll, tree, planes, exact=exact, original_ids=original, offsets=fixed, total=total, inside=True)
        assert (counts == hc).all() and lp.tobytes() == hlp[GUARD:GUARD + total].tobytes() and li.tobytes() == hli[GUARD:GUARD + total].tobytes(), (what, flags)
    return listed


@pytest.mark.parametrize("case", REGION_CASES, ids=adv.case_id)
def test_region(dlls, case):
    kind, n, lim, bq, dtype, seed = case
    raw, bvh, nodes, ids, leaf = build(case)
    tree = R.PrimTree(nodes["bounds"], nodes["index"], raw, ids)
    listed = 0
    for m in (1, 6):
        listed += region_checks(dlls["region"], bvh, tree, R.make_regions(raw, 192, m, dtype, seed + m), (adv.case_id(case), m))
    assert listed > 0
    if kind in amq.LATTICE_KINDS or kind == "spheres":
        planes = amq.lattice_regions(_rng(case, 4 + 3), raw, dtype, 192, 3)
        assert amq.planes_through_vertices(raw, planes) > 0
        region_checks(dlls["region"], bvh, tree, planes, (adv.case_id(case), "lattice"))


# ---- winding --------------------------------------------------------------------------------------------------------------------------------

def winding_checks(dll, bvh, nodes, dprims, raw, kind, pts, what):
    """winding_prepare twice (the same bytes, == the harness's, (node_count + 1, 8)), winding_numbers == harness for every beta under
    WINDING_FLAGS; beta = inf against winding_ref64 (the dyadic tier: every query, 16 eps n), exactly 0 on scenes without area."""
    prims = _np(dprims)
    dt = prims.dtype.type
    dev = Device(bvh, dt)
    mom_buf, mom = dev.prepare(dprims)
    assert mom.shape == (len(nodes) + 1, 8) and np.isfinite(mom).all()
    assert dev.prepare(dprims)[1].tobytes() == mom.tobytes(), what
    assert mom.tobytes() == wind_host.host_prepare(dll, nodes["bounds"], nodes["index"], prims, threads=HOST_THREADS).tobytes(), what
    q = wind_host.queries4(pts, dt)
    for beta in wind_host.BETAS:
        h_w, h_cnt = wind_host.host_walk(dll, nodes["bounds"], nodes["index"], prims, mom, q, beta=beta, threads=HOST_THREADS)
        for flags in WINDING_FLAGS:
            w, cnt = dev.winding(dprims, mom_buf, q, beta, flags)
            assert w.tobytes() == h_w.tobytes(), (what, beta, flags)
            assert (cnt == h_cnt).all(), (what, beta, flags, cnt, h_cnt)
        assert np.isfinite(w).all(), (what, beta)
        if kind in amq.AREALESS_KINDS:
            assert (w == 0).all(), (what, beta)
        if math.isinf(beta):
            ref = amq.winding_ref64(raw, q)
            if kind in amq.DYADIC_WINDING:
                keep, bound = np.ones(len(q), dtype=bool), 16 * float(np.finfo(dt).eps) * len(prims)
            else:
                keep = amq.clear_of_surface(raw, q, CLEARANCE)
                bound = max(16 * float(np.finfo(dt).eps) * len(prims), 4 * ROUNDED_MEASURED[dt])
                assert (~keep).mean() <= 0.05, what
            err = np.abs(w.astype(np.float64) - ref)[keep]
            assert err.max() <= bound, (what, float(err.max()), bound)


@pytest.mark.parametrize("case", WINDING_CASES, ids=adv.case_id)
def test_winding(dlls, case):
    import bvh_amd
    kind, n, lim, bq, dtype, seed = case
    raw, bvh, nodes, ids, leaf = build(case)
    dprims = bvh_amd.precompute_tris(raw, bvh.device_prim_ids())
    pts = amq.winding_points(_rng(case, 5), raw, kind, dtype)
    winding_checks(dlls["winding"], bvh, nodes, dprims, raw, kind, pts, adv.case_id(case))


# ---- moving geometry: the topology of one scene, the geometry of another ----------------------------------------------------------------------

@pytest.mark.parametrize("lim", [(3, 15), (1, 1)], ids=["leaf3_15", "leaf1_1"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_moving_geometry(dlls, lim, dtype):
    """Built on `uniform`, refit_tris to lattice points, then to `dups`: all four queries against the harness on the re-read nodes both
    times (winding with fresh moments), the topology words unchanged."""
    import bvh_amd
    n = 1500
    rng = np.random.default_rng(81 + lim[1])
    first = adv.scene(rng, n, "uniform", dtype)
    bb, cc = bvh_amd.tri_bounds(first)
    bvh = device_build(bb, cc, lim, (0, 2))
    index0 = bvh.nodes["index"].copy()
    ids = bvh.prim_ids.astype(np.uint32)
    dprims = None
    for case in amq.MOVING_CASES[(lim, np.dtype(dtype).name)]:
        kind = case[0]
        raw = adv.scene(np.random.default_rng(case[5]), n, kind, dtype)
        dprims = bvh.refit_tris(raw, out=dprims)
        assert _np(dprims).tobytes() == _np(bvh_amd.precompute_tris(raw, bvh.device_prim_ids())).tobytes()
        nodes = bvh.nodes
        assert (nodes["index"] == index0).all()               # the topology is still the uniform scene's
        check_shape(nodes, n, lim)
        what = ("moving", kind, lim, np.dtype(dtype).name)
        rays, radii, marks = amq.rays(_rng(case, 1), raw, dtype)
        cast_checks(dlls["cast"], bvh, nodes, ids, dprims, 0, raw, rays, radii, marks, what)
        witnesses = distance_checks(dlls["distance"], bvh, nodes, ids, raw, kind, _rng(case, 3), what)
        assert witnesses is None or min(witnesses) > 0, witnesses
        tree = R.PrimTree(nodes["bounds"], nodes["index"], raw, ids)
        planes = amq.lattice_regions(_rng(case, 4), raw, dtype, 192, 3) if kind == "points_lattice" else R.make_regions(raw, 192, 6, dtype, 5)
        assert region_checks(dlls["region"], bvh, tree, planes, what) > 0
        winding_checks(dlls["winding"], bvh, nodes, dprims, raw, kind, amq.winding_points(_rng(case, 5), raw, kind, dtype), what)
