"""MI355X: batched all-hits ray queries (bvh3X_intersect_rays_all_*, bvh_amd.ray_hit_count / ray_hits). The device's counts, records,
padding and counters are byte-equal to the host harness's (the same text compiled by g++, tests/test_ray_hits_host.py) and to the
reference set (tests/ray_hits_ref.py); block edges; count / offsets / fill against one pass into fixed slots; trees deeper than 64
levels; per-ray results do not depend on batch order, size, the reordering flags, the stream or the slicing of a launch; the relation
to closest-hit intersect; flags, errors and the Python layer."""
import ctypes as C

import numpy as np
import pytest

import oracle
from conftest import load_golden
from ray_hits_ref import INVALID, dense_tris, expected_lists, points_on, rays_through, reference_lib
from test_ray_hits_host import (GUARD, SENT_BYTE, chain, chain_rays, compile_harness, golden_case, guards_intact, hit_dtype, holds_closest, host_ray_hits,
                                host_walk, miss_record, seeded_case, untouched)

pytestmark = pytest.mark.gpu

ROBUST, SORTED, ORIGINAL_IDS, UNSORTED = 2, 4, 8, 16


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return compile_harness(tmp_path_factory.mktemp("ray_hits_gpu"))


@pytest.fixture(scope="module")
def lib():
    return reference_lib()


def _np(t, dtype=None):
    a = t.detach().cpu().numpy()
    return a if dtype is None else a.view(dtype)


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_bvh(tree, nodes, ids=None):
    import bvh_amd
    n = len(tree.prims)
    return bvh_amd.Bvh.from_nodes(np.ascontiguousarray(nodes), (np.arange(n) if ids is None else ids).astype(np.uint64))


def device_walk(bvh, tree, dprims, drays, flags=0, offsets=None, total=0, counts=True, counters=True, stream=None):
    """One call of bvh3X_intersect_rays_all_*: (counts or None, records WITH guard zones or None, counters)."""
    import torch
    from bvh_amd import _lib
    n = drays.shape[0]
    ht = hit_dtype(tree)
    c = _cuda(np.full(n + 2 * GUARD, 0xABABABAB, dtype=np.uint32)) if counts else None
    cnt = torch.zeros(3, dtype=torch.int64, device="cuda") if counters else None
    off = rec = None
    if offsets is not None:
        off = _cuda(np.ascontiguousarray(offsets, dtype=np.uint64).view(np.int64))
        rec = _cuda(np.full((total + 2 * GUARD) * ht.itemsize, SENT_BYTE, dtype=np.uint8))
        assert rec.data_ptr() % 32 == 0
    fn = getattr(_lib.load(), f"bvh{bvh._s}_intersect_rays_all_{'sphere' if tree.leaf else 'tri'}")
    rc = fn(bvh._h, dprims.data_ptr(), drays.data_ptr(), n, flags, c.data_ptr() + 4 * GUARD if counts else None, off.data_ptr() if off is not None else None,
            rec.data_ptr() + GUARD * ht.itemsize if rec is not None else None, cnt.data_ptr() if counters else None, stream)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    if counts:
        c = _np(c, np.uint32)
        assert (c[:GUARD] == 0xABABABAB).all() and (c[GUARD + n:] == 0xABABABAB).all()
        c = c[GUARD:GUARD + n]
    return c, None if rec is None else _np(rec).view(ht), None if cnt is None else _np(cnt).astype(np.uint64)


def device_ray_hits(bvh, tree, dprims, drays, flags=0):
    """Count, bvh_amd_offsets_from_counts, fill through the C ABI: (offsets, records, counts, counters of the fill pass)."""
    import bvh_amd
    counts, _, cnt0 = device_walk(bvh, tree, dprims, drays, flags)
    offsets = _np(bvh_amd.offsets_from_counts(_cuda(counts.view(np.int32)))).view(np.uint64)
    total = int(offsets[-1])
    c2, rec, cnt = device_walk(bvh, tree, dprims, drays, flags, offsets=offsets, total=total)
    assert (c2 == counts).all() and (cnt == cnt0).all() and guards_intact(rec, total)
    return offsets, rec[GUARD:GUARD + total], counts, cnt


def _same(dev, host):
    for d, h in zip(dev, host):
        assert d.tobytes() == h.tobytes()


@pytest.mark.parametrize("robust", [False, True])
@pytest.mark.parametrize("case", ["tri:1", "tri:2", "tri:3", "tri:200", "sphere:3", "sphere:200", "cornell", "soup2k", "terrain2k", "soup2k_f64", "spheres2k_f64"])
def test_device_equals_host_and_reference(dll, lib, orc, case, robust):
    if ":" in case:                                            # a seeded scene, kind:primitives
        kind, n_prims = case.split(":")
        tree, rays, ref, ids, nodes = seeded_case(lib, kind, int(n_prims))
    else:
        tree, rays, ref, ids, nodes = golden_case(lib, orc, case)
    bvh = device_bvh(tree, nodes, ids)
    dprims, drays = _cuda(tree.prims), _cuda(rays)
    flags = ROBUST if robust else 0
    host = host_ray_hits(dll, tree, rays, robust=robust, threads=8)
    dev = device_ray_hits(bvh, tree, dprims, drays, flags)
    _same(dev, host)
    want_counts, want = expected_lists(*ref[robust], tree.index)
    assert (dev[2] == want_counts).all() and dev[1].tobytes() == want.tobytes()        # the reference set, records byte for byte
    # ORIGINAL_IDS: the same walk, prim mapped
    o = device_ray_hits(bvh, tree, dprims, drays, flags | ORIGINAL_IDS)
    mapped = dev[1].copy()
    mapped["prim"] = ids[dev[1]["prim"].astype(np.int64)].astype(np.uint32)
    assert (o[0] == dev[0]).all() and o[1].tobytes() == mapped.tobytes() and (o[3] == dev[3]).all()
    # k slots per ray from a non-zero offset: prefix, padding with the miss record, untruncated counts, nothing outside the segments
    k, base, n = 2, 3, len(rays)
    fixed = (base + k * np.arange(n + 1)).astype(np.uint64)
    total = base + k * n + 5
    hc, hbuf, _ = host_walk(dll, tree, rays, robust=robust, offsets=fixed, total=total)
    dc, dbuf, _ = device_walk(bvh, tree, dprims, drays, flags, offsets=fixed, total=total)
    assert (dc == hc).all() and dbuf.tobytes() == hbuf.tobytes() and guards_intact(dbuf, total)
    assert untouched(dbuf[GUARD:GUARD + base]).all() and untouched(dbuf[GUARD + base + k * n:]).all()


@pytest.fixture(scope="module")
def dense(dll, lib):
    """The dense 200-triangle scene with 1023 rays, its host lists (fast test) and the device objects."""
    tree, _, _, ids, nodes = seeded_case(lib, "tri", 200)
    raw = dense_tris(200, 400)
    rays = np.concatenate([rays_through([0, 0, 0], [1, 1, 1], 512, 13, np.float32), rays_through([0, 0, 0], [1, 1, 1], 511, 14, np.float32, targets=points_on(raw, 511, 15))])
    host = host_ray_hits(dll, tree, rays, threads=8)
    return tree, nodes, ids, rays, host, device_bvh(tree, nodes, ids), _cuda(tree.prims)


@pytest.mark.parametrize("n", [1, 63, 64, 255, 256, 257, 1023])
def test_block_edges(dense, n):
    tree, _, _, rays, (h_off, h_rec, h_counts, _), bvh, dprims = dense
    off, rec, counts, _ = device_ray_hits(bvh, tree, dprims, _cuda(rays[:n]))
    assert (counts == h_counts[:n]).all() and off.tobytes() == h_off[:n + 1].tobytes() and rec.tobytes() == h_rec[:int(h_off[n])].tobytes()


def test_empty_batch_writes_nothing(dense):
    import torch
    from bvh_amd import _lib
    tree, _, _, rays, _, bvh, dprims = dense
    counts = _cuda(np.full(8, 0xABABABAB, dtype=np.uint32))
    offs = _cuda(np.full(8, 7, dtype=np.int64))
    rec = _cuda(np.full(8 * 16, SENT_BYTE, dtype=np.uint8))
    cnt = _cuda(np.full(3, 5, dtype=np.int64))
    rc = _lib.load().bvh3f_intersect_rays_all_tri(bvh._h, dprims.data_ptr(), None, 0, 0, counts.data_ptr(), offs.data_ptr(), rec.data_ptr(), cnt.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0
    assert (_np(counts, np.uint32) == 0xABABABAB).all() and (_np(offs) == 7).all() and (_np(rec) == SENT_BYTE).all() and (_np(cnt) == 5).all()


def test_two_pass_against_fixed_slots(dense):
    import bvh_amd
    import torch
    tree, _, _, rays, (h_off, h_rec, h_counts, h_cnt), bvh, dprims = dense
    n, k = len(rays), 4
    assert h_counts.max() > k and (h_counts < k).any()
    off, hits = bvh_amd.ray_hits(bvh, dprims, rays)
    assert _np(off, np.uint64).tobytes() == h_off.tobytes() and bvh_amd.hits_to_numpy(hits).tobytes() == h_rec.tobytes()
    off4, hits4, counts = bvh_amd.ray_hits(bvh, dprims, rays, max_per_ray=k)
    assert (_np(off4) == k * np.arange(n + 1)).all() and (_np(counts, np.uint32) == h_counts).all()      # untruncated
    rows = bvh_amd.hits_to_numpy(hits4).reshape(n, k)
    for i in range(n):
        m = min(int(h_counts[i]), k)
        assert rows[i, :m].tobytes() == h_rec[int(h_off[i]):int(h_off[i]) + m].tobytes()
        assert rows[i, m:].tobytes() == np.repeat(miss_record(tree, rays[i, 7]), k - m).tobytes()


@pytest.mark.parametrize("depth", [70, 300])
@pytest.mark.parametrize("stacked", [False, True])
def test_trees_deeper_than_64_levels(dll, restatement, depth, stacked):
    tree, nodes = chain(depth, restatement.prep_tris, stacked)
    bvh = device_bvh(tree, nodes)
    rays = chain_rays(depth, 300)                              # 300: not a multiple of the block; every 4th ray stacks on every level
    host = host_ray_hits(dll, tree, rays, deep_cap=depth - 64 + 1, threads=8)
    assert (host[2][::4] == depth + 1).all()
    _same(device_ray_hits(bvh, tree, _cuda(tree.prims), _cuda(rays)), host)
    _same(device_ray_hits(bvh, tree, _cuda(tree.prims), _cuda(rays), ROBUST), host_ray_hits(dll, tree, rays, robust=True, deep_cap=depth - 64 + 1, threads=8))


def test_sorted_equals_unsorted(dense):
    tree, _, ids, rays, host, bvh, dprims = dense
    odd = rays.copy()
    odd[3, 0] = np.nan                                         # origins and directions that are no number take a key like any other
    odd[9, 4] = np.nan
    odd[11, 3:6] = 0
    for r in (rays, odd):
        base = device_ray_hits(bvh, tree, dprims, _cuda(r), UNSORTED)
        if r is rays:
            _same(base, host)
        _same(device_ray_hits(bvh, tree, dprims, _cuda(r), SORTED), base)
        _same(device_ray_hits(bvh, tree, dprims, _cuda(r), 0), base)
        o = device_ray_hits(bvh, tree, dprims, _cuda(r), SORTED | ORIGINAL_IDS)
        assert (o[1]["prim"] == ids[base[1]["prim"].astype(np.int64)]).all() and (o[0] == base[0]).all() and (o[3] == base[3]).all()


def test_independent_of_position_stream_and_slicing(dll, dense):
    import torch
    from bvh_amd import _lib
    import query_slices as qs
    tree, _, _, rays, (h_off, h_rec, h_counts, _), bvh, dprims = dense
    lists = np.split(h_rec, h_off[1:-1].astype(np.int64))
    perm = np.random.default_rng(3).permutation(len(rays))
    off, rec, counts, _ = device_ray_hits(bvh, tree, dprims, _cuda(rays[perm]))
    assert (counts == h_counts[perm]).all() and rec.tobytes() == np.concatenate([lists[j] for j in perm]).tobytes()
    off, rec, counts, _ = device_ray_hits(bvh, tree, dprims, _cuda(np.repeat(rays[500:503], 100, axis=0)))      # one ray at many positions
    assert rec.tobytes() == np.concatenate([lists[500 + j // 100] for j in range(300)]).tobytes()
    # two streams at once on one const tree: count passes, then fill passes
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    parts = [rays[:600], rays[400:]]
    dparts = [_cuda(p) for p in parts]
    dcounts = [torch.zeros(len(p), dtype=torch.int32, device="cuda") for p in parts]
    f = _lib.load().bvh3f_intersect_rays_all_tri
    torch.cuda.synchronize()
    for s, d, c in zip(streams, dparts, dcounts):
        assert f(bvh._h, dprims.data_ptr(), d.data_ptr(), d.shape[0], 0, c.data_ptr(), None, None, None, C.c_void_p(s.cuda_stream)) == 0
    torch.cuda.synchronize()
    assert (_np(dcounts[0], np.uint32) == h_counts[:600]).all() and (_np(dcounts[1], np.uint32) == h_counts[400:]).all()
    offs = [np.concatenate([[0], np.cumsum(_np(c, np.uint32).astype(np.uint64))]).astype(np.uint64) for c in dcounts]
    bufs = [_cuda(np.full(max(int(o[-1]), 1) * 16, SENT_BYTE, dtype=np.uint8)) for o in offs]
    d_offs = [_cuda(o.view(np.int64)) for o in offs]
    torch.cuda.synchronize()
    for s, d, o, b in zip(streams, dparts, d_offs, bufs):
        assert f(bvh._h, dprims.data_ptr(), d.data_ptr(), d.shape[0], 0, None, o.data_ptr(), b.data_ptr(), None, C.c_void_p(s.cuda_stream)) == 0
    torch.cuda.synchronize()
    assert _np(bufs[0]).tobytes() == h_rec[:int(h_off[600])].tobytes()
    assert _np(bufs[1]).tobytes() == h_rec[int(h_off[400]):].tobytes()
    # a batch the launch path cuts in two (a chain of 4161 levels: the spill of a launch holds 16128 lanes): the same bytes as the host
    # walk, which knows nothing of launches
    depth = 4160
    tris, cnodes, _ = qs.chain(depth, np.float32, stacked=True)
    from test_closest_point_host import precompute
    from test_radius_search_host import Tree
    ctree = Tree(cnodes["bounds"], cnodes["index"], precompute(tris, np.float32), 0)
    per = qs.per_launch(depth, 4)
    n = per + 300
    crays = chain_rays(depth, n, base=qs.chain_base(depth), every=64)
    cbvh = device_bvh(ctree, cnodes)
    host = host_ray_hits(dll, ctree, crays, deep_cap=qs.deep_cap(depth), threads=16)
    dev = device_ray_hits(cbvh, ctree, _cuda(ctree.prims), _cuda(crays))
    assert _lib.load().bvh_amd_last_query_launches() == 2
    _same(dev, host)
    assert (host[2][::64] == depth + 1).all()


def test_relation_to_closest_hit(lib):
    """Whenever closest-hit intersect with the same ROBUST flag hits, the ray's list holds that record; whenever it misses, the list
    is empty. 4096 rays on the 2k soup (byte for byte) and on the 2k double spheres (prim and t0; t1 is clipped by closest-hit only)."""
    import bvh_amd
    import torch
    from bvh_amd import synth
    for scene in ("soup2k", "spheres2k_f64"):
        g = load_golden(scene)
        raw = g["prims"]
        sphere = raw.shape[1] == 4
        bvh = bvh_amd.Bvh.deserialize(g["bvh_parallel_high"].tobytes(), dtype=raw.dtype.type)
        dprims = bvh_amd.gather(raw, bvh.device_prim_ids()) if sphere else bvh_amd.precompute_tris(raw, bvh.device_prim_ids())
        lo, hi = synth.scene_bounds(raw)
        rays = np.concatenate([rays_through(lo, hi, 2048, 21, raw.dtype), rays_through(lo, hi, 2048, 22, raw.dtype, targets=points_on(raw, 2048, 23))])
        leaf = "sphere" if sphere else "tri"
        for robust in (False, True):
            closest = bvh_amd.hits_to_numpy(bvh_amd.intersect(bvh, dprims, rays, robust=robust, leaf=leaf))
            off, hits = bvh_amd.ray_hits(bvh, dprims, rays, leaf=leaf, robust=robust)
            off, hits = _np(off), bvh_amd.hits_to_numpy(hits)
            hit = closest["prim"] != INVALID
            assert hit.sum() > 1000 and (~hit).sum() > 100
            assert ((off[1:] - off[:-1] > 0) == hit).all()
            for r in np.flatnonzero(hit):
                assert holds_closest(hits[off[r]:off[r + 1]], closest[r], sphere), (scene, robust, r)


def test_refusals(dense):
    import bvh_amd
    import torch
    from bvh_amd import _lib
    tree, nodes, ids, rays, _, bvh, dprims = dense
    lib = _lib.load()
    n = len(rays)
    dr = _cuda(rays)
    counts = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    offs = torch.arange(n + 2, dtype=torch.int64, device="cuda") * 2
    rec = torch.zeros((2 * n + 8, 4), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    f = lib.bvh3f_intersect_rays_all_tri
    P = lambda t: t.data_ptr()

    def refused(rc, word):
        assert rc == -2 and word in _lib.last_error(), (rc, _lib.last_error())

    for ok in (0, ROBUST, SORTED | ROBUST | ORIGINAL_IDS, UNSORTED):
        assert f(bvh._h, P(dprims), P(dr), n, ok, P(counts), P(offs), P(rec), P(cnt), None) == 0, _lib.last_error()
    for bad in (1, 1 | ROBUST, 32, 1 << 20):                                                     # ANY_HIT, unknown bits
        refused(f(bvh._h, P(dprims), P(dr), n, bad, P(counts), None, None, None, None), "flags")
    refused(f(None, P(dprims), P(dr), n, 0, P(counts), None, None, None, None), "null bvh")
    refused(f(bvh._h, None, P(dr), n, 0, P(counts), None, None, None, None), "null device pointer")
    refused(f(bvh._h, P(dprims), None, n, 0, P(counts), None, None, None, None), "null device pointer")
    refused(f(bvh._h, P(dprims), P(dr), n, 0, None, None, None, None, None), "d_counts")         # neither counts nor offsets
    refused(f(bvh._h, P(dprims), P(dr), n, 0, P(counts), P(offs), None, None, None), "d_list_hits")      # offsets without records
    refused(f(bvh._h, P(dprims), P(dr), n, 0, P(counts), None, P(rec), None, None), "lists need d_offsets")
    for args in ((P(dprims) + 4, P(dr), n, 0, P(counts), None, None, None, None),                 # misaligned prims, rays, counts,
                 (P(dprims), P(dr) + 8, n - 1, 0, P(counts), None, None, None, None),             # offsets, records, counters
                 (P(dprims), P(dr), n, 0, P(counts) + 2, None, None, None, None),
                 (P(dprims), P(dr), n, 0, P(counts), P(offs) + 4, P(rec), None, None),
                 (P(dprims), P(dr), n, 0, P(counts), P(offs), P(rec) + 8, None, None),
                 (P(dprims), P(dr), n, 0, P(counts), None, None, P(cnt) + 4, None)):
        refused(f(bvh._h, *args), "aligned")
    # alignment to the element is enough: counts from their second entry, offsets and counters from theirs, records from the second record
    assert f(bvh._h, P(dprims), P(dr), n, 0, P(counts) + 4, P(offs) + 8, P(rec) + 16, P(cnt) + 8, None) == 0, _lib.last_error()
    # a 2D tree
    g2 = load_golden("circles2k_2f")
    b2, c2 = bvh_amd.sphere_bounds(g2["prims"])
    bvh2 = bvh_amd.DefaultBuilder.build(b2, c2)
    refused(f(bvh2._h, P(dprims), P(dr), n, 0, P(counts), None, None, None, None), "3D trees only")
    for call in (lambda: bvh_amd.ray_hit_count(bvh2, dprims, rays), lambda: bvh_amd.ray_hits(bvh2, dprims, rays),
                 lambda: bvh_amd.ray_hits(bvh, dprims, rays.astype(np.float64)), lambda: bvh_amd.ray_hit_count(bvh, _np(dprims).astype(np.float64), rays)):
        with pytest.raises(TypeError):
            call()
    with pytest.raises(ValueError):
        bvh_amd.ray_hits(bvh, dprims, rays, leaf="box")


def test_python_layer(dense):
    import bvh_amd
    import torch
    tree, _, ids, rays, (h_off, h_rec, h_counts, h_cnt), bvh, dprims = dense
    n = len(rays)
    c = bvh_amd.ray_hit_count(bvh, dprims, rays)
    assert c.dtype == torch.int32 and c.shape == (n,) and c.is_cuda and (_np(c, np.uint32) == h_counts).all()
    c, cnt = bvh_amd.ray_hit_count(bvh, dprims, _cuda(rays), sort_queries=True, counters=True)
    assert (_np(c, np.uint32) == h_counts).all() and cnt.dtype == torch.int64 and (_np(cnt).astype(np.uint64) == h_cnt).all()
    off, hits = bvh_amd.ray_hits(bvh, dprims, rays)
    assert off.dtype == torch.int64 and off.shape == (n + 1,) and hits.dtype == torch.float32 and hits.shape == (len(h_rec), 4) and hits.is_cuda
    assert _np(off, np.uint64).tobytes() == h_off.tobytes() and bvh_amd.hits_to_numpy(hits).tobytes() == h_rec.tobytes()
    off, ohits, cnt = bvh_amd.ray_hits(bvh, dprims, rays, original_ids=True, sort_queries=False, counters=True)
    assert (bvh_amd.hits_to_numpy(ohits)["prim"] == ids[h_rec["prim"].astype(np.int64)]).all() and (_np(cnt).astype(np.uint64) == h_cnt).all()
    off, hits, counts, cnt = bvh_amd.ray_hits(bvh, dprims, rays, max_per_ray=3, counters=True)
    assert hits.shape == (3 * n, 4) and counts.dtype == torch.int32 and (_np(counts, np.uint32) == h_counts).all() and cnt.shape == (3,)
    e_off, e_hits = bvh_amd.ray_hits(bvh, dprims, np.zeros((0, 8), np.float32))
    assert e_off.tolist() == [0] and e_hits.shape == (0, 4) and bvh_amd.ray_hit_count(bvh, dprims, np.zeros((0, 8), np.float32)).shape == (0,)
    far = rays.copy()
    far[:, :3] += 1000
    far[:, 3:6] = [1, 0, 0]
    z_off, z_hits = bvh_amd.ray_hits(bvh, dprims, far, robust=True)
    assert z_off.tolist() == [0] * (n + 1) and z_hits.shape == (0, 4)
    # double spheres: (m, 4) float64 records
    tree_s, rays_s, _, _, nodes_s = seeded_case(reference_lib(), "sphere", 200)
    bvh_s = device_bvh(tree_s, nodes_s)
    off, hits = bvh_amd.ray_hits(bvh_s, tree_s.prims, rays_s, leaf="sphere", robust=True)
    rec = bvh_amd.hits_to_numpy(hits)
    assert hits.dtype == torch.float64 and rec.dtype == oracle.HITD and (rec["pad"] == 0).all() and (rec["v"] == 0).all() and (rec["t"] <= rec["u"]).all()
