"""MI355X: batched nearest-hits ray queries (bvh3X_intersect_rays_nearest_*, bvh_amd.ray_hits_nearest). The device's rows, counts and
counters are byte-equal to the host harness's (the same text compiled by g++, tests/test_ray_nearest_host.py) and to the rows derived
from the unmodified reference (tests/ray_nearest_ref.py), with guard zones around the device buffers; block edges at the three
block sizes; a ray's row does not depend on batch order, size, the reordering flags, the stream or the slicing of a launch; k = 1
against bvh_amd.intersect and k = 64 against sorted bvh_amd.ray_hits; flags, errors and the Python layer."""
import ctypes as C

import numpy as np
import pytest

import oracle
import query_slices as qs
from conftest import load_golden
from ray_hits_ref import INVALID, dense_tris, points_on, rays_through, reference_lib
from ray_nearest_ref import (GUARD, K_DENSE, K_TINY, SENT_BYTE, SENT_COUNT, block_lanes, compile_harness, differing_rows, expected_rows, first_two_tie,
                             grid_case, hit_dtype, host_nearest, record_guards_intact, sorted_lists)
from test_ray_hits_host import chain, chain_rays, golden_case, seeded_case

pytestmark = pytest.mark.gpu

ROBUST, SORTED, ORIGINAL_IDS, UNSORTED = 2, 4, 8, 16


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return compile_harness(tmp_path_factory.mktemp("ray_nearest_gpu"))


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


def device_nearest(bvh, tree, dprims, drays, k, flags=0, counts=True, counters=True, stream=None):
    """One call of bvh3X_intersect_rays_nearest_*: (rows (n, k), counts or None, counters or None). Rows and counts sit between guard
    zones on the device, which must come back untouched."""
    import torch
    from bvh_amd import _lib
    n = drays.shape[0]
    ht = hit_dtype(tree)
    c = _cuda(np.full(n + 2 * GUARD, SENT_COUNT, dtype=np.uint32)) if counts else None
    cnt = torch.zeros(3, dtype=torch.int64, device="cuda") if counters else None
    rec = _cuda(np.full((n * k + 2 * GUARD) * ht.itemsize, SENT_BYTE, dtype=np.uint8))
    assert rec.data_ptr() % 32 == 0
    fn = getattr(_lib.load(), f"bvh{bvh._s}_intersect_rays_nearest_{'sphere' if tree.leaf else 'tri'}")
    rc = fn(bvh._h, dprims.data_ptr(), drays.data_ptr(), n, k, flags, rec.data_ptr() + GUARD * ht.itemsize, c.data_ptr() + 4 * GUARD if counts else None,
            cnt.data_ptr() if counters else None, stream)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    buf = _np(rec).view(ht)
    assert record_guards_intact(buf, n * k)
    if counts:
        c = _np(c, np.uint32)
        assert (c[:GUARD] == SENT_COUNT).all() and (c[GUARD + n:] == SENT_COUNT).all()
        c = c[GUARD:GUARD + n]
    return buf[GUARD:GUARD + n * k].reshape(n, k), c, None if cnt is None else _np(cnt).astype(np.uint64)


def _same(dev, host):
    for d, h in zip(dev, host):
        assert d.tobytes() == h.tobytes()


@pytest.mark.parametrize("robust", [False, True])
@pytest.mark.parametrize("case", ["tri:1", "tri:2", "tri:3", "tri:200", "sphere:1", "sphere:2", "sphere:3", "sphere:200", "grid", "cornell", "soup2k",
                                  "terrain2k", "soup2k_f64", "spheres2k_f64"])
def test_device_equals_host_and_reference(dll, lib, orc, case, robust):
    tiny = False
    if case == "grid":
        tree, rays, ref, ids, nodes = grid_case(lib)
    elif ":" in case:                                          # a seeded scene, kind:primitives
        kind, n_prims = case.split(":")
        tree, rays, ref, ids, nodes = seeded_case(lib, kind, int(n_prims))
        tiny = int(n_prims) < 200
    else:
        tree, rays, ref, ids, nodes = golden_case(lib, orc, case)
    bvh = device_bvh(tree, nodes, ids)
    dprims, drays = _cuda(tree.prims), _cuda(rays)
    flags = ROBUST if robust else 0
    all_counts, sorted_ = sorted_lists(*ref[robust], tree.index)
    for k in (K_TINY if tiny else K_DENSE):
        host = host_nearest(dll, tree, rays, k, robust=robust, threads=8)
        dev = device_nearest(bvh, tree, dprims, drays, k, flags)
        _same(dev, host)
        want, want_counts = expected_rows(tree, rays, sorted_, k)
        assert differing_rows(dev[0], want) == 0 and (dev[1] == want_counts).all()      # the reference's rows, byte for byte
    # the cases count where the reference's own lists show that k cuts rows (tests/test_ray_nearest_host.py has the reasons)
    cut = {k: int((all_counts > k).sum()) for k in K_DENSE}
    if case in ("tri:200", "sphere:200"):
        assert all(cut[k] > 0 for k in (1, 2, 3, 8, 9, 16, 17, 33)) and cut[64] == 0, cut
    if case == "grid":
        assert first_two_tie(sorted_).sum() >= len(rays) // 4
        assert all(cut[k] > 0 for k in (1, 2, 3, 8, 9, 16, 17)) and (cut[33] > 0 and cut[64] > 0 if robust else cut[33] == 0 and cut[64] == 0), cut
    # ORIGINAL_IDS: the same walk and order, prim mapped; without counts and counters: the same rows
    k = 3
    dev = device_nearest(bvh, tree, dprims, drays, k, flags)
    o = device_nearest(bvh, tree, dprims, drays, k, flags | ORIGINAL_IDS)
    want, _ = expected_rows(tree, rays, sorted_, k, prim_ids=ids.astype(np.uint32))
    assert differing_rows(o[0], want) == 0 and (o[1] == dev[1]).all() and (o[2] == dev[2]).all()
    bare = device_nearest(bvh, tree, dprims, drays, k, flags, counts=False, counters=False)
    assert bare[0].tobytes() == dev[0].tobytes()


@pytest.fixture(scope="module")
def dense(dll, lib):
    """The dense 200-triangle scene with 1023 rays and the device objects; host rows per k on demand."""
    tree, _, _, ids, nodes = seeded_case(lib, "tri", 200)
    raw = dense_tris(200, 400)
    rays = np.concatenate([rays_through([0, 0, 0], [1, 1, 1], 512, 13, np.float32), rays_through([0, 0, 0], [1, 1, 1], 511, 14, np.float32, targets=points_on(raw, 511, 15))])
    cache = {}

    def host(k, robust=False):
        if (k, robust) not in cache:
            cache[(k, robust)] = host_nearest(dll, tree, rays, k, robust=robust, threads=8)
        return cache[(k, robust)]
    return tree, nodes, ids, rays, host, device_bvh(tree, nodes, ids), _cuda(tree.prims)


@pytest.mark.parametrize("k", [1, 9, 16, 33])
def test_block_edges(dense, k):
    """k = 1, 9, 16 / 33 take blocks of 256, 128 and 64 float lanes."""
    tree, _, _, rays, host, bvh, dprims = dense
    assert block_lanes(tree, k) == {1: 256, 9: 128, 16: 64, 33: 64}[k]
    h_rows, h_counts, _ = host(k)
    for n in (1, 63, 64, 65, 127, 128, 129, 255, 256, 257):
        rows, counts, _ = device_nearest(bvh, tree, dprims, _cuda(rays[:n]), k)
        assert rows.tobytes() == h_rows[:n].tobytes() and (counts == h_counts[:n]).all(), n


@pytest.mark.parametrize("k", [1, 16, 33])
def test_block_edges_double(dll, lib, k):
    """The double spheres: blocks of 64, 128 and 64 lanes."""
    tree, rays, _, ids, nodes = seeded_case(lib, "sphere", 200)
    assert block_lanes(tree, k) == {1: 64, 16: 128, 33: 64}[k]
    bvh, dprims = device_bvh(tree, nodes, ids), _cuda(tree.prims)
    h_rows, h_counts, _ = host_nearest(dll, tree, rays, k, robust=True, threads=8)
    for n in (1, 63, 64, 65, 127, 128, 129, 255, 256):
        rows, counts, _ = device_nearest(bvh, tree, dprims, _cuda(rays[:n]), k, ROBUST)
        assert rows.tobytes() == h_rows[:n].tobytes() and (counts == h_counts[:n]).all(), n


def test_empty_batch_writes_nothing(dense):
    import torch
    from bvh_amd import _lib
    tree, _, _, rays, _, bvh, dprims = dense
    counts = _cuda(np.full(8, SENT_COUNT, dtype=np.uint32))
    rec = _cuda(np.full(8 * 16, SENT_BYTE, dtype=np.uint8))
    cnt = _cuda(np.full(3, 5, dtype=np.int64))
    rc = _lib.load().bvh3f_intersect_rays_nearest_tri(bvh._h, dprims.data_ptr(), None, 0, 4, 0, rec.data_ptr(), counts.data_ptr(), cnt.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0
    assert (_np(counts, np.uint32) == SENT_COUNT).all() and (_np(rec) == SENT_BYTE).all() and (_np(cnt) == 5).all()


@pytest.mark.parametrize("depth", [70, 300])
@pytest.mark.parametrize("stacked", [False, True])
def test_trees_deeper_than_64_levels(dll, restatement, depth, stacked):
    tree, nodes = chain(depth, restatement.prep_tris, stacked)
    bvh = device_bvh(tree, nodes)
    rays = chain_rays(depth, 300)                              # 300: not a multiple of the block; every 4th ray stacks on every level
    dprims, drays = _cuda(tree.prims), _cuda(rays)
    for k, flags in ((1, 0), (17, 0), (64, ROBUST)):
        host = host_nearest(dll, tree, rays, k, robust=bool(flags), deep_cap=depth - 64 + 1, threads=8)
        assert (host[1][::4] == min(k, depth + 1)).all()
        _same(device_nearest(bvh, tree, dprims, drays, k, flags), host)


def test_sorted_equals_unsorted(dense):
    tree, _, ids, rays, host, bvh, dprims = dense
    odd = rays.copy()
    odd[3, 0] = np.nan                                         # origins and directions that are no number take a key like any other
    odd[9, 4] = np.nan
    odd[11, 3:6] = 0
    odd[12, 6] = np.nan                                        # not walked: a padded row
    odd[13, 6:8] = [2, 1]                                      # tmin > tmax
    k = 8
    for r in (rays, odd):
        base = device_nearest(bvh, tree, dprims, _cuda(r), k, UNSORTED)
        if r is rays:
            _same(base, host(k))
        else:
            assert base[1][12] == 0 and (base[0][12]["prim"] == INVALID).all()
        _same(device_nearest(bvh, tree, dprims, _cuda(r), k, SORTED), base)
        _same(device_nearest(bvh, tree, dprims, _cuda(r), k, 0), base)
        o = device_nearest(bvh, tree, dprims, _cuda(r), k, SORTED | ORIGINAL_IDS)
        valid = base[0]["prim"] != INVALID
        assert (o[0]["prim"][valid] == ids[base[0]["prim"][valid].astype(np.int64)]).all() and (o[1] == base[1]).all() and (o[2] == base[2]).all()


def test_independent_of_position_stream_and_slicing(dll, dense):
    import torch
    from bvh_amd import _lib
    tree, _, _, rays, host, bvh, dprims = dense
    k = 8
    h_rows, h_counts, _ = host(k)
    perm = np.random.default_rng(3).permutation(len(rays))
    rows, counts, _ = device_nearest(bvh, tree, dprims, _cuda(rays[perm]), k)
    assert rows.tobytes() == h_rows[perm].tobytes() and (counts == h_counts[perm]).all()
    rows, counts, _ = device_nearest(bvh, tree, dprims, _cuda(np.repeat(rays[500:503], 100, axis=0)), k)      # one ray at many positions
    assert rows.tobytes() == np.repeat(h_rows[500:503], 100, axis=0).tobytes()
    # two streams at once on one const tree
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    parts = [rays[:600], rays[400:]]
    dparts = [_cuda(p) for p in parts]
    outs = [torch.zeros((len(p), k, 4), dtype=torch.float32, device="cuda") for p in parts]
    dcounts = [torch.zeros(len(p), dtype=torch.int32, device="cuda") for p in parts]
    f = _lib.load().bvh3f_intersect_rays_nearest_tri
    torch.cuda.synchronize()
    for s, d, o, c in zip(streams, dparts, outs, dcounts):
        assert f(bvh._h, dprims.data_ptr(), d.data_ptr(), d.shape[0], k, 0, o.data_ptr(), c.data_ptr(), None, C.c_void_p(s.cuda_stream)) == 0
    torch.cuda.synchronize()
    assert _np(outs[0]).tobytes() == h_rows[:600].tobytes() and _np(outs[1]).tobytes() == h_rows[400:].tobytes()
    assert (_np(dcounts[0], np.uint32) == h_counts[:600]).all() and (_np(dcounts[1], np.uint32) == h_counts[400:]).all()
    # a batch the launch path cuts in two (a chain of 4161 levels: the spill of a launch, 8 bytes per entry, holds 8064 lanes): the same
    # bytes as the host walk, which knows nothing of launches
    depth = 4160
    tris, cnodes, _ = qs.chain(depth, np.float32, stacked=True)
    from test_closest_point_host import precompute
    from test_radius_search_host import Tree
    ctree = Tree(cnodes["bounds"], cnodes["index"], precompute(tris, np.float32), 0)
    lanes = block_lanes(ctree, k)
    per = qs.per_launch(depth, 8, lanes)
    n = per + 300
    crays = chain_rays(depth, n, base=qs.chain_base(depth), every=64)
    cbvh = device_bvh(ctree, cnodes)
    c_host = host_nearest(dll, ctree, crays, k, deep_cap=qs.deep_cap(depth), threads=16)
    c_dev = device_nearest(cbvh, ctree, _cuda(ctree.prims), _cuda(crays), k)
    assert _lib.load().bvh_amd_last_query_launches() == 2
    _same(c_dev, c_host)
    assert (c_host[1][::64] == k).all()


def test_k1_against_intersect_and_k64_against_ray_hits(lib):
    """4096 rays on the 2k soup, the 2k double spheres and the layered grid. k = 1: the hit / miss and the t bits of bvh_amd.intersect
    with the same ROBUST flag, its prim wherever the ray's all-hits list has no second record at that t. k = 64: the ray's
    bvh_amd.ray_hits list sorted by (t, prim), byte for byte (no list here is longer than 64 unless asserted cut)."""
    import bvh_amd
    from bvh_amd import synth
    scenes = []
    for scene in ("soup2k", "spheres2k_f64"):
        g = load_golden(scene)
        raw = g["prims"]
        sphere = raw.shape[1] == 4
        bvh = bvh_amd.Bvh.deserialize(g["bvh_parallel_high"].tobytes(), dtype=raw.dtype.type)
        dprims = bvh_amd.gather(raw, bvh.device_prim_ids()) if sphere else bvh_amd.precompute_tris(raw, bvh.device_prim_ids())
        lo, hi = synth.scene_bounds(raw)
        rays = np.concatenate([rays_through(lo, hi, 2048, 21, raw.dtype), rays_through(lo, hi, 2048, 22, raw.dtype, targets=points_on(raw, 2048, 23))])
        scenes.append((scene, bvh, dprims, rays, "sphere" if sphere else "tri"))
    from ray_nearest_ref import layered_grid
    raw, rays = layered_grid(4096)
    bb, cc = bvh_amd.tri_bounds(raw)
    bvh = bvh_amd.DefaultBuilder.build(bb, cc)
    scenes.append(("grid", bvh, bvh_amd.precompute_tris(raw, bvh.device_prim_ids()), rays, "tri"))
    for scene, bvh, dprims, rays, leaf in scenes:
        for robust in (False, True):
            closest = bvh_amd.hits_to_numpy(bvh_amd.intersect(bvh, dprims, rays, robust=robust, leaf=leaf))
            off, hits = bvh_amd.ray_hits(bvh, dprims, rays, leaf=leaf, robust=robust)
            off, hits = _np(off), bvh_amd.hits_to_numpy(hits)
            sorted_ = [np.sort(hits[off[r]:off[r + 1]], order=["t", "prim"]) for r in range(len(rays))]
            rows1, counts1 = bvh_amd.ray_hits_nearest(bvh, dprims, rays, 1, leaf=leaf, robust=robust)
            row1 = bvh_amd.hits_to_numpy(rows1)
            hit = closest["prim"] != INVALID
            assert hit.sum() > 1000
            assert ((row1["prim"] != INVALID) == hit).all() and (_np(counts1) == hit).all()
            bits = np.uint64 if row1["t"].dtype == np.float64 else np.uint32
            assert (np.ascontiguousarray(row1["t"]).view(bits) == np.ascontiguousarray(closest["t"]).view(bits)).all()
            tie = first_two_tie(sorted_)
            assert (row1["prim"][hit & ~tie] == closest["prim"][hit & ~tie]).all()
            if scene == "grid":
                assert (hit & tie).sum() >= len(rays) // 4
                assert (row1["prim"][hit & tie] == np.array([s["prim"][0] for s, x in zip(sorted_, hit & tie) if x])).all()   # the lowest index
            rows64, counts64 = bvh_amd.ray_hits_nearest(bvh, dprims, rays, 64, leaf=leaf, robust=robust)
            rows64 = bvh_amd.hits_to_numpy(rows64).reshape(len(rays), 64)
            lengths = off[1:] - off[:-1]
            assert (_np(counts64) == np.minimum(lengths, 64)).all()
            for r in range(len(rays)):
                m = min(int(lengths[r]), 64)
                assert rows64[r, :m].tobytes() == sorted_[r][:m].tobytes(), (scene, robust, r)
                assert (rows64[r, m:]["prim"] == INVALID).all()


def test_refusals(dense):
    import bvh_amd
    import torch
    from bvh_amd import _lib
    tree, nodes, ids, rays, _, bvh, dprims = dense
    lib = _lib.load()
    n, k = len(rays), 2
    dr = _cuda(rays)
    counts = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    rec = torch.zeros((k * n + 8, 4), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    f = lib.bvh3f_intersect_rays_nearest_tri
    P = lambda t: t.data_ptr()

    def refused(rc, word):
        assert rc == -2 and word in _lib.last_error(), (rc, _lib.last_error())

    for ok in (0, ROBUST, SORTED | ROBUST | ORIGINAL_IDS, UNSORTED):
        assert f(bvh._h, P(dprims), P(dr), n, k, ok, P(rec), P(counts), P(cnt), None) == 0, _lib.last_error()
    assert f(bvh._h, P(dprims), P(dr), n, k, 0, P(rec), None, None, None) == 0, _lib.last_error()      # counts and counters are optional
    for bad in (1, 1 | ROBUST, 32, 1 << 20):                                                     # ANY_HIT, unknown bits
        refused(f(bvh._h, P(dprims), P(dr), n, k, bad, P(rec), P(counts), None, None), "flags")
    for bad_k in (0, 65, 1 << 20):
        refused(f(bvh._h, P(dprims), P(dr), n, bad_k, 0, P(rec), P(counts), None, None), "k must be in [1, 64]")
    refused(f(None, P(dprims), P(dr), n, k, 0, P(rec), P(counts), None, None), "null bvh")
    refused(f(bvh._h, None, P(dr), n, k, 0, P(rec), P(counts), None, None), "null device pointer")
    refused(f(bvh._h, P(dprims), None, n, k, 0, P(rec), P(counts), None, None), "null device pointer")
    refused(f(bvh._h, P(dprims), P(dr), n, k, 0, None, P(counts), None, None), "null device pointer")
    for args in ((P(dprims) + 4, P(dr), n, k, 0, P(rec), P(counts), None, None),                  # misaligned prims, rays, records,
                 (P(dprims), P(dr) + 8, n - 1, k, 0, P(rec), P(counts), None, None),              # counts, counters
                 (P(dprims), P(dr), n, k, 0, P(rec) + 8, P(counts), None, None),
                 (P(dprims), P(dr), n, k, 0, P(rec), P(counts) + 2, None, None),
                 (P(dprims), P(dr), n, k, 0, P(rec), P(counts), P(cnt) + 4, None)):
        refused(f(bvh._h, *args), "aligned")
    # alignment to the element is enough: records from the second record, counts and counters from their second entry
    assert f(bvh._h, P(dprims), P(dr), n, k, 0, P(rec) + 16, P(counts) + 4, P(cnt) + 8, None) == 0, _lib.last_error()
    # a 2D tree
    g2 = load_golden("circles2k_2f")
    b2, c2 = bvh_amd.sphere_bounds(g2["prims"])
    bvh2 = bvh_amd.DefaultBuilder.build(b2, c2)
    refused(f(bvh2._h, P(dprims), P(dr), n, k, 0, P(rec), P(counts), None, None), "3D trees only")
    for call in (lambda: bvh_amd.ray_hits_nearest(bvh2, dprims, rays, 2), lambda: bvh_amd.ray_hits_nearest(bvh, dprims, rays.astype(np.float64), 2),
                 lambda: bvh_amd.ray_hits_nearest(bvh, _np(dprims).astype(np.float64), rays, 2)):
        with pytest.raises(TypeError):
            call()
    for bad_k in (0, 65, -1):
        with pytest.raises(ValueError):
            bvh_amd.ray_hits_nearest(bvh, dprims, rays, bad_k)
    with pytest.raises(ValueError):
        bvh_amd.ray_hits_nearest(bvh, dprims, rays, 2, leaf="box")


def test_python_layer(dense):
    import bvh_amd
    import torch
    tree, _, ids, rays, host, bvh, dprims = dense
    n, k = len(rays), 3
    h_rows, h_counts, h_cnt = host(k)
    hits, counts = bvh_amd.ray_hits_nearest(bvh, dprims, rays, k)
    assert hits.dtype == torch.float32 and hits.shape == (n, k, 4) and hits.is_cuda and counts.dtype == torch.int32 and counts.shape == (n,)
    assert bvh_amd.hits_to_numpy(hits).tobytes() == h_rows.tobytes() and (_np(counts, np.uint32) == h_counts).all()
    hits, counts, cnt = bvh_amd.ray_hits_nearest(bvh, dprims, _cuda(rays), k, sort_queries=True, counters=True)
    assert bvh_amd.hits_to_numpy(hits).tobytes() == h_rows.tobytes() and cnt.dtype == torch.int64 and (_np(cnt).astype(np.uint64) == h_cnt).all()
    ohits, _ = bvh_amd.ray_hits_nearest(bvh, dprims, rays, k, original_ids=True, sort_queries=False)
    got = bvh_amd.hits_to_numpy(ohits).reshape(n, k)
    valid = h_rows["prim"] != INVALID
    assert (got["prim"][valid] == ids[h_rows["prim"][valid].astype(np.int64)]).all() and (got["prim"][~valid] == INVALID).all()
    r_rows, r_counts, _ = host(k, robust=True)
    hits, counts = bvh_amd.ray_hits_nearest(bvh, dprims, rays, k, robust=True)
    assert bvh_amd.hits_to_numpy(hits).tobytes() == r_rows.tobytes()
    e_hits, e_counts = bvh_amd.ray_hits_nearest(bvh, dprims, np.zeros((0, 8), np.float32), k)
    assert e_hits.shape == (0, k, 4) and e_counts.shape == (0,)
    far = rays.copy()
    far[:, :3] += 1000
    far[:, 3:6] = [1, 0, 0]
    z_hits, z_counts = bvh_amd.ray_hits_nearest(bvh, dprims, far, k, robust=True)
    z = bvh_amd.hits_to_numpy(z_hits)
    assert (_np(z_counts) == 0).all() and (z["prim"] == INVALID).all() and (z["t"].reshape(n, k) == far[:, 7:8]).all() and (z["u"] == 0).all()
    # double spheres: (n, k, 4) float64 records {prim, t0, t1, 0}
    tree_s, rays_s, _, _, nodes_s = seeded_case(reference_lib(), "sphere", 200)
    bvh_s = device_bvh(tree_s, nodes_s)
    hits, counts = bvh_amd.ray_hits_nearest(bvh_s, tree_s.prims, rays_s, 5, leaf="sphere", robust=True)
    rec = bvh_amd.hits_to_numpy(hits).reshape(len(rays_s), 5)
    assert hits.dtype == torch.float64 and rec.dtype == oracle.HITD and (rec["pad"] == 0).all() and (rec["v"] == 0).all()
    full = _np(counts) == 5
    assert full.any() and (np.diff(rec[full]["t"], axis=1) >= 0).all() and (rec[full]["t"] <= rec[full]["u"]).all()
