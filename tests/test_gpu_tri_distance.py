"""MI355X: batched triangle-distance queries (bvh3X_tri_distance, bvh_amd.tri_distance). The device's records, query barycentrics and
counters are byte-equal to the host harness's (the same text compiled by g++, tests/test_tri_distance_host.py) on the golden scenes
and a 20,000-triangle float soup built on the device, with a scalar max_distance and a per-query array; trees deeper than 64 levels
against the harness's brute force; a one-triangle tree, n = 1 and n = 0; a record does not depend on the reordering flags, on the
batch it is in, or on ORIGINAL_IDS beyond prim; out= is honoured; moved geometry after refit_tris; the cross-check with
tri_intersect_count; refusals. (The refusal of a tree without a device copy or without device prim ids is point_query_check's and the
launch path's, shared with the other queries; no constructor of the library leaves such a tree, so it is not reached here.)"""
import numpy as np
import pytest

import tri_intersect_ref as R
from conftest import load_golden
from test_closest_point_host import INVALID
from test_tri_distance_host import (HAND, SCENES, T0, chain_queries, compile_harness, host_brute, host_walk, scene_queries)

pytestmark = pytest.mark.gpu

SORTED, ORIGINAL_IDS, UNSORTED = 4, 8, 16


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return compile_harness(tmp_path_factory.mktemp("tri_distance_gpu"))


def _device(bvh, tris, q, max_distance=np.inf, **kw):
    """bvh_amd.tri_distance with everything asked for -> (records, (n, 2) query barycentrics, counters), numpy."""
    import bvh_amd
    hits, uv, cnt = bvh_amd.tri_distance(bvh, tris, q, max_distance, query_uv=True, counters=True, **kw)
    return bvh_amd.hits_to_numpy(hits), uv.cpu().numpy(), cnt.cpu().numpy().astype(np.uint64)


def _device_vs_host(dll, bvh, tree, q, max_distance=np.inf, deep_cap=0):
    """The device against the host walk over the same tree: records, query barycentrics and counters, byte for byte."""
    got, uv, cnt = _device(bvh, tree.tris, q, max_distance)
    h_hits, h_uv, h_cnt = host_walk(dll, tree, q, max_distance, deep_cap=deep_cap, threads=8)
    assert got.tobytes() == h_hits.tobytes(), np.flatnonzero((got["prim"] != h_hits["prim"]) | (got["t"] != h_hits["t"]))[:8]
    assert uv.tobytes() == h_uv.tobytes() and (cnt == h_cnt).all(), (cnt, h_cnt)
    return h_hits, h_uv


def device_tree(tree):
    """The device twin of a harness tree."""
    import bvh_amd
    import oracle
    nodes = np.zeros(len(tree.index), dtype=oracle.NODED if tree.double else oracle.NODEF)
    nodes["bounds"], nodes["index"] = tree.bounds, tree.index
    return bvh_amd.Bvh.from_nodes(nodes, tree.ids.astype(np.uint64))


@pytest.mark.parametrize("scene", SCENES)
def test_device_equals_host_golden(dll, scene):
    import bvh_amd
    tree = R.golden_tree(scene, "parallel_high")
    bvh = bvh_amd.Bvh.deserialize(load_golden(scene)["bvh_parallel_high"].tobytes(), dtype=tree.dtype.type)
    q = scene_queries(tree.tris, 2048, 33)
    hits, _ = _device_vs_host(dll, bvh, tree, q)                                           # unbounded, one scalar
    assert (hits["prim"] != INVALID).all() and 50 < (hits["t"] == 0).sum() < len(q)
    lim = np.where(np.arange(len(q)) % 3 == 0, np.inf, np.median(hits["t"])).astype(tree.dtype)
    part, _ = _device_vs_host(dll, bvh, tree, q, lim)                                      # one max_distance per query
    assert 100 < (part["prim"] == INVALID).sum() < len(q) - 100
    _device_vs_host(dll, bvh, tree, q, float(np.median(hits["t"])))


def test_device_equals_host_float_soup_built_on_the_device(dll):
    import bvh_amd
    from bvh_amd import synth
    tris = synth.soup(20000, dtype=np.float32)
    bb, cc = bvh_amd.tri_bounds(tris)
    bvh = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.Medium))
    nodes = bvh.nodes
    tree = R.TriTree(nodes["bounds"], nodes["index"], tris, bvh.prim_ids)
    q = scene_queries(tris[::8], 2048, 35)                     # (made from every 8th triangle: the generator compares all pairs)
    hits, _ = _device_vs_host(dll, bvh, tree, q)
    assert (hits["t"] == 0).sum() > 100 and (hits["t"] > 0).sum() > 500
    _device_vs_host(dll, bvh, tree, q, np.where(np.arange(len(q)) % 2 == 0, 0.01, np.inf).astype(np.float32))


@pytest.mark.parametrize("depth", [65, 300])
def test_trees_deeper_than_64_levels(dll, depth):
    """The Deep kernels: a chain tree, the stack spilling to HBM; 300 queries (not a multiple of the block). Byte-equal to the brute
    force."""
    tree = R.chain_tree(depth, stacked=True)
    bvh = device_tree(tree)
    q = chain_queries(depth, 300)
    hits, uv = _device_vs_host(dll, bvh, tree, q, deep_cap=depth - 64 + 1)
    brute, buv, _ = host_brute(dll, tree, q)
    assert hits.tobytes() == brute.tobytes() and uv.tobytes() == buv.tobytes()
    assert (hits["t"][::4] == 0).all() and (hits["t"] > 0).sum() > 100


def test_one_triangle_tree_and_tiny_batches(dll):
    import bvh_amd
    from oracle import NODEF
    tri = np.array([T0], dtype=np.float32)
    nodes = np.zeros(1, dtype=NODEF)
    nodes[0]["bounds"], nodes[0]["index"] = [0, 4, 0, 4, 0, 0], (0 << 4) | 1
    tree = R.TriTree(nodes["bounds"], nodes["index"], tri, np.zeros(1, dtype=np.uint32))
    bvh = bvh_amd.Bvh.from_nodes(nodes, np.zeros(1, dtype=np.uint64))
    q = np.array([HAND["vertex_face"][0], HAND["piercing"][0], HAND["point_query"][0], HAND["segment_query_through"][0]], dtype=np.float32)
    q = np.concatenate([q, q[:2]])
    q[4, 3], q[5, 0] = np.nan, np.nan
    lim = np.array([np.inf, np.inf, np.inf, np.inf, np.inf, 1.0], dtype=np.float32)
    hits, uv = _device_vs_host(dll, bvh, tree, q, lim)
    assert hits["prim"].tolist() == [0, 0, 0, 0, INVALID, INVALID] and hits["t"][:3].tolist() == [2.0, 0.0, 5.0] and hits["t"][3] <= 1e-6
    assert hits["t"][4:].tolist() == [np.inf, 1.0] and (uv[4:] == 0).all()
    for bad in (np.nan, -1.0):                                                             # a NaN or negative max_distance: the miss record
        miss, muv = _device_vs_host(dll, bvh, tree, q[:2], np.array([bad, bad], dtype=np.float32))
        assert (miss["prim"] == INVALID).all() and (miss["u"] == 0).all() and (muv == 0).all()
    one, _ = _device_vs_host(dll, bvh, tree, q[:1])                                        # n = 1
    assert one.tobytes() == hits[:1].tobytes()
    empty = bvh_amd.tri_distance(bvh, tri, np.zeros((0, 9), np.float32))                   # n = 0
    assert empty.shape == (0, 4)
    e_hits, e_uv = bvh_amd.tri_distance(bvh, tri, np.zeros((0, 9), np.float32), np.zeros(0, np.float32), query_uv=True)
    assert e_hits.shape == (0, 4) and e_uv.shape == (0, 2)


@pytest.fixture(scope="module")
def soup(dll):
    """The 2k soup, 2,048 queries with their max distances, the device tree and the host harness's records."""
    import bvh_amd
    tree = R.golden_tree("soup2k", "parallel_high")
    bvh = bvh_amd.Bvh.deserialize(load_golden("soup2k")["bvh_parallel_high"].tobytes())
    q = scene_queries(tree.tris, 2048, 37)
    free, _, _ = host_walk(dll, tree, q, threads=8)
    lim = np.where(np.arange(len(q)) % 2 == 0, np.median(free["t"][free["t"] > 0]), np.inf).astype(np.float32)
    host, huv, _ = host_walk(dll, tree, q, lim, threads=8)
    return bvh, tree, q, lim, host, huv


def test_flags_batches_and_out(soup):
    import bvh_amd
    import torch
    bvh, tree, q, lim, host, huv = soup
    tris = torch.from_numpy(tree.tris).cuda()

    def run(qq, ll, **kw):
        hits, uv = bvh_amd.tri_distance(bvh, tris, qq, ll, query_uv=True, **kw)
        return bvh_amd.hits_to_numpy(hits), uv.cpu().numpy()

    base, buv = run(q, lim, sort_queries=False)
    assert base.tobytes() == host.tobytes() and buv.tobytes() == huv.tobytes()
    for kw in ({"sort_queries": True}, {}):                                                 # SORTED, and the library's choice
        h, u = run(q, lim, **kw)
        assert h.tobytes() == base.tobytes() and u.tobytes() == buv.tobytes()
    half = len(q) // 2 + 77                                                                 # the slice of the batch a query is in
    a, b = run(q[:half], lim[:half]), run(q[half:], lim[half:], sort_queries=True)
    assert np.concatenate([a[0], b[0]]).tobytes() == base.tobytes() and np.concatenate([a[1], b[1]]).tobytes() == buv.tobytes()
    perm = np.random.default_rng(3).permutation(len(q))
    h, u = run(q[perm], lim[perm], sort_queries=True)
    assert h.tobytes() == base[perm].tobytes() and u.tobytes() == buv[perm].tobytes()
    orig, ouv = run(q, lim, original_ids=True, sort_queries=True)                           # ORIGINAL_IDS maps prim and nothing else
    hit = base["prim"] != INVALID
    assert 200 < hit.sum() < len(q) - 200
    assert (orig["prim"][hit] == tree.ids[base["prim"][hit].astype(np.int64)]).all() and (orig["prim"][~hit] == INVALID).all()
    for f in ("t", "u", "v"):
        assert orig[f].tobytes() == base[f].tobytes()
    assert ouv.tobytes() == buv.tobytes()
    out = torch.full((len(q) + 3, 4), 7.0, dtype=torch.float32, device="cuda")              # out= is honoured, nothing beyond n records written
    back = bvh_amd.tri_distance(bvh, tris, q, torch.from_numpy(lim).cuda(), out=out)
    assert back.data_ptr() == out.data_ptr()
    assert bvh_amd.hits_to_numpy(out[:len(q)]).tobytes() == base.tobytes() and (out[len(q):] == 7.0).all().item()


def test_moving_geometry(dll):
    """Build on soup2k, move every triangle, refit_tris: the query answers for the moved mesh (the host harness on the refitted
    tree's own nodes and the moved triangles)."""
    import bvh_amd
    import torch
    raw = load_golden("soup2k")["prims"]
    bb, cc = bvh_amd.tri_bounds(raw)
    bvh = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.High))
    diag = float(np.linalg.norm(raw.reshape(-1, 3).max(axis=0) - raw.reshape(-1, 3).min(axis=0)))
    rng = np.random.default_rng(17)
    shift = ((rng.random((len(raw), 1, 3)) * 2 - 1) * 0.05 * diag).astype(np.float32)
    moved = np.ascontiguousarray((raw.reshape(-1, 3, 3) + shift).reshape(-1, 9))
    q = scene_queries(moved, 1024, 39)
    before = bvh_amd.hits_to_numpy(bvh_amd.tri_distance(bvh, raw, q))
    bvh.refit_tris(torch.from_numpy(moved).cuda())
    nodes = bvh.nodes
    tree = R.TriTree(nodes["bounds"], nodes["index"], moved, bvh.prim_ids)
    hits, _ = _device_vs_host(dll, bvh, tree, q)
    assert (hits["t"] == 0).sum() > 50 and hits.tobytes() != before.tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_zero_distance_is_tri_intersect_count(dll, orc, dtype):
    """On the quarter-integer lattice (triangles with area on both sides) {q : t == 0} equals {q : count > 0}; on soup2k, where the
    queries include segments and points that the intersection query refuses, {q : count > 0} is a subset of {q : t == 0}."""
    import bvh_amd
    lat = R.lattice_tris()
    lat = lat[(np.cross(lat[:, 1] - lat[:, 0], lat[:, 2] - lat[:, 0]) != 0).any(axis=1)]
    other = R.lattice_tris(256, seed=77)
    other = other[(np.cross(other[:, 1] - other[:, 0], other[:, 2] - other[:, 0]) != 0).any(axis=1)]
    other = np.concatenate([other, other[::3] + np.array([14, 0, 0]), other[1::3] + np.array([0, -11, 9])])      # (in the lattice, beside it, off its corner)
    tris, q = (lat.reshape(-1, 9) / 4.0).astype(dtype), (other.reshape(-1, 9) / 4.0).astype(dtype)
    tree = R.built_tree(orc, tris, dtype)
    bvh = device_tree(tree)
    hits, _ = _device_vs_host(dll, bvh, tree, q)
    counts = bvh_amd.tri_intersect_count(bvh, tree.tris, q).cpu().numpy()
    assert ((hits["t"] == 0) == (counts > 0)).all() and 20 < (counts > 0).sum() < len(q) - 20
    if dtype == np.float32:
        stree = R.golden_tree("soup2k", "parallel_high")
        sbvh = bvh_amd.Bvh.deserialize(load_golden("soup2k")["bvh_parallel_high"].tobytes())
        sq = scene_queries(stree.tris, 2048, 41)
        shits = bvh_amd.hits_to_numpy(bvh_amd.tri_distance(sbvh, stree.tris, sq))
        scounts = bvh_amd.tri_intersect_count(sbvh, stree.tris, sq).cpu().numpy()
        assert (shits["t"][scounts > 0] == 0).all() and (scounts > 0).sum() > 100


def test_refusals(soup):
    import bvh_amd
    import torch
    from bvh_amd import _lib
    bvh, tree, q, lim, host, huv = soup
    lib = _lib.load()
    n, nt = len(q), len(tree.tris)
    dt, dq, dl = torch.from_numpy(tree.tris).cuda(), torch.from_numpy(q).cuda(), torch.from_numpy(lim).cuda()
    rec = torch.full((n + 8, 4), 7.0, dtype=torch.float32, device="cuda")
    uv = torch.full((n + 8, 2), 7.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((4,), 77, dtype=torch.int64, device="cuda")
    f = lib.bvh3f_tri_distance
    P = lambda t: t.data_ptr()
    inf = float("inf")

    def refused(rc, word):
        assert rc == -2 and word in _lib.last_error(), (rc, _lib.last_error())

    assert f(bvh._h, P(dt), nt, None, 0, inf, None, 0, None, None, None, None) == 0                # n == 0: a no-op
    for bad in (1, 2, 32, 64, 1 << 20):                                                           # ANY_HIT, ROBUST, TRI_SKIP_SHARED, unknown bits
        refused(f(bvh._h, P(dt), nt, P(dq), n, inf, None, bad, P(rec), None, None, None), "flags")
    refused(f(None, P(dt), nt, P(dq), n, inf, None, 0, P(rec), None, None, None), "null bvh")
    refused(f(bvh._h, None, nt, P(dq), n, inf, None, 0, P(rec), None, None, None), "null device pointer")
    refused(f(bvh._h, P(dt), nt, None, n, inf, None, 0, P(rec), None, None, None), "null device pointer")
    refused(f(bvh._h, P(dt), nt, P(dq), n, inf, None, 0, None, None, None, None), "null device pointer")
    for args in ((P(dt) + 2, nt - 1, P(dq), n, inf, None, 0, P(rec), None, None, None),           # misaligned triangles, queries, max distances,
                 (P(dt), nt, P(dq) + 2, n - 1, inf, None, 0, P(rec), None, None, None),           # records, query barycentrics, counters
                 (P(dt), nt, P(dq), n, inf, P(dl) + 2, 0, P(rec), None, None, None),
                 (P(dt), nt, P(dq), n, inf, None, 0, P(rec) + 8, None, None, None),
                 (P(dt), nt, P(dq), n, inf, None, 0, P(rec), P(uv) + 2, None, None),
                 (P(dt), nt, P(dq), n, inf, None, 0, P(rec), None, P(cnt) + 4, None)):
        refused(f(bvh._h, *args), "aligned")
    largest = int(tree.ids.max())
    for nt_bad in (largest, largest - 5, 1):                                                      # n_tris at or below the largest prim id
        refused(f(bvh._h, P(dt), nt_bad, P(dq), n, inf, None, 0, P(rec), P(uv), P(cnt), None), "prim_ids refers")
    g2 = load_golden("circles2k_2f")                                                              # a 2D tree
    b2, c2 = bvh_amd.sphere_bounds(g2["prims"])
    bvh2 = bvh_amd.DefaultBuilder.build(b2, c2)
    refused(f(bvh2._h, P(dt), nt, P(dq), n, inf, None, 0, P(rec), P(uv), P(cnt), None), "3D trees only")
    torch.cuda.synchronize()
    assert (rec == 7.0).all().item() and (uv == 7.0).all().item() and (cnt == 77).all().item()    # every refusal left the outputs untouched
    # what is accepted: every flag combination, optional pointers, alignment to the element
    for ok in (0, SORTED, SORTED | ORIGINAL_IDS, UNSORTED):
        assert f(bvh._h, P(dt), nt, P(dq), n, inf, P(dl), ok, P(rec), P(uv), P(cnt), None) == 0, _lib.last_error()
    assert f(bvh._h, P(dt), largest + 1, P(dq) + 4 * 9, n - 1, inf, P(dl) + 4, 0, P(rec) + 16, P(uv) + 8, P(cnt) + 8, None) == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert bvh_amd.hits_to_numpy(rec[1:n]).tobytes() == host[1:].tobytes() and (rec[n:] == 7.0).all().item()
    assert uv[1:n].cpu().numpy().tobytes() == huv[1:].tobytes() and (uv[n:] == 7.0).all().item()
    for call in (lambda: bvh_amd.tri_distance(bvh2, tree.tris, q), lambda: bvh_amd.tri_distance(bvh, tree.tris, q.astype(np.float64)),
                 lambda: bvh_amd.tri_distance(bvh, tree.tris.astype(np.float64), q), lambda: bvh_amd.tri_distance(bvh, tree.tris, q, lim.astype(np.float64)),
                 lambda: bvh_amd.tri_distance(bvh, tree.tris, q, out=torch.zeros((n, 4), dtype=torch.float64, device="cuda"))):
        with pytest.raises(TypeError):
            call()
    for bad_lim in (lim[:-1], np.concatenate([lim, lim[:1]]), lim.reshape(-1, 2)):                # a wrong d_max_distances length
        with pytest.raises(ValueError):
            bvh_amd.tri_distance(bvh, tree.tris, q, bad_lim)
