"""MI355X: batched box-overlap queries and self-overlap pairs (bvh3X_overlap_boxes / bvh3X_overlap_self, bvh_amd.overlap_count /
overlap_search / self_overlaps). The device's counts, lists and counters are byte-equal to the host harness's (the same text compiled
by g++, tests/test_overlap_host.py), which in turn equals a numpy brute force exactly; block edges; the reordering flags; trees deeper
than 64 levels; independence of batch size, position and stream; moving geometry (tri_bounds -> refit_boxes -> queries); refusals;
the Python layer.

bvh_amd_last_launch_reordered reports ray launches only, and a reordered launch fetches, tests and visits exactly what an unreordered
one does, so which path ran is not observable from outside: the reordering test asks for the flags explicitly and compares results
and counters."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from test_closest_point_host import GOLDEN_SCENES
from test_overlap_host import (GUARD, INVALID, SELF_PAIRS, SENT_PRIM, TREES, Tree, brute, chain, chain_boxes, compile_harness, expected_lists, golden_tree,
                               host_overlap, host_walk, prim_boxes, query_boxes, self_expected)

pytestmark = pytest.mark.gpu

ORIGINAL_IDS, SORTED, UNSORTED = 8, 4, 16


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return compile_harness(tmp_path_factory.mktemp("overlap_gpu"))


def _np(t, dtype=None):
    a = t.detach().cpu().numpy()
    return a if dtype is None else a.view(dtype)


def _cuda(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


def device_walk(bvh, bboxes, queries, offsets=None, total=0, counts=True, flags=0, stream=None):
    """One call of the C entry point, shaped like test_overlap_host.host_walk: queries None = bvh3X_overlap_self. The list buffer holds
    `total` entries between two guard zones of GUARD sentinels and is returned WITH the guards. -> (counts, list, counters), numpy."""
    import torch
    from bvh_amd import _lib
    lib = _lib.load()
    bb = bboxes if isinstance(bboxes, torch.Tensor) else _cuda(bboxes)
    n = bvh.prim_count if queries is None else len(queries)
    c = _cuda(np.full(n, 0xABABABAB, dtype=np.uint32)) if counts else None
    cnt = torch.zeros(3, dtype=torch.int64, device="cuda")
    off = lp = None
    if offsets is not None:
        off = _cuda(np.ascontiguousarray(offsets, dtype=np.uint64))
        lp = _cuda(np.full(total + 2 * GUARD, SENT_PRIM, dtype=np.uint32))
    P = lambda t, skip=0: None if t is None else t.data_ptr() + skip
    if queries is None:
        rc = getattr(lib, f"bvh{bvh._s}_overlap_self")(bvh._h, P(bb), bb.shape[0], flags, P(c), P(off), P(lp, 4 * GUARD), P(cnt), stream)
    else:
        q = queries if isinstance(queries, torch.Tensor) else _cuda(queries)
        rc = getattr(lib, f"bvh{bvh._s}_overlap_boxes")(bvh._h, P(bb), bb.shape[0], P(q), n, flags, P(c), P(off), P(lp, 4 * GUARD), P(cnt), stream)
    assert rc == 0, _lib.last_error()
    return (None if c is None else _np(c, np.uint32)), (None if lp is None else _np(lp, np.uint32)), _np(cnt).astype(np.uint64)


def device_overlap(bvh, bboxes, queries, flags=0):
    """Count pass, bvh_amd_offsets_from_counts, fill pass -> what host_overlap returns, with its checks."""
    import bvh_amd
    counts, _, cnt0 = device_walk(bvh, bboxes, queries, flags=flags)
    offsets = _np(bvh_amd.offsets_from_counts(_cuda(counts)), np.uint64)
    total = int(offsets[-1])
    c2, lp, cnt = device_walk(bvh, bboxes, queries, offsets=offsets, total=total, flags=flags)
    assert (c2 == counts).all() and (cnt == cnt0).all()
    assert (lp[:GUARD] == SENT_PRIM).all() and (lp[GUARD + total:] == SENT_PRIM).all()
    return offsets, lp[GUARD:GUARD + total], counts, cnt


def _same(dev, host):
    for d, h in zip(dev, host):
        assert d.dtype == h.dtype and d.tobytes() == h.tobytes()


def golden_device_tree(scene, mode):
    import bvh_amd
    g = load_golden(scene)
    double = g["prims"].dtype == np.float64
    bvh = bvh_amd.Bvh.deserialize(g[f"bvh_{mode}"].tobytes(), dtype=np.float64 if double else np.float32)
    tree, raw = golden_tree(scene, mode)
    return bvh, tree, raw


@pytest.mark.parametrize("scene", GOLDEN_SCENES)
@pytest.mark.parametrize("mode", TREES)
def test_device_equals_host_golden(dll, scene, mode):
    bvh, tree, raw = golden_device_tree(scene, mode)
    assert bvh._s == ("3d" if tree.double else "3f")
    bb = _cuda(tree.bboxes)
    for q in (query_boxes(raw, 1024, tree.dtype, 11), prim_boxes(raw)):
        host = host_overlap(dll, tree, q, threads=8)
        _same(device_overlap(bvh, bb, q), host)
        _same(device_overlap(bvh, bb, q, flags=ORIGINAL_IDS), host_overlap(dll, tree, q, threads=8, original_ids=True))
        assert host[0][-1] > 0
    # k = 3 slots per query behind a non-zero base: truncated lists, padding, guard zones on the device buffer
    n, k, base = len(q), 3, 7
    fixed = (base + k * np.arange(n + 1)).astype(np.uint64)
    total = base + k * n + 5
    _same(device_walk(bvh, bb, q, offsets=fixed, total=total), host_walk(dll, tree, q, offsets=fixed, total=total))
    _same(device_walk(bvh, bb, q, offsets=fixed, total=total, counts=False)[1:], host_walk(dll, tree, q, offsets=fixed, total=total, counts=False)[1:])
    # self mode
    host = host_overlap(dll, tree, None, threads=8)
    assert int(host[0][-1]) == SELF_PAIRS[scene]
    _same(device_overlap(bvh, bb, None), host)
    _same(device_overlap(bvh, bb, None, flags=ORIGINAL_IDS), host_overlap(dll, tree, None, threads=8, original_ids=True))
    fixed = (2 * np.arange(tree.n + 1)).astype(np.uint64)
    _same(device_walk(bvh, bb, None, offsets=fixed, total=2 * tree.n), host_walk(dll, tree, None, offsets=fixed, total=2 * tree.n))


@pytest.fixture(scope="module")
def soup(dll):
    """soup2k, parallel_high: the device tree, the harness's, 1024 query boxes and the harness's exact lists for them."""
    bvh, tree, raw = golden_device_tree("soup2k", "parallel_high")
    q = query_boxes(raw, 1024, np.float32, 21)
    return bvh, tree, _cuda(tree.bboxes), q, host_overlap(dll, tree, q, threads=8)


@pytest.mark.parametrize("n", [1, 63, 64, 255, 256, 257, 1023])
def test_block_edges(soup, n):
    bvh, tree, bb, q, (h_off, h_ids, h_counts, _) = soup
    off, ids, counts, _ = device_overlap(bvh, bb, q[:n])
    assert (counts == h_counts[:n]).all() and ids.tobytes() == h_ids[:int(h_off[n])].tobytes()


def test_empty_batch_writes_nothing(soup):
    import torch
    from bvh_amd import _lib
    bvh, tree, bb, q, _ = soup
    dq = _cuda(q)
    c = _cuda(np.full(8, 0xABABABAB, dtype=np.uint32))
    lp = _cuda(np.full(8, SENT_PRIM, dtype=np.uint32))
    off = torch.zeros(9, dtype=torch.int64, device="cuda")
    cnt = torch.full((3,), 77, dtype=torch.int64, device="cuda")
    f = _lib.load().bvh3f_overlap_boxes
    assert f(bvh._h, bb.data_ptr(), bb.shape[0], dq.data_ptr(), 0, 0, c.data_ptr(), off.data_ptr(), lp.data_ptr(), cnt.data_ptr(), None) == 0
    assert f(bvh._h, None, 0, None, 0, 0, None, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert (_np(c, np.uint32) == 0xABABABAB).all() and (_np(lp, np.uint32) == SENT_PRIM).all() and (_np(cnt) == 77).all()


def test_sorted_equals_unsorted(soup):
    bvh, tree, bb, q, host = soup
    base = device_overlap(bvh, bb, q, flags=UNSORTED)
    _same(base, host)
    for flags in (SORTED, 0, SORTED | ORIGINAL_IDS):
        again = device_overlap(bvh, bb, q, flags=flags)
        if flags & ORIGINAL_IDS:
            assert (again[1] == tree.ids[base[1].astype(np.int64)]).all() and (again[0] == base[0]).all() and (again[3] == base[3]).all()
        else:
            _same(again, base)
    # boxes whose centre is no number (-inf + inf, a NaN) take a key like any other
    odd = q.copy()
    odd[3] = [-np.inf] * 3 + [np.inf] * 3
    odd[9, 1] = np.nan
    _same(device_overlap(bvh, bb, odd, flags=SORTED), device_overlap(bvh, bb, odd, flags=UNSORTED))


@pytest.mark.parametrize("depth", [70, 300])
@pytest.mark.parametrize("stacked", [False, True])
def test_trees_deeper_than_64_levels(dll, restatement, depth, stacked):
    import bvh_amd
    tree, nodes, _ = chain(depth, restatement.prep_tris, stacked)
    bvh = bvh_amd.Bvh.from_nodes(nodes, tree.ids.astype(np.uint64))
    q = chain_boxes(depth, 300)                                # 300: not a multiple of the block
    cap = depth - 64 + 1                                       # what the launch path sizes the spill to
    host = host_overlap(dll, tree, q, deep_cap=cap)
    assert (host[2][::4] == depth + 1).all()
    _same(device_overlap(bvh, tree.bboxes, q), host)
    _same(device_overlap(bvh, tree.bboxes, None), host_overlap(dll, tree, None, deep_cap=cap))


def test_independent_of_position_batch_and_stream(soup):
    import torch
    bvh, tree, bb, q, (h_off, h_ids, h_counts, _) = soup
    lists = np.split(h_ids, h_off[1:-1].astype(np.int64))
    perm = np.random.default_rng(3).permutation(len(q))
    off, ids, counts, _ = device_overlap(bvh, bb, q[perm])
    assert (counts == h_counts[perm]).all() and ids.tobytes() == np.concatenate([lists[j] for j in perm]).tobytes()
    off, ids, counts, _ = device_overlap(bvh, bb, np.repeat(q[500:503], 100, axis=0))           # one query at many positions
    assert ids.tobytes() == np.concatenate([lists[500 + j // 100] for j in range(300)]).tobytes()
    # two streams at once on one const tree: count passes, then fill passes
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    parts = [q[:600], q[400:]]
    torch.cuda.synchronize()
    out = []
    for s, part in zip(streams, parts):
        with torch.cuda.stream(s):
            out.append(device_walk(bvh, bb, _cuda(part), stream=C.c_void_p(s.cuda_stream))[0])
    torch.cuda.synchronize()
    assert (out[0] == h_counts[:600]).all() and (out[1] == h_counts[400:]).all()
    dq = [_cuda(p) for p in parts]
    offs = [np.concatenate([[0], np.cumsum(c.astype(np.uint64))]).astype(np.uint64) for c in out]
    bufs, d_offs = [], []
    for o in offs:
        bufs.append(_cuda(np.full(int(o[-1]), SENT_PRIM, dtype=np.uint32)))
        d_offs.append(_cuda(o))
    torch.cuda.synchronize()
    from bvh_amd import _lib
    f = _lib.load().bvh3f_overlap_boxes
    for s, d, o, b, part in zip(streams, dq, d_offs, bufs, parts):
        assert f(bvh._h, bb.data_ptr(), bb.shape[0], d.data_ptr(), len(part), 0, None, o.data_ptr(), b.data_ptr(), None, C.c_void_p(s.cuda_stream)) == 0
    torch.cuda.synchronize()
    assert _np(bufs[0], np.uint32).tobytes() == h_ids[:int(h_off[600])].tobytes()
    assert _np(bufs[1], np.uint32).tobytes() == h_ids[int(h_off[400]):].tobytes()


def test_moving_geometry():
    """Build on soup2k, move every triangle, tri_bounds -> refit_boxes: self_overlaps and overlap_search on the moved boxes equal the
    numpy brute force on the moved boxes exactly."""
    import bvh_amd
    raw = load_golden("soup2k")["prims"]
    bb, cc = bvh_amd.tri_bounds(raw)
    bvh = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.High))
    lo, hi = raw.reshape(-1, 3).min(axis=0), raw.reshape(-1, 3).max(axis=0)
    diag = float(np.linalg.norm(hi - lo))
    rng = np.random.default_rng(17)
    shift = ((rng.random((len(raw), 1, 3)) * 2 - 1) * 0.05 * diag).astype(np.float32)
    moved = (raw.reshape(-1, 3, 3) + shift).reshape(-1, 9)
    mb, _ = bvh_amd.tri_bounds(moved)
    bvh.refit_boxes(mb)
    boxes = _np(mb)
    assert (boxes == prim_boxes(moved)).all()
    nodes = bvh.nodes
    tree = Tree(nodes["bounds"], nodes["index"], boxes, bvh.prim_ids)
    ids = tree.ids.astype(np.int64)
    # self: the pair set, in both id modes
    within, (want_counts, want_ids) = self_expected(tree)
    rows = np.repeat(np.arange(tree.n), want_counts)
    pairs = _np(bvh_amd.self_overlaps(bvh, mb, original_ids=False))
    assert pairs.dtype == np.int64 and pairs.shape == (len(want_ids), 2) and len(want_ids) > 100
    assert (pairs[:, 0] == rows).all() and (pairs[:, 1] == want_ids).all() and (pairs[:, 0] < pairs[:, 1]).all()
    opairs = _np(bvh_amd.self_overlaps(bvh, mb))
    assert (opairs[:, 0] == ids[rows]).all() and (opairs[:, 1] == ids[want_ids.astype(np.int64)]).all()
    full = brute(boxes, boxes)                                 # by original id, no tree involved
    want_set = {(min(a, b), max(a, b)) for a, b in zip(*np.nonzero(np.triu(full, 1)))}
    got_set = {(min(a, b), max(a, b)) for a, b in opairs.tolist()}
    assert got_set == want_set and len(got_set) == len(opairs)
    # query boxes
    q = query_boxes(moved, 1024, np.float32, 29)
    off, lst = bvh_amd.overlap_search(bvh, mb, q)
    wc, wi = expected_lists(brute(tree.ordered_boxes(), q), tree.dfs)
    assert (np.diff(_np(off)) == wc).all() and _np(lst, np.uint32).tobytes() == wi.tobytes() and len(wi) > 1024
    off, lst = bvh_amd.overlap_search(bvh, mb, q, original_ids=True)
    assert (_np(lst) == ids[wi.astype(np.int64)]).all()


def test_refusals(soup):
    import bvh_amd
    import torch
    from bvh_amd import _lib
    bvh, tree, bb, q, _ = soup
    lib = _lib.load()
    n = len(q)
    dq = _cuda(q)
    counts = torch.zeros(max(n, tree.n), dtype=torch.int32, device="cuda")
    offs = torch.arange(max(n, tree.n) + 1, dtype=torch.int64, device="cuda") * 2
    lp = torch.zeros(2 * max(n, tree.n) + 4, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    fb, fs = lib.bvh3f_overlap_boxes, lib.bvh3f_overlap_self
    P = lambda t: t.data_ptr()
    nb = bb.shape[0]

    def refused(rc, word):
        assert rc == -2 and word in _lib.last_error(), (rc, _lib.last_error())

    assert fb(bvh._h, P(bb), nb, P(dq), n, 0, P(counts), P(offs), P(lp), P(cnt), None) == 0
    assert fs(bvh._h, P(bb), nb, 0, P(counts), P(offs), P(lp), P(cnt), None) == 0
    for bad in (1, 2, 32, 1 << 20):                                                              # ANY_HIT, ROBUST, unknown bits
        refused(fb(bvh._h, P(bb), nb, P(dq), n, bad, P(counts), None, None, None, None), "flags")
        refused(fs(bvh._h, P(bb), nb, bad, P(counts), None, None, None, None), "flags")
    for bad in (SORTED, UNSORTED, SORTED | ORIGINAL_IDS):                                        # self mode never reorders
        refused(fs(bvh._h, P(bb), nb, bad, P(counts), None, None, None, None), "flags")
    refused(fb(None, P(bb), nb, P(dq), n, 0, P(counts), None, None, None, None), "null bvh")
    refused(fs(None, P(bb), nb, 0, P(counts), None, None, None, None), "null bvh")
    refused(fb(bvh._h, None, nb, P(dq), n, 0, P(counts), None, None, None, None), "null device pointer")
    refused(fb(bvh._h, P(bb), nb, None, n, 0, P(counts), None, None, None, None), "null device pointer")
    refused(fs(bvh._h, None, nb, 0, P(counts), None, None, None, None), "null device pointer")
    refused(fb(bvh._h, P(bb), nb, P(dq), n, 0, None, None, None, None, None), "d_counts")        # neither counts nor offsets
    refused(fs(bvh._h, P(bb), nb, 0, None, None, None, None, None), "d_counts")
    refused(fb(bvh._h, P(bb), nb, P(dq), n, 0, P(counts), P(offs), None, None, None), "d_list_prims")     # offsets without a list
    refused(fb(bvh._h, P(bb), nb, P(dq), n, 0, P(counts), None, P(lp), None, None), "lists need d_offsets")
    refused(fs(bvh._h, P(bb), nb, 0, P(counts), None, P(lp), None, None), "lists need d_offsets")
    for args in ((P(bb) + 2, nb - 1, P(dq), n, 0, P(counts), None, None, None, None),             # misaligned boxes, queries, counts,
                 (P(bb), nb, P(dq) + 2, n - 1, 0, P(counts), None, None, None, None),             # offsets, list, counters
                 (P(bb), nb, P(dq), n, 0, P(counts) + 2, None, None, None, None),
                 (P(bb), nb, P(dq), n, 0, P(counts), P(offs) + 4, P(lp), None, None),
                 (P(bb), nb, P(dq), n, 0, P(counts), P(offs), P(lp) + 2, None, None),
                 (P(bb), nb, P(dq), n, 0, P(counts), None, None, P(cnt) + 4, None)):
        refused(fb(bvh._h, *args), "aligned")
    # alignment to the element is enough: queries from their second scalar on, counts and list from their second entry
    assert fb(bvh._h, P(bb), nb, P(dq) + 4, n - 1, 0, P(counts) + 4, P(offs) + 8, P(lp) + 4, P(cnt) + 8, None) == 0, _lib.last_error()
    largest = int(tree.ids.max())
    for nb_bad in (largest, largest - 5, 1):                                                     # n_boxes at or below the largest prim id
        refused(fb(bvh._h, P(bb), nb_bad, P(dq), n, 0, P(counts), None, None, None, None), "prim_ids refers")
        refused(fs(bvh._h, P(bb), nb_bad, 0, P(counts), None, None, None, None), "prim_ids refers")
    assert fb(bvh._h, P(bb), largest + 1, P(dq), n, 0, P(counts), None, None, None, None) == 0
    # a 2D tree
    g2 = load_golden("circles2k_2f")
    b2, c2 = bvh_amd.sphere_bounds(g2["prims"])
    bvh2 = bvh_amd.DefaultBuilder.build(b2, c2)
    refused(fb(bvh2._h, P(bb), nb, P(dq), n, 0, P(counts), None, None, None, None), "3D trees only")
    refused(fs(bvh2._h, P(bb), nb, 0, P(counts), None, None, None, None), "3D trees only")
    for call in (lambda: bvh_amd.overlap_count(bvh2, tree.bboxes, q), lambda: bvh_amd.overlap_search(bvh2, tree.bboxes, q),
                 lambda: bvh_amd.self_overlaps(bvh2, tree.bboxes), lambda: bvh_amd.overlap_search(bvh, tree.bboxes.astype(np.float64), q),
                 lambda: bvh_amd.overlap_count(bvh, tree.bboxes, q.astype(np.float64))):
        with pytest.raises(TypeError):
            call()


def test_python_layer(soup):
    import bvh_amd
    import torch
    bvh, tree, bb, q, (h_off, h_ids, h_counts, h_cnt) = soup
    n = len(q)
    c = bvh_amd.overlap_count(bvh, tree.bboxes, q)
    assert c.dtype == torch.int32 and c.shape == (n,) and (_np(c, np.uint32) == h_counts).all()
    c, cnt = bvh_amd.overlap_count(bvh, bb, _cuda(q), sort_queries=True, counters=True)
    assert (_np(c, np.uint32) == h_counts).all() and cnt.dtype == torch.int64 and (_np(cnt).astype(np.uint64) == h_cnt).all()
    off, ids = bvh_amd.overlap_search(bvh, bb, q)
    assert off.dtype == torch.int64 and off.shape == (n + 1,) and ids.dtype == torch.int32 and ids.shape == (len(h_ids),)
    assert _np(off, np.uint64).tobytes() == h_off.tobytes() and _np(ids, np.uint32).tobytes() == h_ids.tobytes()
    off, oids, cnt = bvh_amd.overlap_search(bvh, bb, q, original_ids=True, sort_queries=False, counters=True)
    assert (_np(oids) == tree.ids[h_ids.astype(np.int64)]).all() and (_np(cnt).astype(np.uint64) == h_cnt).all()
    k = 4
    off, ids, counts = bvh_amd.overlap_search(bvh, bb, q, max_per_query=k)
    assert (_np(off) == k * np.arange(n + 1)).all() and ids.shape == (n * k,) and counts.dtype == torch.int32 and (_np(counts, np.uint32) == h_counts).all()
    rows = _np(ids).reshape(n, k)
    for i in range(n):
        m = min(int(h_counts[i]), k)
        assert (rows[i, :m].view(np.uint32) == h_ids[int(h_off[i]):int(h_off[i]) + m]).all() and (rows[i, m:] == -1).all()
    assert h_counts.max() > k and (h_counts < k).any()
    e_off, e_ids = bvh_amd.overlap_search(bvh, bb, np.zeros((0, 6), np.float32))
    assert e_off.tolist() == [0] and e_ids.shape == (0,) and bvh_amd.overlap_count(bvh, bb, np.zeros((0, 6), np.float32)).shape == (0,)
    far = q + np.float32(1000)
    z_off, z_ids = bvh_amd.overlap_search(bvh, bb, far)
    assert z_off.tolist() == [0] * (n + 1) and z_ids.shape == (0,)
    # self_overlaps: the brute-force pair set, in both id modes
    within, (want_counts, want_ids) = self_expected(tree)
    rows = np.repeat(np.arange(tree.n), want_counts)
    pairs = bvh_amd.self_overlaps(bvh, bb, original_ids=False)
    assert pairs.dtype == torch.int64 and pairs.is_cuda and pairs.shape == (SELF_PAIRS["soup2k"], 2)
    assert (_np(pairs)[:, 0] == rows).all() and (_np(pairs)[:, 1] == want_ids).all()
    opairs, cnt = bvh_amd.self_overlaps(bvh, bb, counters=True)
    full = brute(tree.bboxes, tree.bboxes)
    want_set = {(min(a, b), max(a, b)) for a, b in zip(*np.nonzero(np.triu(full, 1)))}
    assert {(min(a, b), max(a, b)) for a, b in _np(opairs).tolist()} == want_set and len(want_set) == len(opairs) and int(cnt[0]) > 0
    assert INVALID not in _np(opairs)
