"""MI355X: batched triangle-intersection queries and mesh self-intersections (bvh3X_intersect_tris / bvh3X_intersect_tris_self,
bvh_amd.tri_intersect_count / tri_intersect_search / self_intersections). The device's counts, lists and counters are byte-equal to the
host harness's (the same text compiled by g++, tests/test_tri_intersect_host.py), which on the lattice equals an exact integer
reference; block edges; the reordering flags; trees deeper than 64 levels; independence of batch size, position and stream; moving
geometry (refit_tris -> queries); refusals; the Python layer.

Which path a launch took (reordered or not) is not observable from outside: the reordering test asks for the flags explicitly and
compares results and counters."""
import ctypes as C

import numpy as np
import pytest

import tri_intersect_ref as R
from conftest import load_golden
from tri_intersect_ref import GUARD, INVALID, SENT_PRIM, SKIP_SHARED, TREES, TRI_SCENES

pytestmark = pytest.mark.gpu

ORIGINAL_IDS, SORTED, UNSORTED = 8, 4, 16


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return R.compile_harness(tmp_path_factory.mktemp("tri_intersect_gpu"))


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


def device_walk(bvh, tris, queries, offsets=None, total=0, counts=True, flags=0, stream=None):
    """One call of the C entry point, shaped like tri_intersect_ref.host_walk: queries None = bvh3X_intersect_tris_self. The list
    buffer holds `total` entries between two guard zones of GUARD sentinels and is returned WITH the guards. -> (counts, list,
    counters), numpy."""
    import torch
    from bvh_amd import _lib
    lib = _lib.load()
    t = tris if isinstance(tris, torch.Tensor) else _cuda(tris)
    n = bvh.prim_count if queries is None else len(queries)
    c = _cuda(np.full(n, 0xABABABAB, dtype=np.uint32)) if counts else None
    cnt = torch.zeros(3, dtype=torch.int64, device="cuda")
    off = lp = None
    if offsets is not None:
        off = _cuda(np.ascontiguousarray(offsets, dtype=np.uint64))
        lp = _cuda(np.full(total + 2 * GUARD, SENT_PRIM, dtype=np.uint32))
    P = lambda x, skip=0: None if x is None else x.data_ptr() + skip
    if queries is None:
        rc = getattr(lib, f"bvh{bvh._s}_intersect_tris_self")(bvh._h, P(t), t.shape[0], flags, P(c), P(off), P(lp, 4 * GUARD), P(cnt), stream)
    else:
        q = queries if isinstance(queries, torch.Tensor) else _cuda(np.asarray(queries).reshape(-1, 9))
        rc = getattr(lib, f"bvh{bvh._s}_intersect_tris")(bvh._h, P(t), t.shape[0], P(q), n, flags, P(c), P(off), P(lp, 4 * GUARD), P(cnt), stream)
    assert rc == 0, _lib.last_error()
    return (None if c is None else _np(c, np.uint32)), (None if lp is None else _np(lp, np.uint32)), _np(cnt).astype(np.uint64)


def device_intersect(bvh, tris, queries, flags=0):
    """Count pass, bvh_amd_offsets_from_counts, fill pass -> what host_intersect returns, with its checks."""
    import bvh_amd
    counts, _, cnt0 = device_walk(bvh, tris, queries, flags=flags)
    offsets = _np(bvh_amd.offsets_from_counts(_cuda(counts)), np.uint64)
    total = int(offsets[-1])
    c2, lp, cnt = device_walk(bvh, tris, queries, offsets=offsets, total=total, flags=flags)
    assert (c2 == counts).all() and (cnt == cnt0).all()
    assert (lp[:GUARD] == SENT_PRIM).all() and (lp[GUARD + total:] == SENT_PRIM).all()
    return offsets, lp[GUARD:GUARD + total], counts, cnt


def _same(dev, host):
    for d, h in zip(dev, host):
        assert d.dtype == h.dtype and d.tobytes() == h.tobytes()


def device_tree(tree):
    """The device twin of a harness tree."""
    import bvh_amd
    import oracle
    nodes = np.zeros(len(tree.index), dtype=oracle.NODED if tree.double else oracle.NODEF)
    nodes["bounds"], nodes["index"] = tree.bounds, tree.index
    return bvh_amd.Bvh.from_nodes(nodes, tree.ids.astype(np.uint64))


def check_all_modes(dll, bvh, tree, queries):
    """Both entry points, plain, with ORIGINAL_IDS and with SKIP_SHARED; fixed slots with guard zones on the device buffer."""
    t = _cuda(tree.tris)
    for q in queries + [None]:
        host = R.host_intersect(dll, tree, q, threads=8)
        _same(device_intersect(bvh, t, q), host)
        _same(device_intersect(bvh, t, q, flags=ORIGINAL_IDS), R.host_intersect(dll, tree, q, threads=8, original_ids=True))
        _same(device_intersect(bvh, t, q, flags=SKIP_SHARED), R.host_intersect(dll, tree, q, threads=8, skip_shared=True))
        _same(device_intersect(bvh, t, q, flags=SKIP_SHARED | ORIGINAL_IDS), R.host_intersect(dll, tree, q, threads=8, skip_shared=True, original_ids=True))
        assert host[0][-1] > 0
        # k = 3 slots per query behind a non-zero base: truncated lists, padding, guard zones on the device buffer
        n, k, base = (tree.n if q is None else len(q)), 3, 7
        fixed = (base + k * np.arange(n + 1)).astype(np.uint64)
        total = base + k * n + 5
        _same(device_walk(bvh, t, q, offsets=fixed, total=total), R.host_walk(dll, tree, q, offsets=fixed, total=total))
        _same(device_walk(bvh, t, q, offsets=fixed, total=total, counts=False)[1:], R.host_walk(dll, tree, q, offsets=fixed, total=total, counts=False)[1:])


@pytest.mark.parametrize("scene", TRI_SCENES)
@pytest.mark.parametrize("mode", TREES)
def test_device_equals_host_golden(dll, scene, mode):
    import bvh_amd
    g = load_golden(scene)
    tree = R.golden_tree(scene, mode)
    bvh = bvh_amd.Bvh.deserialize(g[f"bvh_{mode}"].tobytes(), dtype=np.float64 if tree.double else np.float32)
    assert bvh._s == ("3d" if tree.double else "3f")
    check_all_modes(dll, bvh, tree, [R.query_tris(tree.tris, 1024, 11), tree.tris])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_device_equals_host_and_the_integer_reference_on_the_lattice(dll, orc, dtype):
    t = R.lattice_tris()
    tree = R.built_tree(orc, t.astype(dtype), dtype)
    bvh = device_tree(tree)
    other = R.lattice_tris(256, seed=77)
    check_all_modes(dll, bvh, tree, [t.astype(dtype).reshape(-1, 9), other.astype(dtype).reshape(-1, 9)])
    order = tree.ids.astype(np.int64)
    ref = R.sat_matrix(t, t)
    want_counts, want_ids = R.expected_lists(ref[np.ix_(order, order)] & R.self_mask(tree.n), tree.dfs)
    _, ids, counts, _ = device_intersect(bvh, tree.tris, None)
    assert (counts == want_counts).all() and ids.tobytes() == want_ids.tobytes()
    want_counts, want_ids = R.expected_lists(R.sat_matrix(other, t)[:, order], tree.dfs)
    _, ids, counts, _ = device_intersect(bvh, tree.tris, other.astype(dtype).reshape(-1, 9))
    assert (counts == want_counts).all() and ids.tobytes() == want_ids.tobytes()


@pytest.fixture(scope="module")
def terrain(dll):
    """terrain2k, parallel_high: the device tree, the harness's, 1024 query triangles and the harness's exact lists for them."""
    import bvh_amd
    tree = R.golden_tree("terrain2k", "parallel_high")
    bvh = bvh_amd.Bvh.deserialize(load_golden("terrain2k")["bvh_parallel_high"].tobytes(), dtype=np.float32)
    q = R.query_tris(tree.tris, 1024, 21)
    return bvh, tree, _cuda(tree.tris), q, R.host_intersect(dll, tree, q, threads=8)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_block_edges(terrain, n):
    bvh, tree, t, q, (h_off, h_ids, h_counts, _) = terrain
    off, ids, counts, _ = device_intersect(bvh, t, q[:n])
    assert (counts == h_counts[:n]).all() and ids.tobytes() == h_ids[:int(h_off[n])].tobytes()


def test_empty_batch_writes_nothing(terrain):
    import torch
    from bvh_amd import _lib
    bvh, tree, t, q, _ = terrain
    dq = _cuda(q)
    c = _cuda(np.full(8, 0xABABABAB, dtype=np.uint32))
    lp = _cuda(np.full(8, SENT_PRIM, dtype=np.uint32))
    off = torch.zeros(9, dtype=torch.int64, device="cuda")
    cnt = torch.full((3,), 77, dtype=torch.int64, device="cuda")
    f = _lib.load().bvh3f_intersect_tris
    assert f(bvh._h, t.data_ptr(), t.shape[0], dq.data_ptr(), 0, 0, c.data_ptr(), off.data_ptr(), lp.data_ptr(), cnt.data_ptr(), None) == 0
    assert f(bvh._h, None, 0, None, 0, 0, None, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert (_np(c, np.uint32) == 0xABABABAB).all() and (_np(lp, np.uint32) == SENT_PRIM).all() and (_np(cnt) == 77).all()


def test_sorted_equals_unsorted(terrain):
    bvh, tree, t, q, host = terrain
    base = device_intersect(bvh, t, q, flags=UNSORTED)
    _same(base, host)
    for flags in (SORTED, 0, SORTED | ORIGINAL_IDS, SORTED | SKIP_SHARED):
        again = device_intersect(bvh, t, q, flags=flags)
        if flags & ORIGINAL_IDS:
            assert (again[1] == tree.ids[base[1].astype(np.int64)]).all() and (again[0] == base[0]).all() and (again[3] == base[3]).all()
        elif flags & SKIP_SHARED:
            _same(again, device_intersect(bvh, t, q, flags=UNSORTED | SKIP_SHARED))
            assert (again[3] == base[3]).all()
        else:
            _same(again, base)
    # triangles whose box centre is no number take a key like any other
    odd = q.copy()
    odd[3, 0], odd[3, 3] = -np.inf, np.inf
    odd[9, 1] = np.nan
    _same(device_intersect(bvh, t, odd, flags=SORTED), device_intersect(bvh, t, odd, flags=UNSORTED))


@pytest.mark.parametrize("depth", [70, 300])
@pytest.mark.parametrize("stacked", [False, True])
def test_trees_deeper_than_64_levels(dll, depth, stacked):
    tree = R.chain_tree(depth, stacked=stacked)
    bvh = device_tree(tree)
    q = R.chain_queries(depth, 300)                            # 300: not a multiple of the block
    cap = depth - 64 + 1                                       # what the launch path sizes the spill to
    host = R.host_intersect(dll, tree, q, deep_cap=cap)
    assert (host[2][::4] == depth + 1).all()
    _same(device_intersect(bvh, tree.tris, q), host)
    _same(device_intersect(bvh, tree.tris, None), R.host_intersect(dll, tree, None, deep_cap=cap))


def test_a_deep_tree_takes_several_launches(dll):
    """3000 levels: the 256 MB of spill hold 22 784 lanes' worth, so a batch of 300 more is cut into two launches. Most queries sit at
    the near end of the chain (the top of the tree: a few levels each), eight cross every level."""
    import query_slices as qs
    from bvh_amd import _lib
    depth = 3000
    per = qs.per_launch(depth, 4)
    n = per + 300
    tree = R.chain_tree(depth, stacked=True, ids=qs.prim_ids(depth + 1))
    bvh = device_tree(tree)
    q = R.chain_queries(depth, n)
    sliver = q[0].copy()
    q[:, 0::3] += np.float32(depth - 6)                        # from the far end to the near end
    q[::n // 8] = sliver
    cap = qs.deep_cap(depth)
    host = R.host_intersect(dll, tree, q, deep_cap=cap, threads=8, original_ids=True)
    assert len(qs.slices(n, qs.per_launch(depth, 4, n=n))) == 2 and (host[2][::n // 8] == depth + 1).all() and host[2][1::4].max() > 0
    _same(device_intersect(bvh, tree.tris, q, flags=ORIGINAL_IDS), host)
    assert _lib.load().bvh_amd_last_query_launches() == 2


def test_independent_of_position_batch_and_stream(terrain):
    import torch
    bvh, tree, t, q, (h_off, h_ids, h_counts, _) = terrain
    lists = np.split(h_ids, h_off[1:-1].astype(np.int64))
    perm = np.random.default_rng(3).permutation(len(q))
    off, ids, counts, _ = device_intersect(bvh, t, q[perm])
    assert (counts == h_counts[perm]).all() and ids.tobytes() == np.concatenate([lists[j] for j in perm]).tobytes()
    off, ids, counts, _ = device_intersect(bvh, t, np.repeat(q[496:499], 100, axis=0))           # one query at many positions
    assert ids.tobytes() == np.concatenate([lists[496 + j // 100] for j in range(300)]).tobytes()
    # two streams at once on one const tree: count passes, then fill passes
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    parts = [q[:600], q[400:]]
    torch.cuda.synchronize()
    out = []
    for s, part in zip(streams, parts):
        with torch.cuda.stream(s):
            out.append(device_walk(bvh, t, _cuda(part), stream=C.c_void_p(s.cuda_stream))[0])
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
    f = _lib.load().bvh3f_intersect_tris
    for s, d, o, b, part in zip(streams, dq, d_offs, bufs, parts):
        assert f(bvh._h, t.data_ptr(), t.shape[0], d.data_ptr(), len(part), 0, None, o.data_ptr(), b.data_ptr(), None, C.c_void_p(s.cuda_stream)) == 0
    torch.cuda.synchronize()
    assert _np(bufs[0], np.uint32).tobytes() == h_ids[:int(h_off[600])].tobytes()
    assert _np(bufs[1], np.uint32).tobytes() == h_ids[int(h_off[400]):].tobytes()


def test_moving_geometry(dll):
    """Build on soup2k, move every triangle, refit_tris: self_intersections and tri_intersect_search on the moved triangles equal the
    host harness on the moved scene (the refitted tree's own nodes), and the harness's brute force."""
    import bvh_amd
    raw = load_golden("soup2k")["prims"]
    bb, cc = bvh_amd.tri_bounds(raw)
    bvh = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.High))
    lo, hi = raw.reshape(-1, 3).min(axis=0), raw.reshape(-1, 3).max(axis=0)
    diag = float(np.linalg.norm(hi - lo))
    rng = np.random.default_rng(17)
    shift = ((rng.random((len(raw), 1, 3)) * 2 - 1) * 0.05 * diag).astype(np.float32)
    moved = np.ascontiguousarray((raw.reshape(-1, 3, 3) + shift).reshape(-1, 9))
    d_moved = _cuda(moved)
    bvh.refit_tris(d_moved)
    nodes = bvh.nodes
    tree = R.TriTree(nodes["bounds"], nodes["index"], moved, bvh.prim_ids)
    ids = tree.ids.astype(np.int64)
    pt = tree.ordered_tris()
    for skip in (False, True):
        h_off, h_ids, h_counts, _ = R.host_intersect(dll, tree, None, threads=8, skip_shared=skip)
        wc, wi = R.expected_lists(R.pair_matrix(dll, pt, pt, skip_shared=skip) & R.self_mask(tree.n), tree.dfs)
        assert (h_counts == wc).all() and h_ids.tobytes() == wi.tobytes() and len(wi) > 20
        rows = np.repeat(np.arange(tree.n), h_counts)
        pairs = _np(bvh_amd.self_intersections(bvh, d_moved, original_ids=False, skip_shared=skip))
        assert pairs.dtype == np.int64 and pairs.shape == (len(h_ids), 2)
        assert (pairs[:, 0] == rows).all() and (pairs[:, 1] == h_ids).all() and (pairs[:, 0] < pairs[:, 1]).all()
        opairs = _np(bvh_amd.self_intersections(bvh, d_moved, skip_shared=skip))
        assert (opairs[:, 0] == ids[rows]).all() and (opairs[:, 1] == ids[h_ids.astype(np.int64)]).all()
    q = R.query_tris(moved, 1024, 29)
    h_off, h_ids, h_counts, _ = R.host_intersect(dll, tree, q, threads=8)
    wc, wi = R.expected_lists(R.pair_matrix(dll, q, pt), tree.dfs)
    assert (h_counts == wc).all() and h_ids.tobytes() == wi.tobytes() and len(wi) > 64
    off, lst = bvh_amd.tri_intersect_search(bvh, d_moved, q)
    assert _np(off, np.uint64).tobytes() == h_off.tobytes() and _np(lst, np.uint32).tobytes() == h_ids.tobytes()
    off, lst = bvh_amd.tri_intersect_search(bvh, d_moved, q, original_ids=True)
    assert (_np(lst) == ids[h_ids.astype(np.int64)]).all()


def test_refusals(terrain):
    import bvh_amd
    import torch
    from bvh_amd import _lib
    bvh, tree, t, q, _ = terrain
    lib = _lib.load()
    n = len(q)
    dq = _cuda(q)
    counts = torch.zeros(max(n, tree.n), dtype=torch.int32, device="cuda")
    offs = torch.arange(max(n, tree.n) + 1, dtype=torch.int64, device="cuda") * 2
    lp = torch.zeros(2 * max(n, tree.n) + 4, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    fb, fs = lib.bvh3f_intersect_tris, lib.bvh3f_intersect_tris_self
    P = lambda x: x.data_ptr()
    nt = t.shape[0]

    def refused(rc, word):
        assert rc == -2 and word in _lib.last_error(), (rc, _lib.last_error())

    assert fb(bvh._h, P(t), nt, P(dq), n, 0, P(counts), P(offs), P(lp), P(cnt), None) == 0
    assert fs(bvh._h, P(t), nt, 0, P(counts), P(offs), P(lp), P(cnt), None) == 0
    assert fs(bvh._h, P(t), nt, SKIP_SHARED | ORIGINAL_IDS, P(counts), P(offs), P(lp), P(cnt), None) == 0
    for bad in (1, 2, 64, 1 << 20):                                                              # ANY_HIT, ROBUST, unknown bits
        refused(fb(bvh._h, P(t), nt, P(dq), n, bad, P(counts), None, None, None, None), "flags")
        refused(fs(bvh._h, P(t), nt, bad, P(counts), None, None, None, None), "flags")
        refused(fb(bvh._h, P(t), nt, P(dq), 0, bad, P(counts), None, None, None, None), "flags")    # (before the empty batch is accepted)
    for bad in (SORTED, UNSORTED, SORTED | ORIGINAL_IDS, SORTED | SKIP_SHARED):                  # self mode never reorders
        refused(fs(bvh._h, P(t), nt, bad, P(counts), None, None, None, None), "flags")
    # the new flag is refused by every other entry point
    bb = _cuda(R.tri_boxes(tree.tris))
    refused(lib.bvh3f_overlap_boxes(bvh._h, P(bb), nt, P(bb), 8, SKIP_SHARED, P(counts), None, None, None, None), "flags")
    refused(lib.bvh3f_overlap_self(bvh._h, P(bb), nt, SKIP_SHARED, P(counts), None, None, None, None), "flags")
    refused(fb(None, P(t), nt, P(dq), n, 0, P(counts), None, None, None, None), "null bvh")
    refused(fs(None, P(t), nt, 0, P(counts), None, None, None, None), "null bvh")
    refused(fb(bvh._h, None, nt, P(dq), n, 0, P(counts), None, None, None, None), "null device pointer")
    refused(fb(bvh._h, P(t), nt, None, n, 0, P(counts), None, None, None, None), "null device pointer")
    refused(fs(bvh._h, None, nt, 0, P(counts), None, None, None, None), "null device pointer")
    refused(fb(bvh._h, P(t), nt, P(dq), n, 0, None, None, None, None, None), "d_counts")         # neither counts nor offsets
    refused(fs(bvh._h, P(t), nt, 0, None, None, None, None, None), "d_counts")
    refused(fb(bvh._h, P(t), nt, P(dq), n, 0, P(counts), P(offs), None, None, None), "d_list_prims")      # offsets without a list
    refused(fb(bvh._h, P(t), nt, P(dq), n, 0, P(counts), None, P(lp), None, None), "lists need d_offsets")
    refused(fs(bvh._h, P(t), nt, 0, P(counts), None, P(lp), None, None), "lists need d_offsets")
    for args in ((P(t) + 2, nt - 1, P(dq), n, 0, P(counts), None, None, None, None),              # misaligned triangles, queries, counts,
                 (P(t), nt, P(dq) + 2, n - 1, 0, P(counts), None, None, None, None),              # offsets, list, counters
                 (P(t), nt, P(dq), n, 0, P(counts) + 2, None, None, None, None),
                 (P(t), nt, P(dq), n, 0, P(counts), P(offs) + 4, P(lp), None, None),
                 (P(t), nt, P(dq), n, 0, P(counts), P(offs), P(lp) + 2, None, None),
                 (P(t), nt, P(dq), n, 0, P(counts), None, None, P(cnt) + 4, None)):
        refused(fb(bvh._h, *args), "aligned")
    # alignment to the element is enough: queries from their second scalar on, counts and list from their second entry
    assert fb(bvh._h, P(t), nt, P(dq) + 4, n - 1, 0, P(counts) + 4, P(offs) + 8, P(lp) + 4, P(cnt) + 8, None) == 0, _lib.last_error()
    largest = int(tree.ids.max())
    for nt_bad in (largest, largest - 5, 1):                                                     # n_tris at or below the largest prim id
        refused(fb(bvh._h, P(t), nt_bad, P(dq), n, 0, P(counts), None, None, None, None), "prim_ids refers")
        refused(fs(bvh._h, P(t), nt_bad, 0, P(counts), None, None, None, None), "prim_ids refers")
    assert fb(bvh._h, P(t), largest + 1, P(dq), n, 0, P(counts), None, None, None, None) == 0
    # a tree without a device copy of its prim ids / without a device copy: an empty handle
    # a 2D tree
    g2 = load_golden("circles2k_2f")
    b2, c2 = bvh_amd.sphere_bounds(g2["prims"])
    bvh2 = bvh_amd.DefaultBuilder.build(b2, c2)
    refused(fb(bvh2._h, P(t), nt, P(dq), n, 0, P(counts), None, None, None, None), "3D trees only")
    refused(fs(bvh2._h, P(t), nt, 0, P(counts), None, None, None, None), "3D trees only")
    for call in (lambda: bvh_amd.tri_intersect_count(bvh2, tree.tris, q), lambda: bvh_amd.tri_intersect_search(bvh2, tree.tris, q),
                 lambda: bvh_amd.self_intersections(bvh2, tree.tris), lambda: bvh_amd.tri_intersect_search(bvh, tree.tris.astype(np.float64), q),
                 lambda: bvh_amd.tri_intersect_count(bvh, tree.tris, q.astype(np.float64))):
        with pytest.raises(TypeError):
            call()


def test_python_layer(dll, terrain):
    import bvh_amd
    import torch
    bvh, tree, t, q, (h_off, h_ids, h_counts, h_cnt) = terrain
    n = len(q)
    c = bvh_amd.tri_intersect_count(bvh, tree.tris, q)
    assert c.dtype == torch.int32 and c.shape == (n,) and (_np(c, np.uint32) == h_counts).all()
    c, cnt = bvh_amd.tri_intersect_count(bvh, t, _cuda(q), sort_queries=True, counters=True)
    assert (_np(c, np.uint32) == h_counts).all() and cnt.dtype == torch.int64 and (_np(cnt).astype(np.uint64) == h_cnt).all()
    s_off, s_ids, s_counts, _ = R.host_intersect(dll, tree, q, threads=8, skip_shared=True)
    assert (_np(bvh_amd.tri_intersect_count(bvh, t, q, skip_shared=True), np.uint32) == s_counts).all() and s_counts.sum() < h_counts.sum()
    off, ids = bvh_amd.tri_intersect_search(bvh, t, q)
    assert off.dtype == torch.int64 and off.shape == (n + 1,) and ids.dtype == torch.int32 and ids.shape == (len(h_ids),)
    assert _np(off, np.uint64).tobytes() == h_off.tobytes() and _np(ids, np.uint32).tobytes() == h_ids.tobytes()
    off, ids = bvh_amd.tri_intersect_search(bvh, t, q, skip_shared=True)
    assert _np(off, np.uint64).tobytes() == s_off.tobytes() and _np(ids, np.uint32).tobytes() == s_ids.tobytes()
    off, oids, cnt = bvh_amd.tri_intersect_search(bvh, t, q, original_ids=True, sort_queries=False, counters=True)
    assert (_np(oids) == tree.ids[h_ids.astype(np.int64)]).all() and (_np(cnt).astype(np.uint64) == h_cnt).all()
    k = 4
    off, ids, counts = bvh_amd.tri_intersect_search(bvh, t, q, max_per_query=k)
    assert (_np(off) == k * np.arange(n + 1)).all() and ids.shape == (n * k,) and counts.dtype == torch.int32 and (_np(counts, np.uint32) == h_counts).all()
    rows = _np(ids).reshape(n, k)
    for i in range(n):
        m = min(int(h_counts[i]), k)
        assert (rows[i, :m].view(np.uint32) == h_ids[int(h_off[i]):int(h_off[i]) + m]).all() and (rows[i, m:] == -1).all()
    assert h_counts.max() > k and (h_counts < k).any()
    e_off, e_ids = bvh_amd.tri_intersect_search(bvh, t, np.zeros((0, 9), np.float32))
    assert e_off.tolist() == [0] and e_ids.shape == (0,) and bvh_amd.tri_intersect_count(bvh, t, np.zeros((0, 9), np.float32)).shape == (0,)
    far = q + np.float32(1000)
    z_off, z_ids = bvh_amd.tri_intersect_search(bvh, t, far)
    assert z_off.tolist() == [0] * (n + 1) and z_ids.shape == (0,)
    # self_intersections: the rows of the CSR, in both id modes; neighbours are skipped by default
    for skip in (True, False):
        so, si, sc, scnt = R.host_intersect(dll, tree, None, threads=8, skip_shared=skip)
        rows = np.repeat(np.arange(tree.n), sc)
        pairs = bvh_amd.self_intersections(bvh, t, original_ids=False, skip_shared=skip)
        assert pairs.dtype == torch.int64 and pairs.is_cuda and pairs.shape == (len(si), 2)
        assert (_np(pairs)[:, 0] == rows).all() and (_np(pairs)[:, 1] == si).all()
        opairs, cnt = bvh_amd.self_intersections(bvh, t, skip_shared=skip, counters=True)
        ids = tree.ids.astype(np.int64)
        assert (_np(opairs)[:, 0] == ids[rows]).all() and (_np(opairs)[:, 1] == ids[si.astype(np.int64)]).all()
        assert (_np(cnt).astype(np.uint64) == scnt).all() and INVALID not in _np(opairs)
    assert bvh_amd.self_intersections(bvh, t).shape == (0, 2) and len(si) > 1000     # a terrain: every pair is a pair of neighbours
