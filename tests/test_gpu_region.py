"""MI355X: batched convex-region queries (bvh3X_region_tris / bvh3X_region_spheres, bvh_amd.region_count / region_search /
frustum_planes). The device's counts, lists, inside flags and counters are byte-equal to the host harness's (the same text compiled by
g++, tests/test_region_host.py), which in turn equals the numpy brute force and exact clipping; block edges; trees deeper than 64
levels; independence of batch size, position and stream; moving geometry (refit_tris -> queries); refusals; the Python layer."""
import ctypes as C

import numpy as np
import pytest

import region_ref as R
from conftest import load_golden
from region_ref import GUARD, SENT_INSIDE, SENT_PRIM
from test_closest_point_host import GOLDEN_SCENES

pytestmark = pytest.mark.gpu

ORIGINAL_IDS, SORTED, UNSORTED, EXACT = 8, 4, 16, R.REGION_EXACT


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return R.compile_harness(tmp_path_factory.mktemp("region_gpu"))


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


def entry(bvh, leaf):
    from bvh_amd import _lib
    return getattr(_lib.load(), f"bvh{bvh._s}_region_{'spheres' if leaf else 'tris'}")


def device_walk(bvh, tree, prims, planes, flags=0, offsets=None, total=0, counts=True, inside=False, stream=None):
    """One call of the C entry point, shaped like region_ref.host_walk. The list buffers hold `total` entries between two guard zones
    of GUARD sentinels and are returned WITH the guards. -> (counts, list, inside flags, counters), numpy."""
    import torch
    from bvh_amd import _lib
    pr = prims if isinstance(prims, torch.Tensor) else _cuda(prims)
    q = planes if isinstance(planes, torch.Tensor) else _cuda(np.ascontiguousarray(planes, dtype=tree.dtype))
    n, m = q.shape[0], q.shape[1]
    c = _cuda(np.full(n, 0xABABABAB, dtype=np.uint32)) if counts else None
    cnt = torch.zeros(3, dtype=torch.int64, device="cuda")
    off = lp = li = None
    if offsets is not None:
        off = _cuda(np.ascontiguousarray(offsets, dtype=np.uint64))
        lp = _cuda(np.full(total + 2 * GUARD, SENT_PRIM, dtype=np.uint32))
        if inside:
            li = _cuda(np.full(total + 2 * GUARD, SENT_INSIDE, dtype=np.uint8))
    P = lambda t, skip=0: None if t is None else t.data_ptr() + skip
    rc = entry(bvh, tree.leaf)(bvh._h, P(pr), pr.shape[0], P(q), m, n, flags, P(c), P(off), P(lp, 4 * GUARD), P(li, GUARD), P(cnt), stream)
    assert rc == 0, _lib.last_error()
    return (None if c is None else _np(c, np.uint32)), (None if lp is None else _np(lp, np.uint32)), (None if li is None else _np(li)), \
        _np(cnt).astype(np.uint64)


def device_region(bvh, tree, prims, planes, flags=0):
    """Count pass, bvh_amd_offsets_from_counts, fill pass with inside flags -> what region_ref.host_region returns, with its checks."""
    import bvh_amd
    counts, _, _, cnt0 = device_walk(bvh, tree, prims, planes, flags=flags)
    offsets = _np(bvh_amd.offsets_from_counts(_cuda(counts)), np.uint64)
    total = int(offsets[-1])
    c2, lp, li, cnt = device_walk(bvh, tree, prims, planes, flags=flags, offsets=offsets, total=total, inside=True)
    assert (c2 == counts).all() and (cnt == cnt0).all()
    assert R.guards_intact(lp, total) and R.inside_guards_intact(li, total)
    return offsets, lp[GUARD:GUARD + total], li[GUARD:GUARD + total], counts, cnt


def _same(dev, host):
    for d, h in zip(dev, host):
        if d is None and h is None:
            continue
        assert d.dtype == h.dtype and d.tobytes() == h.tobytes()


def device_tree(tree):
    """The device twin of a harness tree."""
    import bvh_amd
    import oracle
    nodes = np.zeros(len(tree.index), dtype=oracle.NODED if tree.double else oracle.NODEF)
    nodes["bounds"], nodes["index"] = tree.bounds, tree.index
    return bvh_amd.Bvh.from_nodes(nodes, tree.ids.astype(np.uint64))


@pytest.mark.parametrize("scene", GOLDEN_SCENES)
@pytest.mark.parametrize("mode", R.TREES)
def test_device_equals_host_golden(dll, scene, mode):
    import bvh_amd
    tree = R.golden_tree(scene, mode)
    g = load_golden(scene)
    bvh = bvh_amd.Bvh.deserialize(g[f"bvh_{mode}"].tobytes(), dtype=tree.dtype)
    assert bvh._s == ("3d" if tree.double else "3f")
    pr = _cuda(tree.prims)
    for m in (1, 6, 8):
        planes = R.make_regions(tree.prims, 320, m, tree.dtype, 40 + m)
        for exact in ((False, True) if tree.leaf == 0 else (False,)):
            host = R.host_region(dll, tree, planes, exact=exact, threads=8)
            assert host[0][-1] > 0
            _same(device_region(bvh, tree, pr, planes, flags=EXACT if exact else 0), host)
            if m == 6:
                _same(device_region(bvh, tree, pr, planes, flags=ORIGINAL_IDS | (EXACT if exact else 0)),
                      R.host_region(dll, tree, planes, exact=exact, threads=8, original_ids=True))
    # k = 3 slots per query behind a non-zero base: truncated lists, padding, guard zones on the device buffers
    n, k, base = len(planes), 3, 7
    fixed = (base + k * np.arange(n + 1)).astype(np.uint64)
    total = base + k * n + 5
    _same(device_walk(bvh, tree, pr, planes, offsets=fixed, total=total, inside=True), R.host_walk(dll, tree, planes, offsets=fixed, total=total, inside=True))
    _same(device_walk(bvh, tree, pr, planes, offsets=fixed, total=total, counts=False)[1:], R.host_walk(dll, tree, planes, offsets=fixed, total=total, counts=False)[1:])


@pytest.fixture(scope="module")
def soup(dll):
    """soup2k, parallel_high: the device tree, the harness's, 513 regions of 6 planes and the harness's CULL and EXACT lists for them."""
    import bvh_amd
    tree = R.golden_tree("soup2k", "parallel_high")
    bvh = bvh_amd.Bvh.deserialize(load_golden("soup2k")["bvh_parallel_high"].tobytes(), dtype=np.float32)
    q = R.make_regions(tree.prims, 513, 6, np.float32, 21)
    return bvh, tree, _cuda(tree.prims), q, R.host_region(dll, tree, q, threads=8), R.host_region(dll, tree, q, exact=True, threads=8)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_block_edges(soup, n):
    bvh, tree, pr, q, cull, exact = soup
    for flags, (h_off, h_ids, h_ins, h_counts, _) in ((0, cull), (EXACT, exact)):
        off, ids, ins, counts, _ = device_region(bvh, tree, pr, q[:n], flags=flags)
        assert (counts == h_counts[:n]).all() and ids.tobytes() == h_ids[:int(h_off[n])].tobytes() and ins.tobytes() == h_ins[:int(h_off[n])].tobytes()


def test_empty_batch_writes_nothing(soup):
    import torch
    bvh, tree, pr, q, _, _ = soup
    dq = _cuda(q)
    c = _cuda(np.full(8, 0xABABABAB, dtype=np.uint32))
    lp = _cuda(np.full(8, SENT_PRIM, dtype=np.uint32))
    li = _cuda(np.full(8, SENT_INSIDE, dtype=np.uint8))
    off = torch.zeros(9, dtype=torch.int64, device="cuda")
    cnt = torch.full((3,), 77, dtype=torch.int64, device="cuda")
    f = entry(bvh, 0)
    assert f(bvh._h, pr.data_ptr(), pr.shape[0], dq.data_ptr(), 6, 0, 0, c.data_ptr(), off.data_ptr(), lp.data_ptr(), li.data_ptr(), cnt.data_ptr(), None) == 0
    assert f(bvh._h, None, 0, None, 6, 0, 0, None, None, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert (_np(c, np.uint32) == 0xABABABAB).all() and (_np(lp, np.uint32) == SENT_PRIM).all() and (_np(li) == SENT_INSIDE).all() and (_np(cnt) == 77).all()


@pytest.mark.parametrize("depth", [70, 200])
@pytest.mark.parametrize("stacked", [False, True])
def test_trees_deeper_than_64_levels(dll, depth, stacked):
    import query_slices as qs
    tree = R.chain_tree(depth, stacked)
    bvh = device_tree(tree)
    base = qs.chain_base(depth)
    rng = np.random.default_rng(depth)
    n = 300                                                    # not a multiple of the block
    planes = np.zeros((n, 2, 4), dtype=np.float32)
    planes[:, 0] = [0, 0, 1, 0.5]
    planes[:, 1, 0] = 1
    planes[:, 1, 3] = -(base - depth + 10 * rng.random(n))
    planes[::4, 1] = [0, 0, 0, 0]
    cap = depth - 64 + 1                                       # what the launch path sizes the spill to
    for exact in (False, True):
        host = R.host_region(dll, tree, planes, exact=exact, deep_cap=cap)
        assert (host[3][::4] == depth + 1).all()
        _same(device_region(bvh, tree, tree.prims, planes, flags=EXACT if exact else 0), host)


def test_a_deep_tree_takes_several_launches(dll):
    """3000 levels: the 256 MB of spill hold 22 784 lanes' worth, so a batch of 300 more is cut into two launches."""
    from bvh_amd import _lib
    depth = 3000
    tree = R.chain_tree(depth, True)
    bvh = device_tree(tree)
    lanes = (256 << 20) // ((depth - 64 + 1) * 4) // 256 * 256
    n = lanes + 300
    planes = np.zeros((n, 1, 4), dtype=np.float32)
    planes[:] = [1, 0, 0, -1.0]                                 # x <= 1: nothing (the chain sits at x >= 1000) ...
    every = np.arange(0, n, 997)
    planes[every] = [0, 0, 1, 0.5]                              # ... but every 997th region keeps every level alive
    counts, _, _, _ = device_walk(bvh, tree, tree.prims, planes)
    assert _lib.load().bvh_amd_last_query_launches() == 2
    want = np.zeros(n, dtype=np.uint32)
    want[every] = depth + 1
    assert (counts == want).all()


def test_independent_of_position_batch_and_stream(soup):
    import torch
    bvh, tree, pr, q, (h_off, h_ids, h_ins, h_counts, _), _ = soup
    lists = np.split(h_ids, h_off[1:-1].astype(np.int64))
    perm = np.random.default_rng(3).permutation(len(q))
    off, ids, ins, counts, _ = device_region(bvh, tree, pr, q[perm])
    assert (counts == h_counts[perm]).all() and ids.tobytes() == np.concatenate([lists[j] for j in perm]).tobytes()
    off, ids, ins, counts, _ = device_region(bvh, tree, pr, np.repeat(q[100:103], 100, axis=0))          # one region at many positions
    assert ids.tobytes() == np.concatenate([lists[100 + j // 100] for j in range(300)]).tobytes()
    # two streams at once on one const tree
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    parts = [q[:300], q[200:]]
    torch.cuda.synchronize()
    out = []
    for s, part in zip(streams, parts):
        with torch.cuda.stream(s):
            out.append(device_walk(bvh, tree, pr, _cuda(part), stream=C.c_void_p(s.cuda_stream))[0])
    torch.cuda.synchronize()
    assert (out[0] == h_counts[:300]).all() and (out[1] == h_counts[200:]).all()


def test_moving_geometry(dll):
    """Build on soup2k, move every triangle, refit_tris: region_search on the moved triangles equals the brute force on them."""
    import bvh_amd
    raw = load_golden("soup2k")["prims"]
    bb, cc = bvh_amd.tri_bounds(raw)
    bvh = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.High))
    pts = raw.reshape(-1, 3)
    diag = float(np.linalg.norm(pts.max(axis=0) - pts.min(axis=0)))
    rng = np.random.default_rng(17)
    shift = ((rng.random((len(raw), 1, 3)) * 2 - 1) * 0.05 * diag).astype(np.float32)
    moved = np.ascontiguousarray((raw.reshape(-1, 3, 3) + shift).reshape(-1, 9))
    bvh.refit_tris(moved)
    nodes = bvh.nodes
    tree = R.PrimTree(nodes["bounds"], nodes["index"], moved, bvh.prim_ids)
    planes = R.make_regions(moved, 384, 6, np.float32, 29)
    match, inside = R.brute_cull(tree.ordered(), planes)
    wc, wi = R.expected_lists(match, tree.dfs)
    off, lst, ins = bvh_amd.region_search(bvh, moved, planes, inside=True)
    assert (np.diff(_np(off)) == wc).all() and _np(lst, np.uint32).tobytes() == wi.tobytes() and len(wi) > 384
    assert _np(ins).tobytes() == R.expected_inside(match, inside, tree.dfs).tobytes()
    q, i = np.nonzero(match)
    _, e, _ = R.host_pairs(dll, tree.ordered()[i], planes[q], np.float32)
    em = match.copy()
    em[q, i] = e
    ec, ei = R.expected_lists(em, tree.dfs)
    off, lst = bvh_amd.region_search(bvh, moved, planes, exact=True, original_ids=True)
    assert (np.diff(_np(off)) == ec).all() and (_np(lst) == tree.ids[ei.astype(np.int64)]).all() and len(ei) < len(wi)


def test_refusals(soup):
    import bvh_amd
    import torch
    from bvh_amd import _lib
    bvh, tree, pr, q, _, _ = soup
    n, m = q.shape[0], q.shape[1]
    dq = _cuda(q)
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    offs = torch.arange(n + 1, dtype=torch.int64, device="cuda") * 2
    lp = torch.zeros(2 * n + 4, dtype=torch.int32, device="cuda")
    li = torch.zeros(2 * n + 4, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    ft, fs = entry(bvh, 0), entry(bvh, 1)
    P = lambda t: t.data_ptr()
    npr = pr.shape[0]

    def refused(rc, word):
        assert rc == -2 and word in _lib.last_error(), (rc, _lib.last_error())

    assert ft(bvh._h, P(pr), npr, P(dq), m, n, 0, P(counts), P(offs), P(lp), P(li), P(cnt), None) == 0
    assert ft(bvh._h, P(pr), npr, P(dq), m, n, EXACT | ORIGINAL_IDS, P(counts), P(offs), P(lp), None, None, None) == 0
    for bad in (1, 2, 32, 128, 1 << 20, SORTED, UNSORTED, SORTED | ORIGINAL_IDS):                # ANY_HIT, ROBUST, SKIP_SHARED, unknown bits, reordering
        refused(ft(bvh._h, P(pr), npr, P(dq), m, n, bad, P(counts), None, None, None, None, None), "flags")
        refused(fs(bvh._h, P(pr), npr, P(dq), m, n, bad, P(counts), None, None, None, None, None), "flags")
    refused(fs(bvh._h, P(pr), npr, P(dq), m, n, EXACT, P(counts), None, None, None, None, None), "REGION_EXACT")     # EXACT on spheres
    for bad_m in (0, 9, 1 << 40):
        refused(ft(bvh._h, P(pr), npr, P(dq), bad_m, 1, 0, P(counts), None, None, None, None, None), "planes per query")
    refused(ft(None, P(pr), npr, P(dq), m, n, 0, P(counts), None, None, None, None, None), "null bvh")
    refused(ft(bvh._h, None, npr, P(dq), m, n, 0, P(counts), None, None, None, None, None), "null device pointer")
    refused(ft(bvh._h, P(pr), npr, None, m, n, 0, P(counts), None, None, None, None, None), "null device pointer")
    refused(ft(bvh._h, P(pr), npr, P(dq), m, n, 0, None, None, None, None, None, None), "d_counts")                  # neither counts nor offsets
    refused(ft(bvh._h, P(pr), npr, P(dq), m, n, 0, P(counts), P(offs), None, None, None, None), "d_list_prims")      # offsets without a list
    refused(ft(bvh._h, P(pr), npr, P(dq), m, n, 0, P(counts), None, P(lp), None, None, None), "lists need d_offsets")
    refused(ft(bvh._h, P(pr), npr, P(dq), m, n, 0, P(counts), None, None, P(li), None, None), "lists need d_offsets")   # d_list_inside without offsets
    for args in ((P(pr) + 2, npr - 1, P(dq), m, n, 0, P(counts), None, None, None, None, None),   # misaligned primitives, planes, counts,
                 (P(pr), npr, P(dq) + 2, m, n - 1, 0, P(counts), None, None, None, None, None),   # offsets, list, counters
                 (P(pr), npr, P(dq), m, n, 0, P(counts) + 2, None, None, None, None, None),
                 (P(pr), npr, P(dq), m, n, 0, P(counts), P(offs) + 4, P(lp), None, None, None),
                 (P(pr), npr, P(dq), m, n, 0, P(counts), P(offs), P(lp) + 2, None, None, None),
                 (P(pr), npr, P(dq), m, n, 0, P(counts), None, None, None, P(cnt) + 4, None)):
        refused(ft(bvh._h, *args), "aligned")
    # alignment to the element is enough: planes from their second scalar on, counts and lists from their second entry
    assert ft(bvh._h, P(pr), npr, P(dq) + 4, m, n - 1, 0, P(counts) + 4, P(offs) + 8, P(lp) + 4, P(li) + 1, P(cnt) + 8, None) == 0, _lib.last_error()
    largest = int(tree.ids.max())
    for bad_n in (largest, largest - 5, 1):                                                      # n_prims at or below the largest prim id
        refused(ft(bvh._h, P(pr), bad_n, P(dq), m, n, 0, P(counts), None, None, None, None, None), "prim_ids refers")
    assert ft(bvh._h, P(pr), largest + 1, P(dq), m, n, 0, P(counts), None, None, None, None, None) == 0
    # (Not checked: "BVH has no device copy" and "BVH has no device prim ids". Every constructor the library has - the builders,
    #  from_nodes, deserialize, load, extract - uploads the tree and its prim ids before it returns a handle, so no handle without
    #  them can be made from Python or C; the sibling list queries leave these two refusals unchecked for the same reason.)
    # a 2D tree
    g2 = load_golden("circles2k_2f")
    b2, c2 = bvh_amd.sphere_bounds(g2["prims"])
    bvh2 = bvh_amd.DefaultBuilder.build(b2, c2)
    refused(ft(bvh2._h, P(pr), npr, P(dq), m, n, 0, P(counts), None, None, None, None, None), "3D trees only")
    for call in (lambda: bvh_amd.region_count(bvh2, tree.prims, q), lambda: bvh_amd.region_search(bvh, tree.prims.astype(np.float64), q),
                 lambda: bvh_amd.region_count(bvh, tree.prims, q.astype(np.float64))):
        with pytest.raises(TypeError):
            call()
    for call in (lambda: bvh_amd.region_count(bvh, tree.prims, np.zeros((4, 9, 4), np.float32)), lambda: bvh_amd.region_count(bvh, tree.prims, q[:, :, :3]),
                 lambda: bvh_amd.region_count(bvh, tree.prims[:, :4], q, leaf="sphere", exact=True)):
        with pytest.raises(ValueError):
            call()


def test_python_layer(soup):
    import bvh_amd
    import torch
    bvh, tree, pr, q, (h_off, h_ids, h_ins, h_counts, h_cnt), (e_off, e_ids, e_ins, e_counts, _) = soup
    n = len(q)
    c = bvh_amd.region_count(bvh, tree.prims, q)
    assert c.dtype == torch.int32 and c.shape == (n,) and (_np(c, np.uint32) == h_counts).all()
    c, cnt = bvh_amd.region_count(bvh, pr, _cuda(q), exact=True, counters=True)
    assert (_np(c, np.uint32) == e_counts).all() and cnt.dtype == torch.int64 and int(cnt[1]) > 0
    off, ids = bvh_amd.region_search(bvh, pr, q)
    assert off.dtype == torch.int64 and off.shape == (n + 1,) and ids.dtype == torch.int32 and ids.shape == (len(h_ids),)
    assert _np(off, np.uint64).tobytes() == h_off.tobytes() and _np(ids, np.uint32).tobytes() == h_ids.tobytes()
    off, ids, ins, cnt = bvh_amd.region_search(bvh, pr, q, exact=True, inside=True, counters=True)
    assert ins.dtype == torch.uint8 and _np(ids, np.uint32).tobytes() == e_ids.tobytes() and _np(ins).tobytes() == e_ins.tobytes() and int(cnt[0]) > 0
    off, oids = bvh_amd.region_search(bvh, pr, q, original_ids=True)
    assert (_np(oids) == tree.ids[h_ids.astype(np.int64)]).all()
    k = 4
    off, ids, ins, counts = bvh_amd.region_search(bvh, pr, q, max_per_query=k, inside=True)
    assert (_np(off) == k * np.arange(n + 1)).all() and ids.shape == (n * k,) and ins.shape == (n * k,) and (_np(counts, np.uint32) == h_counts).all()
    rows, flg = _np(ids).reshape(n, k), _np(ins).reshape(n, k)
    for i in range(n):
        m = min(int(h_counts[i]), k)
        assert (rows[i, :m].view(np.uint32) == h_ids[int(h_off[i]):int(h_off[i]) + m]).all() and (rows[i, m:] == -1).all()
        assert (flg[i, :m] == h_ins[int(h_off[i]):int(h_off[i]) + m]).all() and (flg[i, m:] == 0).all()
    assert h_counts.max() > k and (h_counts < k).any()
    e_off, e_ids = bvh_amd.region_search(bvh, pr, np.zeros((0, 6, 4), np.float32))
    assert e_off.tolist() == [0] and e_ids.shape == (0,) and bvh_amd.region_count(bvh, pr, np.zeros((0, 6, 4), np.float32)).shape == (0,)


def test_frustum_planes_hold_what_the_camera_sees():
    """pinhole_rays' own frustum (fov_y = pi / 2, aspect = 1): the triangle every primary ray hits shares a point with the frustum, so
    it is in the frustum's EXACT list."""
    import bvh_amd
    raw = load_golden("soup2k")["prims"]
    bb, cc = bvh_amd.tri_bounds(raw)
    bvh = bvh_amd.DefaultBuilder.build(bb, cc)
    pts = raw.reshape(-1, 3).astype(np.float64)
    centre, diag = (pts.min(axis=0) + pts.max(axis=0)) / 2, float(np.linalg.norm(pts.max(axis=0) - pts.min(axis=0)))
    eye, up = centre + np.array([0.1, 0.2, -0.9]) * diag / 3, np.array([0.0, 1.0, 0.0])      # inside the soup: part of it is behind the camera
    direction = centre - eye
    rays = bvh_amd.pinhole_rays(48, 32, eye, direction, up)
    hits = bvh_amd.hits_to_numpy(bvh_amd.intersect(bvh, bvh_amd.precompute_tris(raw, bvh.device_prim_ids()), rays))
    seen = np.unique(hits["prim"][hits["prim"] != R.INVALID])
    assert len(seen) > 50
    planes = bvh_amd.frustum_planes(eye, direction, up, np.pi / 2, 1.0, 0.0, 10 * diag)[None]
    assert planes.shape == (1, 6, 4) and planes.dtype == np.float32
    assert np.allclose(np.linalg.norm(planes[0, :2, :3], axis=1), 1) and (planes[0, :, :3] @ (centre - eye) < 0).sum() >= 5     # normals point out
    off, ids = bvh_amd.region_search(bvh, raw, planes, exact=True)
    listed = set(_np(ids).tolist())
    assert set(seen.tolist()) <= listed and len(listed) < bvh.prim_count
    off, cull = bvh_amd.region_search(bvh, raw, planes)
    assert listed <= set(_np(cull).tolist())
