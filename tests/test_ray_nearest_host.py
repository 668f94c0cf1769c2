"""CPU: the TEXT of the nearest-hits ray kernel (bvh_amd/csrc/ray_nearest_body.inc + knn_heap.inc + tri_test.inc + trace_device.h)
compiled for the host by tests/cpp/ray_nearest_body_host.cpp, held to the unmodified reference: each ray's row must be the
reference's own hit list (tests/ray_hits_ref.py: the reference's intersect, one primitive at a time) sorted by (t, prim) and cut at
k, byte for byte, padded with the miss record. ZERO rows may differ: there is no tolerance anywhere in this file.

Also here: k = 1 against the reference's closest-hit; scenes in which t ties exactly; two deliberately wrong walks that these checks
must reject; the shapes of the output (padding, guard zones, ORIGINAL_IDS, the order array, edge rays); trees deeper than 64 levels
and one sliced launch; the pruning counter; the exported symbols. The device's rows, counts and counters must equal this harness's
bit for bit (tests/test_gpu_ray_nearest.py)."""
import os
import re

import numpy as np
import pytest

import query_slices as qs
from conftest import ROOT
from ray_hits_ref import INVALID, reference_lib, reference_records
from ray_nearest_ref import (K_DENSE, K_TINY, MAX_K, _p, block_lanes, compile_harness, differing_rows, expected_rows, first_two_tie, grid_case,
                             guarded_records, hit_dtype, host_nearest, miss_rows, record_guards_intact, sorted_lists)
from test_closest_point_host import GOLDEN_SCENES
from test_radius_search_host import Tree
from test_ray_hits_host import _hand_tree, chain, chain_rays, golden_case, seeded_case
from test_ray_hits_host import compile_harness as compile_all_hits
from test_ray_hits_host import host_walk as all_hits_walk


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return compile_harness(tmp_path_factory.mktemp("ray_nearest"))


@pytest.fixture(scope="module")
def lib():
    return reference_lib()


_LISTS = {}


def lists_of(key, tree, ref, robust):
    """The reference's sorted lists of a cached case, computed once."""
    if (key, robust) not in _LISTS:
        _LISTS[(key, robust)] = sorted_lists(*ref[robust], tree.index)
    return _LISTS[(key, robust)]


def check_rows(dll, tree, rays, lists, k, robust, mutant=0, **kw):
    """The walk's rows and counts at k against the reference-derived ones. Returns the number of rows the reference's lists show k to cut."""
    all_counts, sorted_ = lists
    want, want_counts = expected_rows(tree, rays, sorted_, k, kw.get("prim_ids"))
    got, counts, _ = host_nearest(dll, tree, rays, k, robust=robust, mutant=mutant, **kw)
    diff = differing_rows(got, want)
    assert diff == 0, f"k={k}: {diff} of {len(rays)} rows differ"
    assert (counts == want_counts).all()
    return int((all_counts > k).sum())


@pytest.mark.parametrize("robust", [False, True])
@pytest.mark.parametrize("n_prims", [1, 2, 3, 200])
@pytest.mark.parametrize("kind", ["tri", "sphere"])
def test_rows_equal_reference_seeded(dll, lib, kind, n_prims, robust):
    tree, rays, ref, _, _ = seeded_case(lib, kind, n_prims)
    lists = lists_of((kind, n_prims), tree, ref, robust)
    cut = {k: check_rows(dll, tree, rays, lists, k, robust, threads=4) for k in (K_DENSE if n_prims == 200 else K_TINY)}
    print(f"{kind} x {n_prims} robust={robust}: rows cut by k: {cut}; longest list {lists[0].max()}")
    if n_prims == 200:
        # a case counts only where the reference's own lists show that k cuts rows: every k below 64 does here, on a quarter of the
        # rays at 1 and 2 and on some ray up to 33, so all three block sizes (k = 1 / 9 / 16, 17, 33) are held to the reference on rows
        # that are cut. k = 64 is NOT a cutting case on these scenes (the longest list has 56 / 45 records): there the row is the whole
        # sorted list; rows cut at 64 are those of the robust grid (test_ties_layered_grid) and of the chains (test_deep_chain)
        assert cut[1] >= len(rays) // 4 and cut[2] >= len(rays) // 4
        for k in (1, 2, 3, 8, 9, 16, 17, 33):
            assert cut[k] > 0, (k, cut)
        assert cut[64] == 0 and 33 < lists[0].max() <= 64
    else:
        assert cut[1] > 0 or n_prims == 1                      # (two or three dense primitives: some ray crosses two)
        assert cut[64] == 0                                    # nothing to cut: the row is the whole sorted list


@pytest.mark.parametrize("robust", [False, True])
@pytest.mark.parametrize("scene", GOLDEN_SCENES)
def test_rows_equal_reference_golden(dll, lib, orc, scene, robust):
    tree, rays, ref, ids, _ = golden_case(lib, orc, scene)
    lists = lists_of(("golden", scene), tree, ref, robust)
    cut = {k: check_rows(dll, tree, rays, lists, k, robust, threads=4) for k in K_DENSE}
    print(f"{scene} robust={robust}: rows cut by k: {cut}; longest list {lists[0].max()}")
    assert cut[1] > 0                                          # (the all-hits tests assert a ray with two hits in every golden scene)
    # original ids map the reported prim only: the order stays that of the BVH-order index
    for k in (1, 3):
        check_rows(dll, tree, rays, lists, k, robust, prim_ids=ids.astype(np.uint32))
    # reading the batch through a permuted order changes nothing
    perm = np.random.default_rng(5).permutation(len(rays)).astype(np.uint32)
    check_rows(dll, tree, rays, lists, 3, robust, order=perm)


def closest_of(lib, tree, nodes, rays, robust):
    bvh = lib.from_arrays(np.ascontiguousarray(nodes), np.arange(len(tree.prims), dtype=np.uint64))
    out = (bvh.intersect_sphere if tree.leaf else bvh.intersect_tri)(tree.prims, rays, any_hit=False, robust=robust)
    if "pad" in out.dtype.names:
        out["pad"] = 0
    return out


def check_k1_against_closest(row1, closest, sorted_):
    """k = 1 against closest-hit: the same hit / miss, the same t bits, the same prim wherever the reference's list has no second
    record at that t. Returns how many rays tie there."""
    bits = np.uint64 if row1["t"].dtype == np.float64 else np.uint32
    hit = closest["prim"] != INVALID
    assert ((row1["prim"] != INVALID) == hit).all()
    assert (np.ascontiguousarray(row1["t"]).view(bits) == np.ascontiguousarray(closest["t"]).view(bits)).all()      # (a miss: tmax both)
    tie = first_two_tie(sorted_)
    assert (row1["prim"][hit & ~tie] == closest["prim"][hit & ~tie]).all()
    return int((hit & tie).sum())


@pytest.mark.parametrize("robust", [False, True])
@pytest.mark.parametrize("case", ["tri200", "sphere200", "grid"] + GOLDEN_SCENES)
def test_k1_is_closest_hit(dll, lib, orc, case, robust):
    if case == "grid":
        tree, rays, ref, _, nodes = grid_case(lib)
    elif case in GOLDEN_SCENES:
        tree, rays, ref, _, nodes = golden_case(lib, orc, case)
    else:
        tree, rays, ref, _, nodes = seeded_case(lib, case[:-3], 200)
    _, sorted_ = lists_of(("k1", case), tree, ref, robust)
    rows, counts, _ = host_nearest(dll, tree, rays, 1, robust=robust)
    closest = closest_of(lib, tree, nodes, rays, robust)
    ties = check_k1_against_closest(rows[:, 0], closest, sorted_)
    print(f"{case} robust={robust}: {int((closest['prim'] != INVALID).sum())} hits, {ties} with a tie at the nearest t")
    assert (counts == (closest["prim"] != INVALID)).all() and counts.sum() > 0


def test_ties_spheres(dll, lib):
    """Rays that start inside several spheres have t0 = tmin for all of them: the rows must order those by index. A batch of 4096
    rays on the seeded 200-sphere scene; an eighth of them must tie (a quarter start inside the cube of overlapping spheres)."""
    tree, rays, ref, _, _ = seeded_case(lib, "sphere", 200, n_rays=4096)
    assert len(rays) == 4096
    for robust in (False, True):
        lists = lists_of(("sphere", 200, 4096), tree, ref, robust)
        tie = first_two_tie(lists[1])
        print(f"spheres robust={robust}: {int(tie.sum())} of {len(rays)} rays tie at their first two records")
        assert tie.sum() >= len(rays) // 8
        for k in (1, 2, 3, 8):
            assert check_rows(dll, tree, rays, lists, k, robust, threads=4) > 0      # (cut rows, on the reference's counts)


def test_ties_layered_grid(dll, lib):
    tree, rays, ref, ids, _ = grid_case(lib)
    for robust in (False, True):
        lists = lists_of(("grid",), tree, ref, robust)
        tie = first_two_tie(lists[1])
        cut = {k: check_rows(dll, tree, rays, lists, k, robust) for k in (1, 2, 3, 8, 9, 16, 17, 33, 64)}
        print(f"grid robust={robust}: {int(tie.sum())} of {len(rays)} rays tie at their first two records; longest list {lists[0].max()}; rows cut by k: {cut}")
        assert tie.sum() >= len(rays) // 4
        # which k cut rows here, on the reference's counts. Fast node test: a ray crosses at most the 8 layers' three triangles (24), so
        # k <= 17 cut and 33, 64 return whole lists. Robust: rays along a quad's edge or diagonal also pass the padded boxes of the
        # neighbours (lists of up to 72), so every k cuts, 64 included: the one scene held to the reference whose rows are cut at 64
        for k in (1, 2, 3, 8, 9, 16, 17):
            assert cut[k] > 0, (robust, k, cut)
        if robust:
            assert cut[33] > 0 and cut[64] > 0 and lists[0].max() > 64
        else:
            assert cut[33] == 0 and cut[64] == 0 and lists[0].max() == 24
        check_rows(dll, tree, rays, lists, 2, robust, prim_ids=ids.astype(np.uint32))      # ties still sort by the BVH-order index


def test_the_checks_bite(dll, lib):
    """Mutant 1 (on equal t the later-tested primitive wins) must fail where t ties; mutant 2 (a sphere's t1 clipped to the shortened
    tmax) must fail on the overlapping spheres. The body passes both, and each mutant passes where its fault cannot show."""
    grid, grays, gref, _, _ = grid_case(lib)
    glists = lists_of(("grid",), grid, gref, False)
    sph, srays, sref, _, _ = seeded_case(lib, "sphere", 200)
    slists = lists_of(("sphere", 200), sph, sref, False)
    for k in (1, 2, 8):
        check_rows(dll, grid, grays, glists, k, False)
        with pytest.raises(AssertionError):
            check_rows(dll, grid, grays, glists, k, False, mutant=1)
        check_rows(dll, grid, grays, glists, k, False, mutant=2)              # (triangles have no t1 to clip)
    for k in (1, 2, 8):
        check_rows(dll, sph, srays, slists, k, False)
        with pytest.raises(AssertionError):
            check_rows(dll, sph, srays, slists, k, False, mutant=2)
    # mutant 1 at k = 1 is closest-hit's rule: where rays tie it reports the reference's closest-hit prim, which the body does not
    tri, trays, tref, _, _ = seeded_case(lib, "tri", 200)
    check_rows(dll, tri, trays, lists_of(("tri", 200), tri, tref, False), 8, False, mutant=1)     # (no ties among random triangles)


def test_output_shapes(dll, lib):
    tree, rays, ref, _, _ = seeded_case(lib, "tri", 200)
    all_counts, sorted_ = lists_of(("tri", 200), tree, ref, False)
    k = 4
    assert (all_counts > k).any() and (all_counts < k).any() and (all_counts == 0).any()
    want, want_counts = expected_rows(tree, rays, sorted_, k)
    got, counts, _ = host_nearest(dll, tree, rays, k)          # (guards around rows and counts: checked inside)
    assert differing_rows(got, want) == 0 and (counts == want_counts).all()
    # padding: the miss record with the ray's own tmax
    pad = miss_rows(tree, rays, k)
    for r in range(len(rays)):
        assert got[r, counts[r]:].tobytes() == pad[r, counts[r]:].tobytes()
        assert (got[r, :counts[r]]["prim"] != INVALID).all()
    # without counts: the same rows
    got2, none, _ = host_nearest(dll, tree, rays, k, counts=False)
    assert none is None and got2.tobytes() == got.tobytes()
    # any LDS stride, any split over threads: the same rows
    for stride in (2, 64, 128, 256):
        g, c, cnt = host_nearest(dll, tree, rays, k, stride=stride, threads=3)
        assert g.tobytes() == got.tobytes() and (c == counts).all()
    # double spheres: the same protocol on 32-byte records {prim, t0, t1, 0}
    tree, rays, ref, _, _ = seeded_case(lib, "sphere", 200)
    got, counts, _ = host_nearest(dll, tree, rays, k, robust=True)
    for r in range(len(rays)):
        m = int(counts[r])
        assert (got[r, :m]["v"] == 0).all() and (got[r, :m]["t"] <= got[r, :m]["u"]).all() and (got[r, :m]["pad"] == 0).all()
        assert (np.diff(got[r, :m]["t"]) >= 0).all()
        assert (got[r, :m]["u"] <= rays[r, 7]).all()           # t1 = min(exit, the ray's OWN tmax)


def test_sphere_t1_is_never_clipped_to_the_shortened_tmax(dll, lib):
    """Some row of the overlapping spheres holds a record whose t1 lies beyond the row's last t0: the shortened tmax did not leak."""
    tree, rays, _, _, _ = seeded_case(lib, "sphere", 200)
    got, counts, _ = host_nearest(dll, tree, rays, 2)
    full = counts == 2
    assert full.any() and (got[full, 0]["u"] > got[full, 1]["t"]).any()


def test_edge_rays(dll, lib):
    """NaN tmin / tmax: count 0 and a fully padded row carrying the ray's own tmax bits. tmin > tmax, a zero direction, NaN
    components: walked, with whatever the reference's tests give."""
    nodes, prims = _hand_tree()
    tree = Tree(nodes["bounds"], nodes["index"], prims, 0)
    nan, inf = np.nan, np.inf
    rays = np.array([[-1, 0, 0, 1, 0, 0, nan, 100], [-1, 0, 0, 1, 0, 0, 0, nan], [-1, 0, 0, 1, 0, 0, nan, nan],
                     [-1, 0, 0, 1, 0, 0, 4, 2],                # tmin > tmax
                     [-1, 0, 0, 0, 0, 0, 0, 100],              # zero direction
                     [2, 0, 0, 0, 0, 0, 0, 100],               # zero direction, origin ON a triangle
                     [nan, 0, 0, 1, 0, 0, 0, 100], [-1, 0, 0, 1, nan, 0, 0, 100],
                     [-1, 0, 0, 1, 0, 0, -inf, inf],           # the whole line
                     [5, 0, 0, -1, 0, 0, 0, 100],              # from behind: the tree's far end first
                     [-1, 0, 0, 1, 0, 0, 0, 100]], dtype=np.float32)
    tmax_bits = rays[:, 7].copy()
    tmax_bits.view(np.uint32)[1] = 0x7FC12345                  # a NaN with a payload: the padding carries these very bits
    rays[:, 7] = tmax_bits
    for robust in (False, True):
        lists = sorted_lists(*reference_records(lib, nodes, prims, rays, 0, robust), nodes["index"])
        assert lists[0][:4].tolist() == [0, 0, 0, 0] and lists[0][8:].tolist() == [5, 5, 5]
        for k in (1, 2, 5, 64):
            want, want_counts = expected_rows(tree, rays, lists[1], k)
            got, counts, _ = host_nearest(dll, tree, rays, k, robust=robust)
            assert differing_rows(got, want) == 0 and (counts == want_counts).all()
        got, counts, _ = host_nearest(dll, tree, rays, 3, robust=robust)
        assert got[1, 0]["t"].view(np.uint32) == 0x7FC12345
        assert got[8]["prim"].tolist() == [0, 1, 2] and got[8]["t"].tolist() == [1, 2, 3]
        assert got[9]["prim"].tolist() == [4, 3, 2] and got[9]["t"].tolist() == [1, 2, 3]
    # a root that is a leaf is tested without a box test
    tree1, rays1, ref1, _, _ = seeded_case(lib, "tri", 1)
    assert (tree1.root & 15) == 1
    got, c, cnt = host_nearest(dll, tree1, rays1, 2)
    assert c.sum() > 0 and cnt[0] == 0 and cnt[2] == len(rays1) and cnt[1] == len(rays1)


def chain_expected(tree, rays, depth, k):
    """The chain's rows written out: triangle j at x = 4000 - j, t exact in float (small integers and one subtraction); the nearest is
    the deepest."""
    t_of = np.float32(4000) - np.arange(depth + 1, dtype=np.float32)[None, :] - rays[:, 0:1]
    lists = []
    for r in range(len(rays)):
        js = [j for j in range(depth, -1, -1) if t_of[r, j] <= rays[r, 7]]
        seg = np.zeros(len(js), dtype=np.dtype([("prim", "<u4"), ("t", "<f4"), ("u", "<f4"), ("v", "<f4")]))
        seg["prim"], seg["t"] = js, t_of[r, js]
        lists.append(seg)
    return lists


@pytest.mark.parametrize("depth", [70, 300])
@pytest.mark.parametrize("stacked", [False, True])
def test_deep_chain(dll, orc, depth, stacked):
    """A ray from in front of the chain's far end enters the rest of the chain before each level's leaf: near-first, it stacks one
    leaf per level whichever side the leaves are on, through LDS (8), scratch (to 64) and the HBM spill. Then the stack unwinds
    against `worst`. Expected: the k nearest triangles in front of tmax, which are the deepest; (u, v) from the all-hits harness."""
    tree, nodes = chain(depth, orc.prep_tris, stacked)
    rays = chain_rays(depth, 48)
    cap = depth - 64 + 1
    all_dll = compile_all_hits(os.path.dirname(dll._name))
    for k in (1, 3, 17, 64):
        want_lists = chain_expected(tree, rays, depth, k)
        got, counts, _ = host_nearest(dll, tree, rays, k, deep_cap=cap, threads=2)
        for r in range(len(rays)):
            m = min(len(want_lists[r]), k)
            assert counts[r] == m
            assert got[r, :m]["prim"].tolist() == want_lists[r]["prim"][:m].tolist(), r
            assert (got[r, :m]["t"] == want_lists[r]["t"][:m]).all()
        assert (counts[::4] == min(k, depth + 1)).all() and 0 < counts[1::4].min()
    # k = 64 against the all-hits walk of the same rays, sorted: byte for byte
    c, _, _ = all_hits_walk(all_dll, tree, rays, deep_cap=cap)
    assert (c[::4] == depth + 1).all() and depth + 1 > 64      # every 4th ray crosses all levels: its row is CUT at 64
    offsets = np.concatenate([[0], np.cumsum(c.astype(np.uint64))]).astype(np.uint64)
    _, buf, _ = all_hits_walk(all_dll, tree, rays, offsets=offsets, total=int(offsets[-1]), deep_cap=cap)
    flat = buf[8:8 + int(offsets[-1])]
    sorted_ = [np.sort(flat[int(offsets[r]):int(offsets[r + 1])], order=["t", "prim"]) for r in range(len(rays))]
    want, want_counts = expected_rows(tree, rays, sorted_, 64)
    got, counts, _ = host_nearest(dll, tree, rays, 64, deep_cap=cap)
    assert differing_rows(got, want) == 0 and (counts == want_counts).all()


def run_sliced(dll, tree, rays, k, per, cap, robust=False, order=None, prim_ids=None):
    """The batch over the launches of `per` slots as point_query_run cuts it -> (rows, counts, query_slices.Sliced)."""
    from test_kernel_body_host import _aligned
    r = _aligned(np.ascontiguousarray(rays, dtype=tree.dtype))
    n_all = len(r)
    stride = block_lanes(tree, k)
    buf, rows = guarded_records(hit_dtype(tree), n_all * k)
    counts = np.full(n_all, 0xABABABAB, dtype=np.uint32)
    order = None if order is None else np.ascontiguousarray(order, dtype=np.uint32)
    prim_ids = None if prim_ids is None else np.ascontiguousarray(prim_ids, dtype=np.uint32)
    run = qs.Sliced()
    for first, n in qs.slices(n_all, per):
        cnt = np.zeros(3, dtype=np.uint64)
        run.add(dll.ray_nearest_host_walk_slice(int(tree.double), tree.leaf, int(robust), _p(tree.pairs), tree.root, _p(tree.prims), _p(r), first, n, per,
                                                k, stride, _p(order), _p(prim_ids), cap, _p(rows), _p(counts), _p(cnt)), cnt)
    assert record_guards_intact(buf, n_all * k)
    return rows.reshape(n_all, k).copy(), counts, run


def test_sliced_launch_emulation(dll, orc):
    """One batch cut into launches of one block over the 70-level chain: slot = first + lane, the spill indexed by the lane and sized
    for the launch. The same bytes and counters as the unsliced walk, the guard zones of spill and LDS untouched."""
    depth, k = 70, 16
    tree, _ = chain(depth, orc.prep_tris, True)
    rays = chain_rays(depth, 300)
    cap = qs.deep_cap(depth)
    want, want_counts, want_cnt = host_nearest(dll, tree, rays, k, deep_cap=cap)
    per = block_lanes(tree, k)
    assert per == 64
    perm = np.random.default_rng(3).permutation(len(rays)).astype(np.uint32)
    for order in (None, perm):
        got, counts, run = run_sliced(dll, tree, rays, k, per, cap, order=order)
        run.check(len(qs.slices(len(rays), per)))              # (every 4th ray stacks on every level: each launch uses its spill)
        assert got.tobytes() == want.tobytes() and (counts == want_counts).all() and (run.total() == want_cnt).all()
    from test_kernel_body_host import _aligned
    r = _aligned(np.ascontiguousarray(rays))
    assert dll.ray_nearest_host_walk_slice(0, 0, 0, _p(tree.pairs), tree.root, _p(tree.prims), _p(r), 0, 300, 256, k, per, None, None, cap, _p(got),
                                           _p(counts), _p(np.zeros(3, dtype=np.uint64))) == -2


def test_the_walk_prunes(dll, lib):
    """At k = 8 the walk tests fewer primitives than the all-hits walk of the same rays, and no more than at k = 64; k >= every list's
    length prunes nothing, so it fetches and tests exactly what all-hits does."""
    tree, rays, ref, _, _ = seeded_case(lib, "tri", 200)
    all_dll = compile_all_hits(os.path.dirname(dll._name))
    _, _, cnt_all = all_hits_walk(all_dll, tree, rays)
    assert lists_of(("tri", 200), tree, ref, False)[0].max() <= 64
    cnt = {k: host_nearest(dll, tree, rays, k)[2] for k in (1, 8, 64)}
    print(f"prim_tests: k=1 {cnt[1][1]}, k=8 {cnt[8][1]}, k=64 {cnt[64][1]}, all-hits {cnt_all[1]}; pairs {cnt[1][0]}, {cnt[8][0]}, {cnt[64][0]}, {cnt_all[0]}")
    assert cnt[8][1] < cnt_all[1] and cnt[8][0] < cnt_all[0]
    assert cnt[1][1] < cnt[8][1] <= cnt[64][1]
    assert (cnt[64] == cnt_all).all()


def test_ray_nearest_symbols_are_declared_and_exported():
    from bvh_amd import _lib, build
    build.build()
    dll = _lib.load()
    header = open(os.path.join(ROOT, "include", "bvh_amd.h")).read()
    declared = set(re.findall(r"BVH_AMD_API[^;]*?\b(bvh\w+)\s*\(", header))
    want = {f"bvh{s}_intersect_rays_nearest_{leaf}" for s in ("3f", "3d") for leaf in ("tri", "sphere")}
    assert {n for n in declared if "rays_nearest" in n} == want
    assert want <= set(_lib.exported_symbols())
    for name in sorted(want):
        assert hasattr(dll, name), name
    for s in ("2f", "2d"):
        for leaf in ("tri", "sphere"):
            assert not hasattr(dll, f"bvh{s}_intersect_rays_nearest_{leaf}")
            assert f"bvh{s}_intersect_rays_nearest_{leaf}" not in _lib.exported_symbols()
    assert re.search(r"#define\s+BVH_AMD_RAY_NEAREST_MAX_K\s+64\b", header) and MAX_K == 64
    import bvh_amd
    assert bvh_amd.RAY_NEAREST_MAX_K == 64
