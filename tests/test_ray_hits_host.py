"""CPU: the TEXT of the all-hits ray kernel (bvh_amd/csrc/ray_hits_body.inc + list_walk.inc + tri_test.inc + trace_device.h) compiled for
the host by tests/cpp/ray_hits_body_host.cpp, held to the unmodified reference (tests/ray_hits_ref.py: the reference's own intersect,
one primitive at a time): the same primitives per ray, byte-equal records, in the tree's left-first depth-first order; the shapes of
the output (count pass, exact offsets, fixed segments, padding, guard records); edge rays; a hand-written walk order; trees deeper than
64 levels; two deliberately wrong walks that these checks must reject; the exported symbols. The device's counts and records must
equal this harness's bit for bit (tests/test_gpu_ray_hits.py).

Density. The seeded 200-primitive scenes (large overlapping triangles / spheres in the unit cube, rays aimed through it) are where a
list is long: the reference's own counts there must show >= 3 hits on at least a quarter of the rays and >= 8 on some ray. The golden
scenes are what they are (the 2k soups are sparse: 1 % of the rays cross 3 triangles); half of their rays are aimed at points on
primitives, and they must show hits at all and some ray with two."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
from conftest import ROOT
from ray_hits_ref import (INVALID, build_tree, dense_spheres, dense_tris, dfs_prim_order, expected_lists, points_on, rays_through, reference_lib,
                          reference_records)
from test_closest_point_host import GOLDEN_SCENES, chain_tree, golden_scene, precompute
from test_radius_search_host import Tree

HARNESS = os.path.join(ROOT, "tests", "cpp", "ray_hits_body_host.cpp")
GUARD = 8                                                      # sentinel records on either side of a record buffer
SENT_BYTE = 0xA5


def compile_harness(out_dir):
    out = os.path.join(str(out_dir), "libray_hits_body_host.so")
    cmd = ["g++", "-std=c++20", "-O1", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-strict-aliasing", "-Wall", "-Wextra", "-Wno-unused-parameter",
           "-Wno-unknown-pragmas", "-Werror", "-shared", "-fPIC", "-pthread", HARNESS, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    dll = C.CDLL(out)
    P, Z, I, U = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32
    dll.ray_hits_host_walk.restype = I
    dll.ray_hits_host_walk.argtypes = [I, I, I, I, P, U, P, P, Z, P, P, U, I, P, P, P, P]
    dll.ray_hits_host_walk_slice.restype = C.c_longlong
    dll.ray_hits_host_walk_slice.argtypes = [I, I, I, P, U, P, P, Z, Z, Z, P, P, U, P, P, P, P]
    return dll


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def hit_dtype(tree):
    return oracle.HITD if tree.double else oracle.HITF


def _aligned_bytes(nbytes, align=32):
    raw = np.empty(nbytes + align, dtype=np.uint8)
    off = (-raw.ctypes.data) % align
    return raw[off:off + nbytes]


def host_walk(dll, tree, rays, robust=False, offsets=None, total=0, counts=True, order=None, prim_ids=None, deep_cap=0, threads=1, mutant=0):
    """One call of the kernel's walk. offsets None: the count pass. Otherwise the record buffer holds `total` records between two guard
    zones of GUARD records of SENT_BYTE bytes and is returned WITH the guards. -> (counts or None, records or None, counters)."""
    from test_kernel_body_host import _aligned
    r = _aligned(np.ascontiguousarray(rays, dtype=tree.dtype))
    n = len(r)
    cnt = np.zeros(3, dtype=np.uint64)
    c = np.full(n, 0xABABABAB, dtype=np.uint32) if counts else None
    off = rec = rec_arg = None
    if offsets is not None:
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        ht = hit_dtype(tree)
        rec = _aligned_bytes((total + 2 * GUARD) * ht.itemsize)
        rec[:] = SENT_BYTE
        rec = rec.view(ht)
        rec_arg = rec[GUARD:].ctypes.data_as(C.c_void_p)
    order = None if order is None else np.ascontiguousarray(order, dtype=np.uint32)
    prim_ids = None if prim_ids is None else np.ascontiguousarray(prim_ids, dtype=np.uint32)
    assert dll.ray_hits_host_walk(int(tree.double), tree.leaf, int(robust), mutant, _p(tree.pairs), tree.root, _p(tree.prims), _p(r), n, _p(order),
                                  _p(prim_ids), deep_cap, threads, _p(c), _p(off), rec_arg, _p(cnt)) == 0
    return c, rec, cnt


def guards_intact(rec, total):
    b = rec.view(np.uint8).reshape(len(rec), -1)
    return bool((b[:GUARD] == SENT_BYTE).all() and (b[GUARD + total:] == SENT_BYTE).all())


def untouched(rec):
    """Which records of a buffer still hold the sentinel bytes."""
    return (rec.view(np.uint8).reshape(len(rec), -1) == SENT_BYTE).all(axis=1)


def host_ray_hits(dll, tree, rays, **kw):
    """Count, offsets, fill: (offsets (n + 1) uint64, records, counts, counters of the fill pass). Checks what every such call must
    satisfy: the fill pass reports the counts of the count pass, exact offsets leave no padding, the guard zones stay untouched."""
    counts, _, cnt0 = host_walk(dll, tree, rays, **kw)
    offsets = np.concatenate([[0], np.cumsum(counts.astype(np.uint64))]).astype(np.uint64)
    total = int(offsets[-1])
    c2, rec, cnt = host_walk(dll, tree, rays, offsets=offsets, total=total, **kw)
    assert (c2 == counts).all() and (cnt == cnt0).all()
    assert guards_intact(rec, total)
    out = rec[GUARD:GUARD + total]
    assert not untouched(out).any()
    return offsets, out, counts, cnt


def miss_record(tree, tmax):
    m = np.zeros(1, dtype=hit_dtype(tree))
    m["prim"], m["t"] = INVALID, tmax
    return m


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return compile_harness(tmp_path_factory.mktemp("ray_hits"))


@pytest.fixture(scope="module")
def lib():
    return reference_lib()


# ---- the scenes: (tree, rays, reference hit / rec per robust) computed once and shared, never changed ---------------------------------

_CACHE = {}


def seeded_case(lib, kind, n_prims, n_rays=256):
    """kind 'tri' (float) or 'sphere' (double): a dense scene in the unit cube, half of the rays aimed at points on primitives."""
    key = (kind, n_prims, n_rays)
    if key not in _CACHE:
        sphere = kind == "sphere"
        raw = dense_spheres(n_prims, 100 + n_prims) if sphere else dense_tris(n_prims, 200 + n_prims)
        nodes, ids, prims = build_tree(lib, raw, sphere)
        dt = prims.dtype
        rays = np.concatenate([rays_through([0, 0, 0], [1, 1, 1], n_rays // 2, 3, dt),
                               rays_through([0, 0, 0], [1, 1, 1], n_rays - n_rays // 2, 4, dt, targets=points_on(raw, n_rays - n_rays // 2, 5))])
        tree = Tree(nodes["bounds"], nodes["index"], prims, int(sphere))
        ref = {rb: reference_records(lib, nodes, prims, rays, int(sphere), rb) for rb in (False, True)}
        _CACHE[key] = (tree, rays, ref, ids, nodes)
    return _CACHE[key]


def golden_case(lib, orc, scene, n_rays=256):
    key = ("golden", scene, n_rays)
    if key not in _CACHE:
        from bvh_amd import synth
        bounds, index, prims, leaf, raw, ids = golden_scene(scene, "parallel_high", orc)
        lo, hi = synth.scene_bounds(raw)
        dt = prims.dtype
        rays = np.concatenate([rays_through(lo, hi, n_rays // 2, 7, dt), rays_through(lo, hi, n_rays - n_rays // 2, 8, dt, targets=points_on(raw, n_rays - n_rays // 2, 9))])
        tree = Tree(bounds, index, prims, leaf)
        nodes = np.zeros(len(index), dtype=oracle.NODED if tree.double else oracle.NODEF)
        nodes["bounds"], nodes["index"] = bounds, index
        ref = {rb: reference_records(lib, nodes, np.ascontiguousarray(prims), rays, leaf, rb) for rb in (False, True)}
        _CACHE[key] = (tree, rays, ref, ids, nodes)
    return _CACHE[key]


def check_against_reference(dll, tree, rays, ref, robust, mutant=0, **kw):
    """The walk's lists against the reference set: per ray the same primitives (as sets), the same records byte for byte, and — the
    order being the tree's — the same bytes back to back. Returns the reference's counts."""
    hit, rec = ref[robust]
    want_counts, want = expected_lists(hit, rec, tree.index)
    if mutant:
        counts, _, _ = host_walk(dll, tree, rays, robust=robust, mutant=mutant)
        offsets = np.concatenate([[0], np.cumsum(counts.astype(np.uint64))]).astype(np.uint64)
        _, buf, _ = host_walk(dll, tree, rays, robust=robust, mutant=mutant, offsets=offsets, total=int(offsets[-1]))
        got = buf[GUARD:GUARD + int(offsets[-1])]
    else:
        offsets, got, counts, _ = host_ray_hits(dll, tree, rays, robust=robust, **kw)
    w_off = np.concatenate([[0], np.cumsum(want_counts.astype(np.int64))])
    for r in range(len(rays)):
        g, w = got[int(offsets[r]):int(offsets[r + 1])], want[w_off[r]:w_off[r + 1]]
        assert set(g["prim"].tolist()) == set(w["prim"].tolist()), (r, g["prim"], w["prim"])
        assert np.sort(g, order=["prim"]).tobytes() == np.sort(w, order=["prim"]).tobytes(), r
    assert (counts == want_counts).all()
    assert got.tobytes() == want.tobytes()
    return want_counts


@pytest.mark.parametrize("robust", [False, True])
@pytest.mark.parametrize("n_prims", [1, 2, 3, 200])
@pytest.mark.parametrize("kind", ["tri", "sphere"])
def test_walk_equals_reference_seeded(dll, lib, kind, n_prims, robust):
    tree, rays, ref, _, _ = seeded_case(lib, kind, n_prims)
    counts = check_against_reference(dll, tree, rays, ref, robust, threads=4)
    print(f"{kind} x {n_prims} robust={robust}: mean list {counts.mean():.2f}, max {counts.max()}, >= 3 on {(counts >= 3).mean():.2f} of the rays")
    assert counts.sum() > 0
    if n_prims == 200:                                         # dense enough to test anything (on the reference's own counts)
        assert (counts >= 3).mean() >= 0.25 and counts.max() >= 8


def holds_closest(seg, closest, sphere):
    """The list `seg` of a ray holds the record closest-hit intersect keeps for it (`closest`, one record): byte for byte for a
    triangle. A sphere's record is {prim, t0, t1 = min(exit, tmax)}, and closest-hit clips t1 to the tmax it has shortened so far while
    the list never shortens: there prim and t0 are the same bits and the list's t1 is the unclipped one, so not below closest-hit's."""
    if not sphere:
        return closest.tobytes() in [seg[k:k + 1].tobytes() for k in range(len(seg))]
    same = seg[(seg["prim"] == closest["prim"]) & (seg["t"] == closest["t"]) & (np.signbit(seg["t"]) == np.signbit(closest["t"]))]
    return len(same) == 1 and closest["u"] <= same["u"][0] and closest["v"] == 0 and same["v"][0] == 0


@pytest.mark.parametrize("robust", [False, True])
@pytest.mark.parametrize("scene", GOLDEN_SCENES)
def test_walk_equals_reference_golden(dll, lib, orc, scene, robust):
    tree, rays, ref, ids, nodes = golden_case(lib, orc, scene)
    assert len(rays) <= 256
    counts = check_against_reference(dll, tree, rays, ref, robust, threads=4)
    print(f"{scene} robust={robust}: mean list {counts.mean():.2f}, max {counts.max()}, >= 3 on {(counts >= 3).mean():.2f} of the rays")
    assert counts.sum() > 0 and counts.max() >= 2
    # the nearest record of the list is what the reference's unmasked closest-hit keeps, byte for byte; no hit there, no list here
    bvh = lib.from_arrays(nodes, np.arange(len(tree.prims), dtype=np.uint64))
    closest = (bvh.intersect_sphere if tree.leaf else bvh.intersect_tri)(tree.prims, rays, any_hit=False, robust=robust)
    if "pad" in closest.dtype.names:
        closest["pad"] = 0
    offsets, got, _, _ = host_ray_hits(dll, tree, rays, robust=robust)
    for r in range(len(rays)):
        seg = got[int(offsets[r]):int(offsets[r + 1])]
        if closest["prim"][r] == INVALID:
            assert len(seg) == 0, r
        else:
            assert holds_closest(seg, closest[r], tree.leaf), r
    # original ids: the same walk, the records' prim mapped through prim_ids
    oo, og, oc, _ = host_ray_hits(dll, tree, rays, robust=robust, prim_ids=ids.astype(np.uint32))
    mapped = got.copy()
    mapped["prim"] = ids[got["prim"].astype(np.int64)].astype(np.uint32)
    assert (oo == offsets).all() and og.tobytes() == mapped.tobytes()
    # reading the batch through a permuted order changes nothing
    perm = np.random.default_rng(5).permutation(len(rays)).astype(np.uint32)
    po, pg, pc, _ = host_ray_hits(dll, tree, rays, robust=robust, order=perm)
    assert (po == offsets).all() and pg.tobytes() == got.tobytes()


@pytest.mark.parametrize("mutant", [1, 2])
def test_the_checks_bite(dll, lib, mutant):
    """A walk that shortens tmax after a hit (1) and one that visits the nearer child first (2) must each fail the comparison the
    body passes on the dense seeded scene."""
    tree, rays, ref, _, _ = seeded_case(lib, "tri", 200)
    check_against_reference(dll, tree, rays, ref, False)                       # the body passes ...
    with pytest.raises(AssertionError):
        check_against_reference(dll, tree, rays, ref, False, mutant=mutant)    # ... the wrong walk does not
    # and each fails for its own reason: shortening loses hits, near-first keeps the set and breaks the order
    hit, rec = ref[False]
    want_counts, want = expected_lists(hit, rec, tree.index)
    counts, _, _ = host_walk(dll, tree, rays, mutant=mutant)
    if mutant == 1:
        assert (counts <= want_counts).all() and (counts < want_counts).any()
    else:
        assert (counts == want_counts).all()
        offsets = np.concatenate([[0], np.cumsum(counts.astype(np.uint64))]).astype(np.uint64)
        _, buf, _ = host_walk(dll, tree, rays, mutant=mutant, offsets=offsets, total=len(want))
        got = buf[GUARD:GUARD + len(want)]
        assert got.tobytes() != want.tobytes() and sorted(got["prim"].tolist()) == sorted(want["prim"].tolist())


def _hand_tree():
    """Five triangles at x = 0..4 facing the x axis (BVH order = position), and this tree over them:
           root
          /    \\
        A        leaf {3, 4}          (the right child holds the far end ...)
       /  \\
    leaf{2} B                         (... and A's left child a middle one)
           / \\
      leaf{0} leaf{1}
    Walk order: 2, 0, 1, 3, 4."""
    tris = np.zeros((5, 9), dtype=np.float32)
    for k in range(5):
        tris[k] = [k, -1, -1, k, 1, -1, k, 0, 1]
    prims = precompute(tris, np.float32)
    box = lambda a, b: [a, b, -1, 1, -1, 1]
    nodes = np.zeros(7, dtype=oracle.NODEF)
    nodes["bounds"] = [box(0, 4), box(0, 2), box(3, 4), box(2, 2), box(0, 1), box(0, 0), box(1, 1)]
    nodes["index"] = [1 << 4, 3 << 4, (3 << 4) | 2, (2 << 4) | 1, 5 << 4, (0 << 4) | 1, (1 << 4) | 1]
    return nodes, prims


def test_walk_order_written_out(dll, lib):
    nodes, prims = _hand_tree()
    tree = Tree(nodes["bounds"], nodes["index"], prims, 0)
    assert dfs_prim_order(nodes["index"]).tolist() == [2, 0, 1, 3, 4]
    rays = np.array([[-1, 0, 0, 1, 0, 0, 0, 100],              # +x through all five: t = 1, 2, 3, 4, 5 at prims 0..4
                     [5, 0, 0, -1, 0, 0, 0, 100],              # -x through all five: the same list (the order is the tree's)
                     [-1, 0, 0, 1, 0, 0, 2.5, 4.5],            # [tmin, tmax] keeps prims 2 and 3 (t = 3, 4)
                     [-1, 0, 0, 1, 0, 0, 2, 2],                # tmin == tmax on a triangle: that one
                     [-1, 5, 0, 1, 0, 0, 0, 100]], dtype=np.float32)   # beside the stack: nothing
    for robust in (False, True):
        offsets, got, counts, cnt = host_ray_hits(dll, tree, rays, robust=robust)
        seg = lambda r: got[int(offsets[r]):int(offsets[r + 1])]
        assert counts.tolist() == [5, 5, 2, 1, 0]
        assert seg(0)["prim"].tolist() == [2, 0, 1, 3, 4] and seg(0)["t"].tolist() == [3, 1, 2, 4, 5]
        assert seg(1)["prim"].tolist() == [2, 0, 1, 3, 4] and seg(1)["t"].tolist() == [3, 5, 4, 2, 1]
        assert seg(2)["prim"].tolist() == [2, 3] and seg(2)["t"].tolist() == [3, 4]
        assert seg(3)["prim"].tolist() == [1] and seg(3)["t"].tolist() == [2]
        assert (seg(0)["u"] == 0.25).all() and (seg(0)["v"] == 0.5).all()      # (0, 0) in the triangle {(-1, -1), (1, -1), (0, 1)}
        hit, rec = reference_records(lib, nodes, prims, rays, 0, robust)
        want_counts, want = expected_lists(hit, rec, nodes["index"])
        assert (want_counts == counts).all() and want.tobytes() == got.tobytes()


def test_output_shapes(dll, lib):
    tree, rays, ref, _, _ = seeded_case(lib, "tri", 200)
    n = len(rays)
    offsets, recs, counts, _ = host_ray_hits(dll, tree, rays)       # count pass == list lengths, no padding, guards: checked inside
    assert counts.max() > 4 and (counts > 0).any()
    # without counts: same lists
    _, buf, _ = host_walk(dll, tree, rays, offsets=offsets, total=len(recs), counts=False)
    assert buf[GUARD:GUARD + len(recs)].tobytes() == recs.tobytes() and guards_intact(buf, len(recs))
    # k = 4 slots per ray, the buffer starting at a non-zero offset: prefix in walk order, padding, untruncated counts, guards
    k, base = 4, 3
    assert (counts > k).any() and (counts < k).any()
    fixed = (base + k * np.arange(n + 1)).astype(np.uint64)
    total = base + k * n + 5                                   # records before offsets[0] and after offsets[n] belong to nobody
    c4, buf, _ = host_walk(dll, tree, rays, offsets=fixed, total=total)
    assert (c4 == counts).all() and guards_intact(buf, total)
    assert untouched(buf[GUARD:GUARD + base]).all() and untouched(buf[GUARD + base + k * n:]).all()
    seg = buf[GUARD + base:GUARD + base + k * n].reshape(n, k)
    for i in range(n):
        m = min(int(counts[i]), k)
        assert seg[i, :m].tobytes() == recs[int(offsets[i]):int(offsets[i]) + m].tobytes()
        assert seg[i, m:].tobytes() == np.repeat(miss_record(tree, rays[i, 7]), k - m).tobytes()
    # stale offsets: a segment that ends before it begins is empty, the others (here all [0, 9)) are kept to; counts are still reported
    stale = np.zeros(n + 1, dtype=np.uint64)
    stale[::2] = 9
    c5, buf, _ = host_walk(dll, tree, rays, offsets=stale, total=16)
    assert (c5 == counts).all()
    assert untouched(buf[GUARD + 9:]).all() and guards_intact(buf, 16)
    # double spheres: the same protocol on 32-byte records
    tree, rays, ref, _, _ = seeded_case(lib, "sphere", 200)
    offsets, recs, counts, _ = host_ray_hits(dll, tree, rays, robust=True)
    fixed = (k * np.arange(len(rays) + 1)).astype(np.uint64)
    c4, buf, _ = host_walk(dll, tree, rays, robust=True, offsets=fixed, total=k * len(rays))
    assert (c4 == counts).all() and guards_intact(buf, k * len(rays))
    seg = buf[GUARD:GUARD + k * len(rays)].reshape(len(rays), k)
    for i in range(len(rays)):
        m = min(int(counts[i]), k)
        assert seg[i, :m].tobytes() == recs[int(offsets[i]):int(offsets[i]) + m].tobytes()
        assert seg[i, m:].tobytes() == np.repeat(miss_record(tree, rays[i, 7]), k - m).tobytes()
        assert (seg[i, :m]["v"] == 0).all() and (seg[i, :m]["t"] <= seg[i, :m]["u"]).all()      # {prim, t0, t1, 0}


def test_edge_rays(dll, lib):
    """NaN tmin / tmax: count 0 and a fully padded segment carrying the ray's own tmax bits. tmin > tmax, a zero direction, NaN
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
                     [-1, 0, 0, 1, 0, 0, 0, 100]], dtype=np.float32)
    tmax_bits = rays[:, 7].copy()
    tmax_bits.view(np.uint32)[1] = 0x7FC12345                  # a NaN with a payload: the padding carries these very bits
    rays[:, 7] = tmax_bits
    for robust in (False, True):
        hit, rec = reference_records(lib, nodes, prims, rays, 0, robust)
        want_counts, want = expected_lists(hit, rec, nodes["index"])
        offsets, got, counts, _ = host_ray_hits(dll, tree, rays, robust=robust)
        assert (counts == want_counts).all() and got.tobytes() == want.tobytes()
        assert counts[:3].tolist() == [0, 0, 0] and counts[3] == 0 and counts[8] == 5 and counts[9] == 5
        fixed = (2 * np.arange(len(rays) + 1)).astype(np.uint64)
        _, buf, _ = host_walk(dll, tree, rays, robust=robust, offsets=fixed, total=2 * len(rays))
        seg = buf[GUARD:-GUARD].reshape(-1, 2)
        for r in (0, 1, 2, 3):
            pad = miss_record(tree, 0)
            pad["t"].view(np.uint32)[0] = rays[r, 7:8].view(np.uint32)[0]
            assert seg[r].tobytes() == np.repeat(pad, 2).tobytes(), r
    # a root that is a leaf is tested without a box test: one triangle, a ray that its (empty) box test could never pass
    tree1, rays1, _, _, _ = seeded_case(lib, "tri", 1)
    assert (tree1.root & 15) == 1
    c, _, cnt = host_walk(dll, tree1, rays1)
    assert c.sum() > 0 and cnt[0] == 0 and cnt[2] == len(rays1)


def chain_rays(depth, n, base=4000, every=4):
    """Rays along +x from in front of the chain (triangles at x = base - k, |y|, |z| <= 1): every 4th (`every`) crosses every level, the
    others end inside the far end of the stack."""
    rng = np.random.default_rng(depth)
    r = np.zeros((n, 8), dtype=np.float32)
    r[:, 0] = base - depth - 2 - rng.random(n)
    r[:, 1] = (rng.random(n) - 0.5) * 0.5
    r[:, 2] = -0.5 + 0.5 * rng.random(n)
    r[:, 3] = 1
    r[:, 7] = 3 + np.floor(10 * rng.random(n))
    r[::every, 7] = 1e6
    return r


def chain(depth, prep_tris, stacked):
    """chain_tree as a Tree over its triangles; stacked: every inner child on the left, so that the left-first walk of a ray that crosses
    every level stacks one leaf per level."""
    tris, nodes, _ = chain_tree(depth, prep_tris)
    if stacked:
        nodes[1::2], nodes[2::2] = nodes[2::2].copy(), nodes[1::2].copy()
    return Tree(nodes["bounds"], nodes["index"], precompute(tris, np.float32), 0), nodes


@pytest.mark.parametrize("depth", [70, 300])
@pytest.mark.parametrize("stacked", [False, True])
def test_deep_chain(dll, orc, restatement, depth, stacked):
    """Stacked, 70 levels cross LDS -> scratch (entry 16), scratch -> HBM (entry 64) and end on the last of the 6 HBM entries given;
    300 levels fill 236. Expected: every triangle in front of tmax, in the tree's order (the restatement's growing stack gives the
    closest-hit record of the deepest one as a cross-check)."""
    tree, nodes = chain(depth, orc.prep_tris, stacked)
    dfs = dfs_prim_order(nodes["index"])
    assert (dfs == (np.arange(depth, -1, -1) if stacked else np.arange(depth + 1))).all()
    rays = chain_rays(depth, 48)
    offsets, got, counts, _ = host_ray_hits(dll, tree, rays, deep_cap=depth - 64 if stacked else depth - 64 + 1)
    assert (counts[::4] == depth + 1).all() and 0 < counts[1::4].min() and counts[1::4].max() < 16
    for r in range(len(rays)):
        seg = got[int(offsets[r]):int(offsets[r + 1])]
        t_of = np.float32(4000) - np.arange(depth + 1, dtype=np.float32) - rays[r, 0]       # exact in float: small integers and one subtraction
        want = [k for k in dfs if t_of[k] <= rays[r, 7]]
        assert seg["prim"].tolist() == want, r
        assert (seg["t"] == t_of[seg["prim"].astype(np.int64)]).all()
    closest = restatement.from_arrays(nodes, np.arange(depth + 1, dtype=np.uint64)).intersect_tri(tree.prims, rays, robust=False)
    for r in range(len(rays)):
        assert holds_closest(got[int(offsets[r]):int(offsets[r + 1])], closest[r], 0)


def test_ray_hits_symbols_are_declared_and_exported():
    from bvh_amd import _lib, build
    build.build()
    dll = _lib.load()
    header = open(os.path.join(ROOT, "include", "bvh_amd.h")).read()
    declared = set(re.findall(r"BVH_AMD_API[^;]*?\b(bvh\w+)\s*\(", header))
    want = {f"bvh{s}_intersect_rays_all_{leaf}" for s in ("3f", "3d") for leaf in ("tri", "sphere")}
    assert {n for n in declared if "rays_all" in n} == want
    assert want <= set(_lib.exported_symbols())
    for name in sorted(want):
        assert hasattr(dll, name), name
    for s in ("2f", "2d"):
        for leaf in ("tri", "sphere"):
            assert not hasattr(dll, f"bvh{s}_intersect_rays_all_{leaf}")
            assert f"bvh{s}_intersect_rays_all_{leaf}" not in _lib.exported_symbols()


def test_sliced_launch_emulation(dll, orc):
    """One batch cut into launches of 256 lanes over the 70-level stacked chain, as point_query_run cuts it: slot = first + lane, the
    spill indexed by the lane and sized for the launch. The same bytes as the unsliced walk, the spill's guard zones untouched."""
    depth = 70
    tree, _ = chain(depth, orc.prep_tris, True)
    rays = chain_rays(depth, 300)
    cap = depth - 64
    offsets, want, counts, _ = host_ray_hits(dll, tree, rays, deep_cap=cap)
    from test_kernel_body_host import _aligned
    r = _aligned(np.ascontiguousarray(rays))
    got_counts = np.zeros(len(rays), dtype=np.uint32)
    buf = np.zeros(len(want) + 1, dtype=oracle.HITF)
    cnt = np.zeros(3, dtype=np.uint64)
    for first in range(0, len(rays), 256):
        n = min(256, len(rays) - first)
        touched = dll.ray_hits_host_walk_slice(0, 0, 0, _p(tree.pairs), tree.root, _p(tree.prims), _p(r), first, n, 256, None, None, cap, _p(got_counts),
                                               _p(offsets), _p(buf), _p(cnt))
        assert touched > 0                                     # (every 4th ray stacks on every level: the spill is used, inside its guards)
    assert (got_counts == counts).all() and buf[:len(want)].tobytes() == want.tobytes()
    assert dll.ray_hits_host_walk_slice(0, 0, 0, _p(tree.pairs), tree.root, _p(tree.prims), _p(r), 0, 300, 256, None, None, cap, _p(got_counts), _p(offsets),
                                        _p(buf), _p(cnt)) == -2
