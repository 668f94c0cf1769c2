"""CPU: the TEXT of the convex-region kernel (bvh_amd/csrc/region_body.inc + list_walk.inc + point_walk.inc + trace_device.h) compiled for the
host by tests/cpp/region_body_host.cpp. The EXACT predicate against exact clipping in rational arithmetic on an integer lattice, and
against its float64 restatement on random floats; the walk over the golden trees against a numpy brute force of the stated plane
expression in the scene's scalar type (EXACT equality, nothing excluded, in the tree's depth-first order); spheres; the inside flags;
the shapes of the output (count pass, exact offsets, fixed segments, padding, guard zones); edge regions and edge triangles; trees
deeper than 64 levels; the exported symbols. The device's counts, lists, flags and counters must equal this harness's byte for byte
(tests/test_gpu_region.py)."""
import os
import re

import numpy as np
import pytest

import region_ref as R
from conftest import ROOT
from region_ref import GUARD, INVALID, SENT_PRIM, guards_intact
from test_closest_point_host import GOLDEN_SCENES

# The smallest delta for which R-(delta) <= host EXACT <= R+(delta) on the 4000 cull-passing pairs of test_exact_sandwich, measured:
# 0 in float and 0 in double (the host's EXACT equals the float64 restatement on every pair). Asserted: 4 x that.
SANDWICH_DELTA = {np.float32: 4 * 0.0, np.float64: 4 * 0.0}
# The walk never drops a sphere whose float64 margin r * len - s exceeds this many u * M ("Convex-region queries").
SPHERE_MARGIN_ULPS = 16


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return R.compile_harness(tmp_path_factory.mktemp("region"))


def lattice_cases(n, seed):
    """n (triangle (3, 3), planes (m, 4)) of small integers, m = 1 .. 8 in turn; zero normals and triangles without area included."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        m = 1 + k % 8
        out.append((rng.integers(-4, 5, size=(3, 3)), np.concatenate([rng.integers(-3, 4, size=(m, 3)), rng.integers(-6, 7, size=(m, 1))], axis=1)))
    return out


def test_lattice_exact_equals_rational_clipping(dll):
    """Every determinant of the predicate is an integer below 2^24 here, so EXACT must be THE answer: Sutherland-Hodgman in Fractions.
    So must the float64 restatement (region_ref.exact64) that test_exact_sandwich measures the kernel against."""
    cases = lattice_cases(3200, 7)
    want = np.array([R.clip_exact(t, p) for t, p in cases])
    assert 800 < want.sum() < 2400
    for dt in (np.float32, np.float64):
        cull, exact = np.zeros(len(cases), dtype=bool), np.zeros(len(cases), dtype=bool)
        for m in range(1, 9):
            idx = np.arange(m - 1, len(cases), 8)
            tris = np.array([cases[k][0].reshape(9) for k in idx], dtype=dt)
            planes = np.array([cases[k][1] for k in idx], dtype=dt)
            c, e, inside = R.host_pairs(dll, tris, planes, dt)
            cull[idx], exact[idx] = c, e
            # CULL and the inside flag against their definitions, in integers
            val = np.einsum("kpc,kvc->kpv", planes[:, :, :3].astype(np.int64), tris.reshape(-1, 3, 3).astype(np.int64)) + planes[:, :, 3:].astype(np.int64)
            assert (c == (val <= 0).any(axis=2).all(axis=1)).all()
            assert (inside == (val <= 0).all(axis=(1, 2))).all()
            # the float64 restatement of the predicate, the reference of test_exact_sandwich, on the integer plane values D[k, p, i]:
            # it, too, must be THE answer here (its determinants are integers below 2^53)
            assert (R.exact64(val) == want[idx]).all()
        print(f"{np.dtype(dt).name}: {len(cases)} cases, {int(want.sum())} intersect, CULL lists {int(cull.sum())}, CULL minus EXACT {int((cull & ~exact).sum())}")
        assert (exact == want).all()
        assert not (exact & ~cull).any() and (cull & ~exact).sum() > 100          # the plane-by-plane test accepts disjoint triangles


def region_brute(tree, planes, exact, dll):
    """(match, inside) matrices [q, BVH-order i]: the numpy brute force of CULL / the sphere test; EXACT: the kernel's predicate on
    the pairs CULL lets through."""
    pr = tree.ordered()
    match, inside = R.brute_cull(pr, planes)
    if exact:
        q, i = np.nonzero(match)
        c, e, _ = R.host_pairs(dll, pr[i], planes[q], tree.dtype)
        assert c.all()
        match = match.copy()
        match[q, i] = e
    return match, inside & match


@pytest.mark.parametrize("scene", GOLDEN_SCENES)
@pytest.mark.parametrize("mode", R.TREES)
def test_walk_equals_brute_force(dll, scene, mode):
    tree = R.golden_tree(scene, mode)
    assert len(tree.dfs) == tree.n and len(set(tree.dfs.tolist())) == tree.n
    listed = 0
    for m in (1, 2, 6, 8):
        planes = R.make_regions(tree.prims, 192, m, tree.dtype, 100 + m)
        match, inside = region_brute(tree, planes, False, dll)
        offsets, ids, ins, counts, cnt = R.host_region(dll, tree, planes, threads=4)
        want_counts, want_ids = R.expected_lists(match, tree.dfs)
        in_brute_only = 0
        if tree.leaf == 1:
            # spheres: the walk's set is a subset of the brute force; what is missing is within rounding of tangent from outside
            walk = np.zeros_like(match)
            walk[np.repeat(np.arange(len(planes)), counts), ids.astype(np.int64)] = True
            assert not (walk & ~match).any()
            q, i = np.nonzero(match & ~walk)
            in_brute_only = len(q)
            if in_brute_only:
                pr, p64 = tree.ordered().astype(np.float64)[i], planes.astype(np.float64)[q]
                s = np.einsum("kpc,kc->kp", p64[:, :, :3], pr[:, :3]) + p64[:, :, 3]
                ln = np.linalg.norm(p64[:, :, :3], axis=2)
                big = (np.abs(p64[:, :, :3]) * (np.abs(pr[:, None, :3]) + pr[:, None, 3:4])).sum(axis=2) + np.abs(p64[:, :, 3])
                margin = pr[:, 3:4] * ln - s
                real = ln > 0                                   # (a padding plane has margin 0 = 16 u M: it drops nothing)
                assert ((margin <= SPHERE_MARGIN_ULPS * np.finfo(tree.dtype).eps / 2 * big) & real).any(axis=1).all()
                match = walk
                want_counts, want_ids = R.expected_lists(match, tree.dfs)
        print(f"{scene} {mode} m={m}: {len(want_ids)} listed (mean {len(want_ids) / len(planes):.1f}), {int(ins.sum())} wholly inside, "
              f"{in_brute_only} in the brute force only")
        assert (counts == want_counts).all() and ids.tobytes() == want_ids.tobytes()
        assert ins.tobytes() == R.expected_inside(match, inside, tree.dfs).tobytes()
        assert cnt[0] > 0 and cnt[1] > 0 and cnt[2] > 0
        listed += len(want_ids)
        kinds = 6 if m >= 6 else 4 if m >= 2 else 3
        empty, everything = np.arange(len(planes)) % kinds == kinds - 2, np.arange(len(planes)) % kinds == kinds - 1
        assert (counts[empty] == 0).all() and (counts[everything] == tree.n).all()
        assert (ins[np.repeat(everything, counts)] == 1).all()                  # a subtree wholly inside: all ones
        if m == 6:
            oo, oi, _, oc, _ = R.host_region(dll, tree, planes, original_ids=True)
            assert (oo == offsets).all() and (oi == tree.ids[ids.astype(np.int64)]).all() and (oc == counts).all()
            if tree.leaf == 0:                                  # EXACT: a subset of CULL, the kernel's predicate on every CULL pair
                em, ei = region_brute(tree, planes, True, dll)
                eo, eids, eins, ec, _ = R.host_region(dll, tree, planes, exact=True, threads=4)
                wc, wi = R.expected_lists(em, tree.dfs)
                assert (ec == wc).all() and eids.tobytes() == wi.tobytes() and eins.tobytes() == R.expected_inside(em, ei, tree.dfs).tobytes()
                assert (ec <= counts).all() and (scene == "cornell" or (ec < counts).any())
    assert listed > 0


def sandwich_pairs(dll, dt, want=4000, seed=11):
    """Cull-passing pairs of unit scale: triangles c + 0.06 normal(3, 3), c uniform in the unit cube, against oriented boxes of
    half-extent 0.05 .. 0.30 centred in the cube, unit normals."""
    rng = np.random.default_rng(seed)
    tris, planes, have = [], [], 0
    while have < want:
        k = 16000
        t = (rng.random((k, 1, 3)) + 0.06 * rng.normal(size=(k, 3, 3))).reshape(k, 9).astype(dt)
        pl = np.array([R.box_planes(rng.random(3), R.rotation(rng), 0.05 + 0.25 * rng.random(3)) for _ in range(k)]).astype(dt)
        c, _, _ = R.host_pairs(dll, t, pl, dt)
        tris.append(t[c]), planes.append(pl[c])
        have += int(c.sum())
    return np.concatenate(tris)[:want], np.concatenate(planes)[:want]


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_exact_sandwich(dll, dt):
    """R-(delta) <= EXACT <= R+(delta): the float64 restatement of the predicate (checked against clipping above) with every plane
    value moved by +delta / -delta."""
    t, pl = sandwich_pairs(dll, dt)
    c, e, _ = R.host_pairs(dll, t, pl, dt)
    assert c.all() and len(t) == 4000
    t64, p64 = t.astype(np.float64), pl.astype(np.float64)
    D = np.stack([np.einsum("kpc,kc->kp", p64[:, :, :3], t64[:, 3 * v:3 * v + 3]) + p64[:, :, 3] for v in range(3)], axis=2)
    delta = SANDWICH_DELTA[dt]
    r_minus, r_plus = R.exact64(D, delta), R.exact64(D, -delta)
    print(f"{np.dtype(dt).name}: {len(t)} cull-passing pairs, EXACT lists {int(e.sum())}, differs from the float64 restatement on "
          f"{int((e != R.exact64(D)).sum())}, R+ minus R- at delta = {delta}: {int((r_plus & ~r_minus).sum())}")
    assert (r_plus & ~r_minus).sum() <= 0.01 * len(t)
    assert not (r_minus & ~e).any() and not (e & ~r_plus).any()
    assert 0 < (c & ~e).sum() < e.sum()


def test_spheres_on_integers_are_exact(dll):
    """Integer centres and radii, normals of integer length: every product and the square root are exact, the walk is the brute force."""
    rng = np.random.default_rng(3)
    n = 300
    sph = np.concatenate([rng.integers(-20, 21, size=(n, 3)), rng.integers(0, 4, size=(n, 1))], axis=1).astype(np.float32)
    from tri_intersect_ref import tri_boxes  # noqa: F401
    import query_slices as qs
    boxes = np.concatenate([sph[:, :3] - sph[:, 3:], sph[:, :3] + sph[:, 3:]], axis=1)
    order = np.lexsort((sph[:, 2], sph[:, 1], sph[:, 0]))
    nodes = qs.chain_nodes(np.ascontiguousarray(boxes[order]))
    tree = R.PrimTree(nodes["bounds"], nodes["index"], sph, order.astype(np.uint32))
    normals = np.array([[1, 0, 0], [-1, 0, 0], [3, 4, 0], [0, -3, 4], [2, 3, 6], [-6, 2, -3], [0, 0, 0]], dtype=np.float32)
    planes = np.zeros((256, 3, 4), dtype=np.float32)
    planes[:, :, :3] = normals[rng.integers(len(normals), size=(256, 3))]
    planes[:, :, 3] = rng.integers(-60, 30, size=(256, 3))
    match, inside = R.brute_cull(tree.ordered(), planes)
    s = np.einsum("qpc,ic->qpi", planes[:, :, :3].astype(np.int64), tree.ordered()[:, :3].astype(np.int64)) + planes[:, :, 3:].astype(np.int64)
    rl = np.rint(np.linalg.norm(planes[:, :, :3], axis=2)).astype(np.int64)[:, :, None] * tree.ordered()[None, None, :, 3].astype(np.int64)
    assert (match == (s <= rl).all(axis=1)).all() and (inside == (s <= -rl).all(axis=1)).all()
    offsets, ids, ins, counts, _ = R.host_region(dll, tree, planes, deep_cap=n - 64)
    wc, wi = R.expected_lists(match, tree.dfs)
    assert (counts == wc).all() and ids.tobytes() == wi.tobytes() and ins.tobytes() == R.expected_inside(match, inside, tree.dfs).tobytes()
    assert 0 < ins.sum() < len(ins) and (counts == 0).any()
    touching = (s == rl).any(axis=1) & match                     # tangent from outside: listed
    assert touching.any()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_spheres_near_tangent_from_outside(dll, dt):
    """Spheres placed within a few roundings of tangent to a plane, on either side: the walk lists nothing the brute force does not,
    every sphere it drops has a float64 margin r * len - s of at most 16 u M for that plane, and every sphere with a larger margin that
    the sphere test accepts is listed."""
    import query_slices as qs
    rng = np.random.default_rng(23)
    n, nq = 600, 64
    u = np.finfo(dt).eps / 2
    normals = np.array([R.rotation(rng)[:, 0] * (0.3 + 3 * rng.random()) for _ in range(nq)])
    axis = np.arange(nq) % 2 == 0                                # every other normal along an axis: |n|_1 = |n|_2, the box has no slack
    normals[axis] = np.eye(3)[rng.integers(3, size=int(axis.sum()))] * rng.choice([-1.0, 1.0], size=(int(axis.sum()), 1)) * (0.3 + 3 * rng.random((int(axis.sum()), 1)))
    consts = rng.normal(size=nq)
    planes = np.zeros((nq, 2, 4))
    planes[:, 0, :3], planes[:, 0, 3] = normals, consts
    planes[:, 1] = [0, 0, 0, 0]                                   # a padding plane: it must not excuse anything
    planes = np.ascontiguousarray(planes.astype(dt))
    p64 = planes.astype(np.float64)
    ln = np.linalg.norm(p64[:, 0, :3], axis=1)
    # sphere j is tangent from outside to plane j % nq up to a signed offset of 0 .. 40 roundings of the terms
    j = np.arange(n) % nq
    r = 0.05 + rng.random(n)
    foot = rng.normal(size=(n, 3)) * 3
    foot -= ((foot * p64[j, 0, :3]).sum(axis=1) + p64[j, 0, 3])[:, None] * p64[j, 0, :3] / (ln[j] ** 2)[:, None]      # on the plane
    big = (np.abs(p64[j, 0, :3]) * (np.abs(foot) + 2 * r[:, None])).sum(axis=1) + np.abs(p64[j, 0, 3])
    off = rng.integers(-40, 41, size=n) * u * big / ln[j]
    c = foot + (r + off)[:, None] * p64[j, 0, :3] / ln[j][:, None]
    sph = np.ascontiguousarray(np.concatenate([c, r[:, None]], axis=1).astype(dt))
    boxes = np.concatenate([sph[:, :3] - sph[:, 3:], sph[:, :3] + sph[:, 3:]], axis=1)           # Sphere::get_bbox, rounded in dt
    order = np.lexsort((sph[:, 2], sph[:, 1], sph[:, 0]))
    nodes = qs.chain_nodes(np.ascontiguousarray(boxes[order]))
    tree = R.PrimTree(nodes["bounds"], nodes["index"], sph, order.astype(np.uint32))
    match, _ = R.brute_cull(tree.ordered(), planes)
    offsets, ids, ins, counts, _ = R.host_region(dll, tree, planes, deep_cap=n - 64)
    walk = np.zeros_like(match)
    walk[np.repeat(np.arange(nq), counts), ids.astype(np.int64)] = True
    assert not (walk & ~match).any()
    pr = tree.ordered().astype(np.float64)
    s = pr[None, :, :3] @ p64[:, 0, :3, None]
    s = s[:, :, 0] + p64[:, 0, 3:4]                               # [q, i]
    bigm = (np.abs(p64[:, None, 0, :3]) * (np.abs(pr[None, :, :3]) + pr[None, :, 3:4])).sum(axis=2) + np.abs(p64[:, 0, 3:4])
    margin = pr[None, :, 3] * ln[:, None] - s
    near = np.abs(margin) <= 64 * u * bigm
    dropped = match & ~walk
    print(f"{np.dtype(dt).name}: {int(near.sum())} pairs within 64 u M of tangent, {int((match & near).sum())} of them accepted by the sphere test, "
          f"{int(dropped.sum())} of those dropped by the node test, largest margin dropped {float((margin / (u * bigm))[dropped].max()) if dropped.any() else 0:.2f} u M")
    assert near.sum() >= n // 2 and (match & near).any() and (~match & near).any()
    assert (margin[dropped] <= SPHERE_MARGIN_ULPS * u * bigm[dropped]).all()
    assert walk[match & (margin > SPHERE_MARGIN_ULPS * u * bigm)].all()


def test_output_shapes(dll):
    tree = R.golden_tree("soup2k", "parallel_high")
    q = R.make_regions(tree.prims, 300, 6, np.float32, 5)
    n = len(q)
    offsets, ids, ins, counts, _ = R.host_region(dll, tree, q)      # count pass == list lengths, no padding, guards: checked inside
    assert counts.max() > 4 and (counts == 0).any() and (counts > 0).any()
    _, lp, li, _ = R.host_walk(dll, tree, q, offsets=offsets, total=len(ids), counts=False)      # without the optional counts and flags
    assert li is None and (lp[GUARD:GUARD + len(ids)] == ids).all() and guards_intact(lp, len(ids))
    # k = 4 slots per query, the buffer starting at a non-zero offset: prefix in walk order, padding, untruncated counts, guards
    k, base = 4, 7
    fixed = (base + k * np.arange(n + 1)).astype(np.uint64)
    total = base + k * n + 5                                   # entries before offsets[0] and after offsets[n] belong to nobody
    c4, lp, li, _ = R.host_walk(dll, tree, q, offsets=fixed, total=total, inside=True)
    assert (c4 == counts).all()
    assert (lp[GUARD:GUARD + base] == SENT_PRIM).all() and (lp[GUARD + base + k * n:] == SENT_PRIM).all() and guards_intact(lp, total)
    assert (li[GUARD:GUARD + base] == R.SENT_INSIDE).all() and (li[GUARD + base + k * n:] == R.SENT_INSIDE).all() and R.inside_guards_intact(li, total)
    seg = lp[GUARD + base:GUARD + base + k * n].reshape(n, k)
    flg = li[GUARD + base:GUARD + base + k * n].reshape(n, k)
    for i in range(n):
        m = min(int(counts[i]), k)
        assert (seg[i, :m] == ids[int(offsets[i]):int(offsets[i]) + m]).all() and (seg[i, m:] == INVALID).all()
        assert (flg[i, :m] == ins[int(offsets[i]):int(offsets[i]) + m]).all() and (flg[i, m:] == 0).all()
    assert (counts > k).any()                                   # truncation happened
    # stale offsets: a segment that ends before it begins is empty, the others (here all [0, 9)) are kept to; counts are still reported
    stale = np.zeros(n + 1, dtype=np.uint64)
    stale[::2] = 9
    c5, lp, li, _ = R.host_walk(dll, tree, q, offsets=stale, total=16, inside=True)
    assert (c5 == counts).all()
    assert not (lp[GUARD + 9:GUARD + 16] != SENT_PRIM).any() and guards_intact(lp, 16)
    assert not (li[GUARD + 9:GUARD + 16] != R.SENT_INSIDE).any() and R.inside_guards_intact(li, 16)


def test_edge_queries(dll):
    """One triangle in the plane z = 0 ({0,0,0}, {2,0,0}, {0,2,0}), one without area, one with a NaN vertex, one far away."""
    nan = np.nan
    tris = np.array([[0, 0, 0, 2, 0, 0, 0, 2, 0], [1, 1, 1, 1, 1, 1, 1, 1, 1], [5, 5, 5, nan, 5, 5, 5, 6, 5], [50, 50, 50, 51, 50, 50, 50, 51, 50]], dtype=np.float32)
    import query_slices as qs
    from tri_intersect_ref import tri_boxes
    bb = tri_boxes(tris)
    bb[2] = [5, 5, 5, 6, 6, 5]                                   # (the box of the finite vertices: min / max skip the NaN)
    nodes = qs.chain_nodes(bb)
    tree = R.PrimTree(nodes["bounds"], nodes["index"], tris, np.arange(4, dtype=np.uint32))
    P = lambda *planes: R.pad_planes(planes, 3)
    regions = np.array([
        P([0, 0, 1, 0]),                       # 0: z <= 0: the coplanar triangle matches (and is wholly inside)
        P([0, 0, 1, 1e-30]),                   # 1: z <= -tiny: it does not
        P([1, 0, 0, -0.0], [-0.0, 0, -1, -0.0]),   # 2: x <= 0 with -0 components: the edge {0,0,0}-{0,2,0} lies in the plane
        P([1, 1, 0, 0]),                       # 3: x + y <= 0: touches at the vertex {0,0,0} only
        P([1, 1, 0, 1e-30]),                   # 4: just not
        P([nan, 0, 0, 0]),                     # 5: NaN component: empty
        P([0, 0, 1, np.inf]),                  # 6: infinite component: empty
        P([0, 0, 1, 0], [0, -np.inf, 0, 0]),   # 7
        P([-1, 0, 0, 1], [1, 0, 0, -1]),       # 8: the slab x = 1 of no thickness: crosses triangle 0, contains the point triangle 1
        P([0, 1, 0, -5.5], [0, -1, 0, 5.5]),   # 9: the plane y = 5.5: between the finite vertices of the NaN triangle
        P([0, 0, 0, 1]),                       # 10: holds nowhere
        P([0, 0, 0, -0.0]),                    # 11: holds everywhere
    ], dtype=np.float32)
    for exact in (False, True):
        offsets, ids, ins, counts, _ = R.host_region(dll, tree, regions, exact=exact)
        seg = lambda k: ids[int(offsets[k]):int(offsets[k + 1])].tolist()
        flags = lambda k: ins[int(offsets[k]):int(offsets[k + 1])].tolist()
        assert seg(0) == [0] and flags(0) == [1] and seg(1) == []
        assert seg(2) == [0] and flags(2) == [0]
        assert seg(3) == [0] and flags(3) == [0] and seg(4) == []
        assert seg(5) == [] and seg(6) == [] and seg(7) == []
        assert seg(8) == [0, 1] and flags(8) == [0, 1]
        # a NaN vertex is inside no plane: CULL goes by the two finite vertices, EXACT never lists a triangle with a NaN plane value
        assert seg(9) == ([] if exact else [2]) and flags(9) == ([] if exact else [0])
        assert seg(10) == []
        assert seg(11) == ([0, 1, 3] if exact else [0, 1, 2, 3]) and flags(11) == ([1, 1, 1] if exact else [1, 1, 0, 1])
        # invalid queries with a segment: padded with INVALID and 0
        fixed = (2 * np.arange(len(regions) + 1)).astype(np.uint64)
        _, lp, li, _ = R.host_walk(dll, tree, regions, exact=exact, offsets=fixed, total=2 * len(regions), inside=True)
        assert (lp[GUARD:-GUARD].reshape(-1, 2)[[5, 6, 7, 10]] == INVALID).all() and (li[GUARD:-GUARD].reshape(-1, 2)[[5, 6, 7, 10]] == 0).all()


@pytest.mark.parametrize("depth", [70, 200])
@pytest.mark.parametrize("stacked", [False, True])
def test_deep_chain(dll, depth, stacked):
    """Stacked, the left-first walk of a region that keeps both children of every level alive stacks one leaf per level: 70 levels
    cross LDS -> scratch (entry 16) and scratch -> HBM (entry 64); 200 fill 136 HBM entries."""
    import query_slices as qs
    tree = R.chain_tree(depth, stacked)
    assert (tree.dfs == (np.arange(depth, -1, -1) if stacked else np.arange(depth + 1))).all()
    base = qs.chain_base(depth)
    rng = np.random.default_rng(depth)
    planes = np.zeros((48, 2, 4), dtype=np.float32)
    planes[:, 0] = [0, 0, 1, 0.5]                               # z <= -0.5: cuts every triangle of the chain, whatever its x
    planes[:, 1, 0] = 1
    planes[:, 1, 3] = -(base - depth + 10 * rng.random(48))     # x <= the far end + a little
    planes[::4, 1] = [0, 0, 0, 0]                               # every 4th: every level
    for exact in (False, True):
        offsets, ids, ins, counts, _ = R.host_region(dll, tree, planes, exact=exact, deep_cap=depth - 64 if stacked else depth - 64 + 1)
        match, inside = region_brute(tree, planes, exact, dll)
        wc, wi = R.expected_lists(match, tree.dfs)
        assert (counts == wc).all() and ids.tobytes() == wi.tobytes() and ins.tobytes() == R.expected_inside(match, inside, tree.dfs).tobytes()
        assert (counts[::4] == depth + 1).all() and 0 < counts[1::4].min() and counts[1::4].max() < 16


def test_region_symbols_are_declared_and_exported():
    from bvh_amd import _lib, build
    build.build()
    dll = _lib.load()
    header = open(os.path.join(ROOT, "include", "bvh_amd.h")).read()
    declared = set(re.findall(r"BVH_AMD_API[^;]*?\b(bvh\w+)\s*\(", header))
    want = {f"bvh{s}_region_{kind}" for s in ("3f", "3d") for kind in ("tris", "spheres")}
    assert {n for n in declared if "region" in n} == want
    assert want <= set(_lib.exported_symbols())
    for name in sorted(want):
        assert hasattr(dll, name), name
    for s in ("2f", "2d"):
        for kind in ("tris", "spheres"):
            assert not hasattr(dll, f"bvh{s}_region_{kind}")
    flags = {name: int(v) for name, v in re.findall(r"\b(BVH_AMD_(?:RAY|TRI|REGION)_\w+)\s*=\s*(\d+)u", header)}
    assert flags["BVH_AMD_REGION_EXACT"] == R.REGION_EXACT and len(flags) >= 7
    for name, v in flags.items():
        assert v & (v - 1) == 0 and (name == "BVH_AMD_REGION_EXACT" or v != flags["BVH_AMD_REGION_EXACT"]), name
    assert len(set(flags.values())) == len(flags)
