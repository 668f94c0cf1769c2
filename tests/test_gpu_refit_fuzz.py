"""MI355X: the device refit from moved primitives (k_refit_prims / k_refit_parents behind Bvh.refit_boxes and Bvh.refit_tris) on the
cases and tree-aware moves of tests/refit_adversarial.py — signed zeros, NaN in the slots where it stays and where it vanishes,
infinities and empty boxes, a root of zero extent, foreign geometry — against the checker's own Bvh::refit, byte for byte.

The trees come from the device builders (checked against the checker's build first) with leaf limits from (1, 1) to (9, 15), from
one primitive to 1500, and enter their first refit in one of six states: fresh, serialized, from_nodes, deserialize, after a host edit
of an inner box, after optimize(). The seven moves run in sequence on the same tree. tests/test_refit_fuzz_host.py holds the
conditions under which these comparisons would catch a fold turned into hardware min / max, a reversed comparison, or a climb that
combines the children the other way round.

Downstream of the refit: the bounds kernels on the moved arrays, tracing and closest_points on roots with a NaN, an infinite or no
extent (also reordered: ray_key.h / query_order.h scale their keys by that root), and traversal_cost()."""
import numpy as np
import pytest

import adversarial_queries as adv
import refit_adversarial as ra
from test_gpu_fuzz import _rays3
from test_gpu_query_fuzz import device_build
from test_gpu_refit_prims import _check_cost, _wide_array, expected_tree

pytestmark = pytest.mark.gpu

STATES = ("optimize", "fresh", "serialized", "from_nodes", "deserialize", "host_edit")
TRACED = ("nan_root", "inf", "collapse", "other_kind")
N_RAYS = 2000
N_POINTS = 1021


def _deal(cases, states):
    """{case: state}: round robin over the cases in order of decreasing size, so that every state meets a deep tree and a tiny one."""
    order = sorted(range(len(cases)), key=lambda j: (-cases[j][1], j))
    return {cases[j]: states[rank % len(states)] for rank, j in enumerate(order)}


STATE_OF = {**_deal(ra.CASES3, STATES), **_deal(ra.CASES2, STATES[1:])}      # (the reinsertion optimizer is 3D)


def _np(t):
    return t.cpu().numpy()


def _same_or_both_nan(got, want):
    """Bytewise, except that a NaN equals a NaN: where a NaN is COMPUTED (a centre, an edge or a normal of a triangle with a NaN or
    two infinities in it) x86 and the GPU differ in the sign of the NaN they generate. Selected values never come here."""
    u = np.uint32 if got.dtype == np.float32 else np.uint64
    return bool(((np.ascontiguousarray(got).view(u) == np.ascontiguousarray(want).view(u)) | (np.isnan(got) & np.isnan(want))).all())


def _hits_equal(got, want):
    """test_gpu_fuzz.py's equality of hit records."""
    return (got["prim"] == want["prim"]) & ((got["t"] == want["t"]) | (np.isnan(got["t"]) & np.isnan(want["t"])))


def enter(state, case, orc, raw, bb, cc):
    """The device tree of the case in `state`, and the (nodes, prim_ids) its refits keep the topology of."""
    import bvh_amd
    kind, n, lim, bq, dtype, seed = case
    dim = ra.dim_of(case)
    ref = orc.build(bb, cc, builder=bq[0], quality=bq[1], min_leaf=lim[0], max_leaf=lim[1])
    gpu = device_build(bb, cc, lim, bq)
    assert gpu.serialize() == ref.serialize(), (adv.case_id(case), "build")
    nodes, ids = ref.nodes(), ref.prim_ids()
    if state == "fresh":                                       # a second build nothing on the host has looked at: the mirror never filled
        gpu = device_build(bb, cc, lim, bq)
    elif state == "from_nodes":
        gpu = bvh_amd.Bvh.from_nodes(nodes, ids)
    elif state == "deserialize":
        gpu = bvh_amd.Bvh.deserialize(ref.serialize(), dtype=dtype, dim=dim)
    elif state == "host_edit":                                 # an inner box edited in the mirror: the refit must overwrite it
        inner = np.flatnonzero((nodes["index"] & 15) == 0)
        if len(inner):
            gpu.set_node_bbox(int(inner[len(inner) // 2]), [-100.0] * dim, [100.0] * dim)
    elif state == "optimize":
        ref.optimize(-1)
        gpu.optimize()
        assert gpu.serialize() == ref.serialize(), (adv.case_id(case), "optimize")
        nodes, ids = gpu.nodes, gpu.prim_ids                   # the refits below must follow THIS topology (new parent links)
        assert nodes.tobytes() == ref.nodes().tobytes() and (ids == ref.prim_ids()).all()
    return gpu, nodes, ids


def check_bounds_kernels(orc, moved):
    """tri_bounds on a moved triangle array: boxes bytewise (selected), centres with NaN == NaN (computed). -> the device boxes."""
    import bvh_amd
    d_bb, d_cc = bvh_amd.tri_bounds(moved)
    bb, cc = orc.prep_tris(moved)
    assert _np(d_bb).tobytes() == bb.tobytes()
    assert _same_or_both_nan(_np(d_cc), cc)
    return d_bb


def _aim(r, moved, rng, dim):
    """Every fourth ray of the batch is turned towards a finite vertex (box corner) of the moved geometry, and every third of those
    is moved onto an axis through it: on a collapsed scene nothing else meets the root box, and a ray along an axis through a box of
    zero extent is where the slab test multiplies 0 by inf."""
    pts = moved.reshape(-1, 3) if moved.shape[1] == 9 else moved.reshape(-1, dim)
    sites = pts[np.isfinite(pts).all(axis=1) & (np.abs(pts) < np.finfo(moved.dtype).max).all(axis=1)].astype(np.float64)
    if not len(sites):
        return r
    k = np.arange(0, len(r), 4)
    tgt = sites[rng.integers(0, len(sites), size=len(k))]
    r[k, dim:2 * dim] = tgt - r[k, :dim].astype(np.float64)
    ax, t = k[::3], tgt[::3]
    a = rng.integers(0, dim, size=len(ax))
    side = np.where(rng.random(len(ax)) < 0.5, 1.0, -1.0)
    org = t.copy()
    org[np.arange(len(ax)), a] += side * (1.0 + np.abs(t[np.arange(len(ax)), a]))
    r[ax, :dim] = org
    r[ax, dim:2 * dim] = 0
    r[ax, dim + a] = -side
    return r


def rays_for(case, moved, rng):
    """(closest rays, any-hit rays): test_gpu_fuzz's rays over the finite part of the moved scene's extent, a quarter of them aimed."""
    dim, dtype = ra.dim_of(case), case[4]
    lo, hi = ra.finite_extent(moved, dim)
    if dim == 3:
        return [_aim(_rays3(rng, N_RAYS, lo, hi, dtype), moved, rng, 3) for _ in range(2)]
    out = []
    for _ in range(2):                                         # test_gpu_fuzz.test_fuzz_2d's rays, over this extent
        r = np.zeros((N_RAYS, 6), dtype=dtype)
        ext = np.maximum(hi - lo, 1e-3)
        r[:, 0:2] = lo - 0.2 * ext + rng.random((N_RAYS, 2)) * 1.4 * ext
        d = rng.standard_normal((N_RAYS, 2))
        d[::5, 0] = 0
        d[1::5, 1] = -0.0
        r[:, 2:4] = d
        r[:, 4] = np.where(rng.random(N_RAYS) < 0.1, -2.0, 0.0)
        r[:, 5] = np.where(rng.random(N_RAYS) < 0.3, rng.random(N_RAYS) * ext.max(), np.finfo(dtype).max)
        out.append(_aim(r, moved, rng, 2))
    return out


def trace_and_query(case, gpu, want, prims, oprims, moved, rng, what):
    """Closest and any-hit, robust on and off, unsorted and reordered, against the checker on ITS refitted tree, counters included;
    the reordered batches equal the unsorted ones bytewise; closest_points reordered equals unsorted (3D)."""
    import bvh_amd
    leaf = "tri" if ra.is_tri(case) else "sphere"
    cpu_trace = want.intersect_tri if ra.is_tri(case) else want.intersect_sphere
    rays, srays = rays_for(case, moved, rng)
    n_hit = 0
    for any_hit in (False, True):
        batch = srays if any_hit else rays
        for robust in (False, True):
            w, cw = cpu_trace(oprims, batch, any_hit, robust, threads=4, counters=True)
            unsorted = None
            for sort_rays in (None, False, True):
                got, cg = bvh_amd.intersect(gpu, prims, batch, any_hit=any_hit, robust=robust, leaf=leaf, counters=True, sort_rays=sort_rays)
                g = bvh_amd.hits_to_numpy(got)
                same = _hits_equal(g, w)
                assert same.all(), (what, any_hit, robust, sort_rays, int((~same).sum()))
                assert (_np(cg).astype(np.uint64) == cw).all(), (what, any_hit, robust, sort_rays, _np(cg), cw)
                if sort_rays is False:
                    unsorted = g.tobytes()
                    n_hit += int((g["prim"] != bvh_amd.INVALID).sum())
                elif sort_rays:
                    assert g.tobytes() == unsorted, (what, any_hit, robust, "reordered batch differs from the unsorted one")
    if ra.dim_of(case) == 3:
        lo, hi = ra.finite_extent(moved, 3)
        pts = (lo - 0.2 * (hi - lo) + rng.random((N_POINTS, 3)) * 1.4 * np.maximum(hi - lo, 1e-3)).astype(case[4])
        plain = bvh_amd.hits_to_numpy(bvh_amd.closest_points(gpu, prims, pts, leaf=leaf, sort_queries=False))
        sorted_ = bvh_amd.hits_to_numpy(bvh_amd.closest_points(gpu, prims, pts, leaf=leaf, sort_queries=True))
        assert sorted_.tobytes() == plain.tobytes(), (what, "closest_points, reordered")
    return n_hit


def check_cost(gpu, want_nodes, what):
    """traversal_cost() on the refitted tree: within test_gpu_refit_prims._check_cost's bound where every box is finite and the root
    has a half-area; exactly 0 where the root's half-area is zero or not finite (upload.hip hands the kernel inv_root_area = 0 then, and
    every share r > 0 fails)."""
    b = want_nodes["bounds"][0].astype(np.float64)
    x, y, z = b[1] - b[0], b[3] - b[2], b[5] - b[4]
    with np.errstate(all="ignore"):
        area = x * y + y * z + z * x
    got = gpu.traversal_cost()
    assert np.isfinite(got) and got >= 0, (what, got)
    if np.isfinite(want_nodes["bounds"]).all() and np.isfinite(area) and area > 0:
        _check_cost(gpu)
    elif not (np.isfinite(area) and area > 0):
        assert got == 0.0, (what, got, area)


@pytest.mark.parametrize("j", range(len(ra.CASES)), ids=[adv.case_id(c) for c in ra.CASES])
def test_refit_sequence(orc, j):
    import bvh_amd
    case = ra.CASES[j]
    kind, n, lim, bq, dtype, seed = case
    dim, tri, what = ra.dim_of(case), ra.is_tri(case), adv.case_id(case)
    state = STATE_OF[case]
    raw = ra.scene(case)
    bb, cc = ra.bounds(orc, raw)
    d_bb, d_cc = (bvh_amd.tri_bounds if tri else bvh_amd.sphere_bounds)(raw)
    assert _np(d_bb).tobytes() == bb.tobytes() and _np(d_cc).tobytes() == cc.tobytes()
    gpu, nodes, ids = enter(state, case, orc, raw, bb, cc)
    perm = ids.astype(np.int64)
    node_count = len(nodes)
    rng = np.random.default_rng(seed + 7)
    out = None
    n_hit = {}
    for m, name in enumerate(ra.MOVES):
        moved = ra.apply(case, name, raw, nodes, ids)
        mb = ra.moved_boxes(orc, moved)
        want = expected_tree(orc, nodes, ids, mb, dim)
        stream = want.serialize()
        # where the boxes come from: the bounds kernels on the device; once per case a plain numpy array
        if tri:
            src = check_bounds_kernels(orc, moved)
        else:
            sph = ra.sphere_source(case, name, raw)
            if sph is not None:
                src, _ = bvh_amd.sphere_bounds(sph)
                assert _np(src).tobytes() == orc.sphere_bboxes(sph)[0].tobytes() == mb.tobytes(), (what, name)
            else:
                src = mb
        if m == j % len(ra.MOVES):
            src = mb
        prims = None
        for method in (("boxes", "tris") if (m + j) % 2 == 0 else ("tris", "boxes")) if tri else ("boxes",):
            for call in ("first", "steady"):
                if method == "boxes":
                    gpu.refit_boxes(src)
                else:                                          # every other move into the tensor the last one returned
                    prims = out = gpu.refit_tris(moved, out=out if m % 2 else None)
                assert gpu.serialize() == stream, (what, state, name, method, call)
                assert gpu.node_count == node_count and (gpu.prim_ids == ids).all(), (what, name, method)
        if tri:
            # refit_tris' PrecomputedTri rows: e1, e2 and n are computed, so NaN == NaN there (see _same_or_both_nan)
            oprims = orc.precompute_tris(moved, ids)
            assert _same_or_both_nan(_np(prims), oprims), (what, name)
            assert _np(prims).tobytes() == _np(bvh_amd.precompute_tris(moved, gpu.device_prim_ids())).tobytes(), (what, name)
        else:
            oprims = np.ascontiguousarray(raw[perm])           # the leaf test keeps the built spheres: only the boxes moved
            prims = bvh_amd.gather(raw, gpu.device_prim_ids())
        if name in TRACED:
            n_hit[name] = trace_and_query(case, gpu, want, prims, oprims, moved, rng, (what, state, name))
            assert gpu.serialize() == stream, (what, name, "after tracing")
        if dim == 3:
            check_cost(gpu, want.nodes(), (what, name))
    print(f"{what}: entered as {state}, {node_count} nodes; hits of 4 x {N_RAYS} rays per traced move: {n_hit}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_wide_array_with_zeros_and_nan(orc, dtype):
    """test_gpu_refit_prims._wide_array (unused sibling pairs, an 80-deep unused chain behind the reachable tree) refitted to the
    `zeros` and the `nan_leaf` boxes: every leaf of the ARRAY is refitted, like the reference's traverse_bottom_up."""
    import bvh_amd
    case = next(c for c in ra.CASES3 if c[1] == 200 and c[2] == (9, 15))
    case = (case[0], case[1], case[2], case[3], dtype, case[5])
    raw, nodes, ids = ra.checker_tree(orc, case)
    wide = _wide_array(nodes)
    t = bvh_amd.Bvh.from_nodes(wide, ids)
    for name in ("zeros", "nan_leaf"):
        mb = ra.moved_boxes(orc, ra.apply(case, name, raw, nodes, ids))
        want = expected_tree(orc, wide, ids, mb)
        t.refit_boxes(mb)
        assert t.serialize() == want.serialize(), name
        t.refit_boxes(mb)
        assert t.serialize() == want.serialize(), (name, "steady")
