"""MI355X: batched winding-number and signed-distance queries (bvh3X_winding_prepare / bvh3X_winding_numbers, bvh_amd.winding_prepare /
winding_numbers / signed_distance / occupancy). The device's moments, winding numbers and counters are byte-equal to the host
harness's (the same text compiled by g++, tests/test_winding_host.py); values do not depend on batch order, the reordering flags or
the launches a batch is cut into; trees deeper than 64 levels; signed distance against closest_points and the analytic inside test;
flags and errors."""
import math

import numpy as np
import pytest

import query_slices as qs
import winding_scenes as ws
from test_closest_point_host import chain_tree, precompute
from test_winding_host import BETAS, compile_harness, host_prepare, host_walk, mirror_siblings, queries4

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return compile_harness(tmp_path_factory.mktemp("winding_gpu"))


_BUILT = {}


def device_scene(name, dtype, quality):
    """(Bvh, BVH-order PrecomputedTri in HBM, raw triangles) of a scene of winding_scenes under DefaultBuilder on the device."""
    import bvh_amd
    key = (name, np.dtype(dtype).name, quality)
    if key not in _BUILT:
        tris = np.ascontiguousarray(ws.SCENES[name][0]().astype(dtype))
        bb, cc = bvh_amd.tri_bounds(tris)
        bvh = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=getattr(bvh_amd.Quality, quality)))
        _BUILT[key] = (bvh, bvh_amd.precompute_tris(tris, bvh.device_prim_ids()), tris)
    return _BUILT[key]


def _np(t):
    return t.cpu().numpy()


def _host_moments(dll, bvh, dprims):
    nodes = bvh.nodes
    return host_prepare(dll, nodes["bounds"], nodes["index"], _np(dprims), threads=8)


def _device_vs_host(dll, bvh, dprims, moments, q, beta, **kw):
    import bvh_amd
    w, cnt = bvh_amd.winding_numbers(bvh, dprims, moments, q, beta=beta, counters=True, **kw)
    nodes = bvh.nodes
    h_w, h_cnt = host_walk(dll, nodes["bounds"], nodes["index"], _np(dprims), _np(moments), q, beta=beta, threads=16)
    assert _np(w).tobytes() == h_w.tobytes(), np.abs(_np(w) - h_w).max()
    assert (_np(cnt).astype(np.uint64) == h_cnt).all(), (cnt, h_cnt)
    return h_w


# ---- moments ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("quality", ["Low", "High"])
@pytest.mark.parametrize("name", ["sphere", "soup2k"])
def test_moments_device_equals_host(dll, name, quality, dtype):
    import bvh_amd
    bvh, dprims, _ = device_scene(name, dtype, quality)
    mom = bvh_amd.winding_prepare(bvh, dprims)
    assert mom.shape == (bvh.node_count + 1, 8)
    assert _np(mom).tobytes() == _host_moments(dll, bvh, dprims).tobytes()
    again = bvh_amd.winding_prepare(bvh, dprims)              # two runs: the climb's arrival order does not show
    assert _np(again).tobytes() == _np(mom).tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_moments_after_refit_tris(dll, dtype):
    import bvh_amd
    tris = np.ascontiguousarray(ws.uv_sphere().astype(dtype))
    bb, cc = bvh_amd.tri_bounds(tris)
    bvh = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.Medium))
    dprims = bvh_amd.precompute_tris(tris, bvh.device_prim_ids())
    stale = _np(bvh_amd.winding_prepare(bvh, dprims))
    rng = np.random.default_rng(2)
    moved = (tris.reshape(-1, 3) * np.array([1.5, 0.75, 1.25]) + np.array([0.2, -0.1, 0.3])).reshape(-1, 9)
    moved = np.ascontiguousarray((moved + 0.01 * rng.normal(size=moved.shape)).astype(dtype))
    dprims2 = bvh.refit_tris(moved)
    mom = bvh_amd.winding_prepare(bvh, dprims2)
    assert _np(mom).tobytes() == _host_moments(dll, bvh, dprims2).tobytes()
    assert _np(mom).tobytes() != stale.tobytes()
    q = queries4(ws.queries(moved.astype(np.float64), n=512)[0], dtype)
    _device_vs_host(dll, bvh, dprims2, mom, q, 2.0)


# ---- winding numbers --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("name,dtype", [("sphere", np.float32), ("sphere", np.float64), ("soup2k", np.float32), ("shell", np.float64)])
def test_winding_device_equals_host(dll, name, dtype, beta):
    import bvh_amd
    import torch
    bvh, dprims, tris = device_scene(name, dtype, "High")
    mom = bvh_amd.winding_prepare(bvh, dprims)
    pts, expect = ws.queries(tris.astype(np.float64), rule=ws.SCENES[name][1])
    q = queries4(pts, dtype)
    base = _device_vs_host(dll, bvh, dprims, mom, q, beta)
    if expect is not None:
        assert (np.rint(base).astype(np.int64) == expect).all()
    # the value of a query does not depend on the reordering, on the batch's order or on its place in a batch
    for sort in (True, False):
        assert _np(bvh_amd.winding_numbers(bvh, dprims, mom, q, beta=beta, sort_queries=sort)).tobytes() == base.tobytes()
    perm = np.random.default_rng(3).permutation(len(q))
    permuted = _np(bvh_amd.winding_numbers(bvh, dprims, mom, torch.from_numpy(q[perm]).cuda(), beta=beta, sort_queries=True))
    assert permuted.tobytes() == base[perm].tobytes()
    assert _np(bvh_amd.winding_numbers(bvh, dprims, mom, q[100:173], beta=beta)).tobytes() == base[100:173].tobytes()
    assert _np(bvh_amd.winding_numbers(bvh, dprims, mom, pts.astype(dtype), beta=beta)).tobytes() == base.tobytes()     # (n, 3) points


def test_winding_device_equals_host_sponza(dll):
    import bvh_amd
    from bvh_amd import synth
    tris = synth.sponza_proxy()
    bb, cc = bvh_amd.tri_bounds(tris)
    bvh = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.High))
    dprims = bvh_amd.precompute_tris(tris, bvh.device_prim_ids())
    mom = bvh_amd.winding_prepare(bvh, dprims)
    assert _np(mom).tobytes() == _host_moments(dll, bvh, dprims).tobytes()
    lo, hi = synth.scene_bounds(tris)
    q = queries4(synth.points_uniform(2048, lo, hi, seed=12), np.float32)
    w = _device_vs_host(dll, bvh, dprims, mom, q, 2.0)
    assert np.isfinite(w).all()


def test_nan_queries(dll):
    import bvh_amd
    import torch
    bvh, dprims, _ = device_scene("sphere", np.float32, "High")
    mom = bvh_amd.winding_prepare(bvh, dprims)
    q = queries4(np.array([[np.nan, 0, 0], [0, np.inf, 0], [0.1, 0.2, 0.3], [3, 3, 3]]), np.float32, fourth=np.nan)
    w = _device_vs_host(dll, bvh, dprims, mom, q, 2.0)
    assert np.isnan(w[:2]).all() and round(float(w[2])) == 1 and round(float(w[3])) == 0
    hits = bvh_amd.hits_to_numpy(bvh_amd.signed_distance(bvh, dprims, mom, q[:, :3].copy()))
    plain = bvh_amd.hits_to_numpy(bvh_amd.closest_points(bvh, dprims, q[:, :3].copy()))
    assert hits[[0, 1, 3]].tobytes() == plain[[0, 1, 3]].tobytes() and hits["t"][2] == -plain["t"][2]
    assert list(_np(bvh_amd.occupancy(bvh, dprims, mom, torch.from_numpy(q).cuda()))) == [False, False, True, False]


@pytest.mark.parametrize("depth", [65, 300])
@pytest.mark.parametrize("mirrored", [False, True])
def test_trees_deeper_than_64_levels(dll, restatement, depth, mirrored):
    import bvh_amd
    tris, nodes, ids = chain_tree(depth, restatement.prep_tris)
    if mirrored:
        nodes = mirror_siblings(nodes)
    bvh = bvh_amd.Bvh.from_nodes(nodes, ids)
    dprims = bvh_amd.precompute_tris(tris, bvh.device_prim_ids())
    assert _np(dprims).tobytes() == precompute(tris, np.float32).tobytes()
    mom = bvh_amd.winding_prepare(bvh, dprims)
    assert _np(mom).tobytes() == host_prepare(dll, nodes["bounds"], nodes["index"], _np(dprims)).tobytes()
    rng = np.random.default_rng(depth)
    pts = np.stack([4000 - depth + rng.random(4096) * depth, (rng.random(4096) - 0.5) * 1.5, (rng.random(4096) - 0.5) * 1.5], axis=1)
    q = queries4(pts, np.float32)
    for beta in (2.0, math.inf):
        w, cnt = bvh_amd.winding_numbers(bvh, dprims, mom, q, beta=beta, counters=True)
        h_w, h_cnt = host_walk(dll, nodes["bounds"], nodes["index"], _np(dprims), _np(mom), q, beta=beta, deep_cap=depth - 64 + 1, threads=16)
        assert _np(w).tobytes() == h_w.tobytes() and (_np(cnt).astype(np.uint64) == h_cnt).all()


def test_sliced_batch_over_a_deep_tree(dll):
    """A chain of 3001 levels with every inner child on the left: at beta = inf every lane stacks one entry per level, and the launch
    path cuts the batch in two (the spill of a launch holds per_launch lanes). The same bytes as the host walk, which knows nothing of
    launches."""
    import bvh_amd
    from bvh_amd import _lib
    depth = 3000
    tris, nodes, _ = qs.chain(depth, np.float32, stacked=True)
    bvh = bvh_amd.Bvh.from_nodes(nodes, np.arange(depth + 1, dtype=np.uint64))
    dprims = bvh_amd.precompute_tris(tris, bvh.device_prim_ids())
    mom = bvh_amd.winding_prepare(bvh, dprims)
    assert _np(mom).tobytes() == host_prepare(dll, nodes["bounds"], nodes["index"], _np(dprims)).tobytes()
    per = qs.per_launch(depth, 4)
    n = per + 300
    rng = np.random.default_rng(depth)
    base = qs.chain_base(depth)
    pts = np.stack([base - depth + rng.random(n) * depth, (rng.random(n) - 0.5) * 1.5, (rng.random(n) - 0.5) * 1.5], axis=1)
    q = queries4(pts, np.float32)
    w, cnt = bvh_amd.winding_numbers(bvh, dprims, mom, q, beta=math.inf, counters=True)
    assert _lib.load().bvh_amd_last_query_launches() == 2
    h_w, h_cnt = host_walk(dll, nodes["bounds"], nodes["index"], _np(dprims), _np(mom), q, beta=math.inf, deep_cap=qs.deep_cap(depth), threads=16)
    assert _np(w).tobytes() == h_w.tobytes() and (_np(cnt).astype(np.uint64) == h_cnt).all()
    assert h_cnt[0] == depth * n and h_cnt[1] == (depth + 1) * n


# ---- signed distance --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,dtype", [("sphere", np.float32), ("shell", np.float32), ("shell", np.float64)])
def test_signed_distance_and_occupancy(name, dtype):
    import bvh_amd
    bvh, dprims, tris = device_scene(name, dtype, "High")
    mom = bvh_amd.winding_prepare(bvh, dprims)
    pts, expect = ws.queries(tris.astype(np.float64), rule=ws.SCENES[name][1])
    pts = pts.astype(dtype)
    inside = expect >= 1
    assert inside.sum() > 100 and (~inside).sum() > 100
    plain = bvh_amd.hits_to_numpy(bvh_amd.closest_points(bvh, dprims, pts))
    signed = bvh_amd.hits_to_numpy(bvh_amd.signed_distance(bvh, dprims, mom, pts))
    assert ((signed["t"] < 0) == inside).all()
    back = signed.copy()
    back["t"] = np.abs(back["t"])
    assert back.tobytes() == plain.tobytes()                  # |t| and every other field: closest_points' bytes
    assert (_np(bvh_amd.occupancy(bvh, dprims, mom, pts)) == inside).all()
    # a finite max_distance: misses keep prim = INVALID and carry the radius, negated inside
    near = bvh_amd.hits_to_numpy(bvh_amd.signed_distance(bvh, dprims, mom, pts, max_distance=0.05))
    plain_near = bvh_amd.hits_to_numpy(bvh_amd.closest_points(bvh, dprims, pts, max_distance=0.05))
    assert ((near["t"] < 0) == inside).all() and (near["prim"] == plain_near["prim"]).all() and (np.abs(near["t"]) == plain_near["t"]).all()


# ---- flags and errors -------------------------------------------------------------------------------------------------------------------

def test_flags_and_errors():
    import bvh_amd
    import torch
    from bvh_amd import _lib
    from conftest import load_golden
    bvh, dprims, tris = device_scene("sphere", np.float32, "High")
    mom = bvh_amd.winding_prepare(bvh, dprims)
    rows = mom.shape[0]
    q = torch.from_numpy(queries4(ws.queries(tris.astype(np.float64), n=256)[0], np.float32)).cuda()
    n = q.shape[0]
    lib = _lib.load()
    SENT = 1234.5
    w = torch.full((n,), SENT, dtype=torch.float32, device="cuda")
    hits = torch.full((n, 4), SENT, dtype=torch.float32, device="cuda")
    cnt = torch.full((3,), 77, dtype=torch.int64, device="cuda")
    f, prep = lib.bvh3f_winding_numbers, lib.bvh3f_winding_prepare
    P = lambda t: t.data_ptr()

    def refused(rc, word):
        torch.cuda.synchronize()
        assert rc == -2 and word in _lib.last_error(), (rc, _lib.last_error())
        assert (w == SENT).all() and (hits == SENT).all() and (cnt == 77).all()          # nothing was written

    assert f(bvh._h, P(dprims), P(mom), rows, P(q), 0, 2.0, 0, None, None, None, None) == 0           # n == 0: a no-op
    refused(f(bvh._h, P(dprims), P(mom), rows, P(q), n, 0.5, 0, P(w), P(hits), P(cnt), None), "beta")
    refused(f(bvh._h, P(dprims), P(mom), rows, P(q), n, math.nan, 0, P(w), P(hits), P(cnt), None), "beta")
    refused(f(bvh._h, P(dprims), P(mom), rows, P(q), n, 2.0, 8, P(w), P(hits), P(cnt), None), "flags")          # ORIGINAL_IDS
    refused(f(bvh._h, P(dprims), P(mom), rows, P(q), n, 2.0, 1, P(w), P(hits), P(cnt), None), "flags")          # ANY_HIT
    refused(f(bvh._h, None, P(mom), rows, P(q), n, 2.0, 0, P(w), P(hits), P(cnt), None), "null")
    refused(f(bvh._h, P(dprims), None, rows, P(q), n, 2.0, 0, P(w), P(hits), P(cnt), None), "null")
    refused(f(bvh._h, P(dprims), P(mom), rows, None, n, 2.0, 0, P(w), P(hits), P(cnt), None), "null")
    refused(f(bvh._h, P(dprims), P(mom), rows, P(q), n, 2.0, 0, None, P(hits), P(cnt), None), "null")
    refused(f(bvh._h, P(dprims), P(mom) + 4, rows, P(q), n, 2.0, 0, P(w), P(hits), P(cnt), None), "aligned")
    refused(f(bvh._h, P(dprims), P(mom), rows, P(q) + 4, n - 1, 2.0, 0, P(w), P(hits), P(cnt), None), "aligned")
    refused(f(bvh._h, P(dprims), P(mom), rows - 1, P(q), n, 2.0, 0, P(w), P(hits), P(cnt), None), "rows")
    refused(f(None, P(dprims), P(mom), rows, P(q), n, 2.0, 0, P(w), P(hits), P(cnt), None), "null")
    # prepare: the same checks, and the caller's buffer untouched
    buf = torch.full((rows, 8), SENT, dtype=torch.float32, device="cuda")

    def prep_refused(rc, word):
        torch.cuda.synchronize()
        assert rc == -2 and word in _lib.last_error(), (rc, _lib.last_error())
        assert (buf == SENT).all()

    prep_refused(prep(bvh._h, None, P(buf), rows, None), "null")
    prep_refused(prep(bvh._h, P(dprims), None, rows, None), "null")
    prep_refused(prep(bvh._h, P(dprims), P(buf) + 4, rows - 1, None), "aligned")
    prep_refused(prep(bvh._h, P(dprims), P(buf), rows - 1, None), "rows")
    prep_refused(prep(None, P(dprims), P(buf), rows, None), "null")
    # a 2D tree: the C ABI and the Python layer
    g2 = load_golden("circles2k_2f")
    bb, cc = bvh_amd.sphere_bounds(g2["prims"])
    bvh2 = bvh_amd.DefaultBuilder.build(bb, cc)
    prep_refused(prep(bvh2._h, P(dprims), P(buf), max(rows, bvh2.node_count + 1), None), "3D")
    refused(f(bvh2._h, P(dprims), P(mom), max(rows, bvh2.node_count + 1), P(q), n, 2.0, 0, P(w), P(hits), P(cnt), None), "3D")
    with pytest.raises(TypeError):
        bvh_amd.winding_prepare(bvh2, dprims)
    with pytest.raises(TypeError):
        bvh_amd.winding_numbers(bvh2, dprims, mom, q)
    with pytest.raises(TypeError):
        bvh_amd.winding_numbers(bvh, dprims, mom, np.zeros((4, 3), np.float64))
    with pytest.raises(bvh_amd.BvhAmdError):
        bvh_amd.winding_numbers(bvh, dprims, mom, q, beta=0.5)
    with pytest.raises(bvh_amd.BvhAmdError):
        bvh_amd.winding_numbers(bvh, dprims, mom[:-1], q)
    assert bvh_amd.winding_numbers(bvh, dprims, mom, np.zeros((0, 3), np.float32)).shape == (0,)
    # out= is written in place
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    assert bvh_amd.winding_numbers(bvh, dprims, mom, q, out=out).data_ptr() == out.data_ptr()
    into = torch.empty((rows, 8), dtype=torch.float32, device="cuda")
    assert bvh_amd.winding_prepare(bvh, dprims, out=into).data_ptr() == into.data_ptr() and _np(into).tobytes() == _np(mom).tobytes()
