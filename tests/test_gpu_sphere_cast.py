"""MI355X: batched sphere-cast queries (bvh3X_sphere_cast_*, bvh_amd.sphere_cast). The device's records and counters are byte-equal
to the host harness's (the same text compiled by g++, tests/test_sphere_cast_host.py) on the golden scenes and a 20,000-sphere float
scene, with a scalar radius and a per-ray array, the fast and the robust box test; trees deeper than 64 levels, a one-primitive tree,
n = 1 and n = 0; a record does not depend on the reordering flags, on the batch it is in, or on ORIGINAL_IDS beyond prim; out= is
honoured; residuals against a float64 brute force in torch; refusals. (The refusal of a tree without a device copy is
point_query_check's, shared with the other queries; no constructor of the library leaves such a tree, so it is not reached here.)"""
import numpy as np
import pytest

from conftest import load_golden
from test_closest_point_host import INVALID, chain_tree, golden_scene, precompute
from test_sphere_cast_host import TOL, TRI, INTERIOR, NRM, _ray, compile_harness, host_brute, host_walk, prim_residuals, scene_rays

pytestmark = pytest.mark.gpu

ROBUST, SORTED, ORIGINAL_IDS, UNSORTED = 2, 4, 8, 16


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return compile_harness(tmp_path_factory.mktemp("sphere_cast_gpu"))


def _device_vs_host(dll, bvh, prims, rays, radius, leaf, robust, deep_cap=0):
    """bvh_amd.sphere_cast against the host walk over the tree's own nodes: records and counters, byte for byte."""
    import bvh_amd
    hits, cnt = bvh_amd.sphere_cast(bvh, prims, rays, radius, leaf="sphere" if leaf else "tri", robust=robust, counters=True)
    nodes = bvh.nodes
    h_hits, h_cnt = host_walk(dll, nodes["bounds"], nodes["index"], prims, rays, radius, leaf, robust=robust, deep_cap=deep_cap, threads=8)
    got = bvh_amd.hits_to_numpy(hits)
    assert got.tobytes() == h_hits.tobytes(), np.flatnonzero((got["prim"] != h_hits["prim"]) | (got["t"] != h_hits["t"]))[:8]
    assert (cnt.cpu().numpy().astype(np.uint64) == h_cnt).all(), (cnt, h_cnt)
    return h_hits


@pytest.mark.parametrize("scene", ["cornell", "soup2k", "terrain2k", "soup2k_f64", "spheres2k_f64"])
@pytest.mark.parametrize("robust", [False, True])
def test_device_equals_host_golden(dll, orc, scene, robust):
    import bvh_amd
    g = load_golden(scene)
    _, _, prims, leaf, raw, _ = golden_scene(scene, "parallel_high", orc)
    bvh = bvh_amd.Bvh.deserialize(g["bvh_parallel_high"].tobytes(), dtype=prims.dtype.type)
    rays, radii, diag = scene_rays(raw, 2048, prims.dtype.type, 7, leaf == 1)
    hits = _device_vs_host(dll, bvh, prims, rays, radii, leaf, robust)                     # one radius per ray
    assert 200 < (hits["prim"] != INVALID).sum() < len(rays)
    _device_vs_host(dll, bvh, prims, rays, 0.01 * diag, leaf, robust)                      # one radius for the batch


def test_device_equals_host_float_spheres(dll):
    import bvh_amd
    from bvh_amd import synth
    sph = synth.spheres(20000, dtype=np.float32)
    bb, cc = bvh_amd.sphere_bounds(sph)
    bvh = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.Medium))
    prims = bvh_amd.gather(sph, bvh.device_prim_ids()).cpu().numpy()
    rays, radii, diag = scene_rays(sph, 2048, np.float32, 8, True)
    for robust in (False, True):
        hits = _device_vs_host(dll, bvh, prims, rays, radii, 1, robust)
        _device_vs_host(dll, bvh, prims, rays, 0.002 * diag, 1, robust)
    assert 200 < (hits["prim"] != INVALID).sum()


@pytest.mark.parametrize("depth", [65, 300])
def test_trees_deeper_than_64_levels(dll, restatement, depth):
    """The Deep kernels: a chain tree, one push per level, the stack spilling to HBM; 300 rays (not a multiple of the block)."""
    import bvh_amd
    tris, nodes, ids = chain_tree(depth, restatement.prep_tris)
    bvh = bvh_amd.Bvh.from_nodes(nodes, ids)
    prims = precompute(tris, np.float32)
    rng = np.random.default_rng(depth)
    n = 300
    rays = np.zeros((n, 8), dtype=np.float32)
    rays[:, 0] = rng.integers(0, 100, n)
    rays[:, 1:3] = rng.integers(-2, 3, (n, 2)) / 4.0
    rays[:, 3] = 1.0
    rays[:, 7] = np.inf
    for robust in (False, True):
        hits = _device_vs_host(dll, bvh, prims, rays, 0.25, 0, robust, deep_cap=depth - 64 + 1)
        brute, _ = host_brute(dll, prims, rays, 0.25, 0)
        assert hits.tobytes() == brute.tobytes() and (hits["prim"] == depth).all()


def test_one_primitive_tree_and_tiny_batches(dll):
    import bvh_amd
    from oracle import NODEF
    tri = TRI.astype(np.float32)[None]
    nodes = np.zeros(1, dtype=NODEF)
    nodes[0]["bounds"] = [tri[0, 0::3].min(), tri[0, 0::3].max(), tri[0, 1::3].min(), tri[0, 1::3].max(), tri[0, 2::3].min(), tri[0, 2::3].max()]
    nodes[0]["index"] = (0 << 4) | 1
    bvh = bvh_amd.Bvh.from_nodes(nodes, np.zeros(1, dtype=np.uint64))
    prims = precompute(tri, np.float32)
    base = _ray(INTERIOR + 2.0 * NRM, -NRM, 0.0, 10.0)
    rays = np.stack([base, _ray(INTERIOR + 2.0 * NRM, -NRM, np.nan, 10.0), _ray(INTERIOR + 2.0 * NRM, -NRM, 0.0, np.nan),
                     _ray(INTERIOR + 2.0 * NRM, -NRM, 3.0, 1.0), _ray(INTERIOR + 2.0 * NRM, NRM, 0.0, 10.0), base, base,
                     _ray(INTERIOR + 0.1 * NRM, np.zeros(3), 0.5, 10.0)]).astype(np.float32)
    radii = np.array([0.25, 0.25, 0.25, 0.25, 0.25, -1.0, np.nan, 0.25], dtype=np.float32)
    hits = _device_vs_host(dll, bvh, prims, rays, radii, 0, False)
    assert hits["prim"][0] == 0 and abs(hits["t"][0] - 1.75) <= 1e-5 and (hits["prim"][1:7] == INVALID).all()
    assert hits["prim"][7] == 0 and hits["t"][7] == 0.5       # dir = 0: the overlap at c(tmin)
    one = _device_vs_host(dll, bvh, prims, rays[:1], 0.25, 0, True)                          # n = 1
    assert one.tobytes() == hits[:1].tobytes()
    empty = bvh_amd.sphere_cast(bvh, prims, np.zeros((0, 8), np.float32), 0.25)             # n = 0
    assert empty.shape == (0, 4)
    assert bvh_amd.sphere_cast(bvh, prims, np.zeros((0, 8), np.float32), np.zeros(0, np.float32)).shape == (0, 4)


@pytest.fixture(scope="module")
def soup(dll):
    """The 2k soup, 2,048 rays with their radii, the device tree and the host harness's records."""
    import bvh_amd
    import oracle
    orc = oracle.load_oracle()
    g = load_golden("soup2k")
    _, _, prims, leaf, raw, ids = golden_scene("soup2k", "parallel_high", orc)
    bvh = bvh_amd.Bvh.deserialize(g["bvh_parallel_high"].tobytes())
    rays, radii, diag = scene_rays(raw, 2048, np.float32, 11, False)
    nodes = bvh.nodes
    host, _ = host_walk(dll, nodes["bounds"], nodes["index"], prims, rays, radii, 0, threads=8)
    return bvh, prims, raw, ids, rays, radii, host


def test_flags_batches_and_out(soup):
    import bvh_amd
    import torch
    bvh, prims, raw, ids, rays, radii, host = soup
    cast = lambda r, rad, **kw: bvh_amd.hits_to_numpy(bvh_amd.sphere_cast(bvh, prims, r, rad, **kw))
    base = cast(rays, radii, sort_queries=False)
    assert base.tobytes() == host.tobytes()
    assert cast(rays, radii, sort_queries=True).tobytes() == base.tobytes()                  # SORTED against UNSORTED
    assert cast(rays, radii).tobytes() == base.tobytes()
    half = len(rays) // 2
    assert np.concatenate([cast(rays[:half], radii[:half]), cast(rays[half:], radii[half:], sort_queries=True)]).tobytes() == base.tobytes()
    perm = np.random.default_rng(3).permutation(len(rays))
    assert cast(rays[perm], radii[perm], sort_queries=True).tobytes() == base[perm].tobytes()
    orig = cast(rays, radii, original_ids=True, sort_queries=True)                           # ORIGINAL_IDS maps prim and nothing else
    hit = base["prim"] != INVALID
    assert (orig["prim"][hit] == ids[base["prim"][hit].astype(np.int64)]).all() and (orig["prim"][~hit] == INVALID).all()
    for f in ("t", "u", "v"):
        assert orig[f].tobytes() == base[f].tobytes()
    out = torch.full((len(rays) + 3, 4), 7.0, dtype=torch.float32, device="cuda")            # out= is honoured, nothing beyond n records written
    back = bvh_amd.sphere_cast(bvh, prims, rays, torch.from_numpy(radii).cuda(), out=out)
    assert back.data_ptr() == out.data_ptr()
    assert bvh_amd.hits_to_numpy(out[:len(rays)]).tobytes() == base.tobytes() and (out[len(rays):] == 7.0).all().item()


def test_residuals_against_f64_brute_force(soup):
    """Every reported contact touches: the float64 distance from c(t) to the NEAREST triangle of the whole scene is r (at most r where
    t == tmin), within TOL * scale; and nothing is penetrated deeper than that on the way there or, for a miss, on the way to tmax."""
    import bvh_amd
    import torch
    from test_gpu_closest_point import brute_f64
    bvh, prims, raw, ids, rays, radii, host = soup
    hits = bvh_amd.hits_to_numpy(bvh_amd.sphere_cast(bvh, prims, rays, radii))
    hit = hits["prim"] != INVALID
    rays64, r = rays.astype(np.float64), radii.astype(np.float64)
    tol = TOL[np.float32]
    res = prim_residuals(raw, ids, rays, radii, hits, False)
    print(f"soup2k on the device: hits {int(hit.sum())}/{len(hit)}, max residual/scale {res.max():.3e}")
    assert (res <= tol).all(), res.max()
    end = np.where(hit, hits["t"].astype(np.float64), np.minimum(rays64[:, 7], 4.0))       # (an unbounded miss: checked up to t = 4)
    scale = np.maximum(np.abs(raw).max(), np.abs(rays64[:, :3] + end[:, None] * rays64[:, 3:6]).max(axis=1))
    scale = np.maximum(scale, np.abs(rays64[:, :3]).max(axis=1))
    for frac in (1.0, 0.75, 0.5, 0.25, 0.0):
        t = rays64[:, 6] + frac * (end - rays64[:, 6])
        d = brute_f64(torch, raw, rays64[:, :3] + t[:, None] * rays64[:, 3:6])
        started_in = hit & (hits["t"] == rays[:, 6])
        assert ((d >= r - tol * scale) | started_in).all(), (frac, np.flatnonzero((d < r - tol * scale) & ~started_in)[:8])
        if frac == 1.0:
            assert (np.abs(d - r) <= tol * scale)[hit & ~started_in].all()
            assert (d <= r + tol * scale)[started_in].all()


def test_refusals(soup):
    import bvh_amd
    import torch
    from bvh_amd import _lib
    bvh, prims, raw, ids, rays, radii, host = soup
    lib = _lib.load()
    n = len(rays)
    dp, dr, drad = torch.from_numpy(prims).cuda(), torch.from_numpy(rays).cuda(), torch.from_numpy(radii).cuda()
    rec = torch.zeros((n + 8, 4), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    f = lib.bvh3f_sphere_cast_tri
    P = lambda t: t.data_ptr()

    def refused(rc, word):
        assert rc == -2 and word in _lib.last_error(), (rc, _lib.last_error())

    for ok in (0, ROBUST, SORTED | ROBUST | ORIGINAL_IDS, UNSORTED):
        assert f(bvh._h, P(dp), P(dr), n, 0.01, P(drad), ok, P(rec), P(cnt), None) == 0, _lib.last_error()
    assert f(bvh._h, P(dp), P(dr), n, 0.01, None, 0, P(rec), None, None) == 0, _lib.last_error()     # radii and counters are optional
    assert f(bvh._h, P(dp), None, 0, 0.01, None, 0, None, None, None) == 0                            # n == 0: a no-op
    for bad in (1, 1 | ROBUST, 32, 1 << 20):                                                         # ANY_HIT, unknown bits
        refused(f(bvh._h, P(dp), P(dr), n, 0.01, None, bad, P(rec), None, None), "flags")
    refused(f(None, P(dp), P(dr), n, 0.01, None, 0, P(rec), None, None), "null bvh")
    refused(f(bvh._h, None, P(dr), n, 0.01, None, 0, P(rec), None, None), "null device pointer")
    refused(f(bvh._h, P(dp), None, n, 0.01, None, 0, P(rec), None, None), "null device pointer")
    refused(f(bvh._h, P(dp), P(dr), n, 0.01, None, 0, None, None, None), "null device pointer")
    for args in ((P(dp) + 4, P(dr), n, 0.01, None, 0, P(rec), None, None),                           # misaligned prims, rays, radii,
                 (P(dp), P(dr) + 8, n - 1, 0.01, None, 0, P(rec), None, None),                       # records, counters
                 (P(dp), P(dr), n, 0.01, P(drad) + 2, 0, P(rec), None, None),
                 (P(dp), P(dr), n, 0.01, None, 0, P(rec) + 8, None, None),
                 (P(dp), P(dr), n, 0.01, None, 0, P(rec), P(cnt) + 4, None)):
        refused(f(bvh._h, *args), "aligned")
    # alignment to the element is enough: radii from their second entry, records from the second record, counters from their second
    assert f(bvh._h, P(dp), P(dr), n - 1, 0.01, P(drad) + 4, 0, P(rec) + 16, P(cnt) + 8, None) == 0, _lib.last_error()
    g2 = load_golden("circles2k_2f")                                                                 # a 2D tree
    b2, c2 = bvh_amd.sphere_bounds(g2["prims"])
    bvh2 = bvh_amd.DefaultBuilder.build(b2, c2)
    refused(f(bvh2._h, P(dp), P(dr), n, 0.01, None, 0, P(rec), None, None), "3D trees only")
    for call in (lambda: bvh_amd.sphere_cast(bvh2, prims, rays, 0.01), lambda: bvh_amd.sphere_cast(bvh, prims, rays.astype(np.float64), 0.01),
                 lambda: bvh_amd.sphere_cast(bvh, prims.astype(np.float64), rays, 0.01), lambda: bvh_amd.sphere_cast(bvh, prims, rays, radii.astype(np.float64)),
                 lambda: bvh_amd.sphere_cast(bvh, prims, rays, 0.01, out=torch.zeros((n, 4), dtype=torch.float64, device="cuda"))):
        with pytest.raises(TypeError):
            call()
    for bad_radii in (radii[:-1], np.concatenate([radii, radii[:1]]), radii.reshape(-1, 2)):        # a wrong d_radii length
        with pytest.raises(ValueError):
            bvh_amd.sphere_cast(bvh, prims, rays, bad_radii)
    with pytest.raises(ValueError):
        bvh_amd.sphere_cast(bvh, prims, rays, 0.01, leaf="box")
