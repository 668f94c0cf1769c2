"""-m gpu: the ticket ranges of reordered launches on the device (csrc/traverse.hip: ticket_ranges_kernel, csrc/trace_body.inc: refill)
and the tail class of the reordering key (csrc/ray_key.h). Per-ray results never depend on the order rays are picked up in: for small
trees and batches of 65,536 rays (the smallest that takes eight ranges), 65,600 (no multiple of anything) and 2^18, with origins that
fill the prefixes evenly (uniform: the prefix boundaries are kept) and that do not (one cell, two prefixes, all outside the root box: the
equal slices are written instead), and with NaN rays, the hit records of the reordered launch — prefilled with a sentinel, chord classes
forced on and off — are byte-equal to those of the launch that traces the rays as given, and no record keeps the sentinel. The
persistent grid is forced (batches this small would otherwise take the one-shot grid, which draws no tickets)."""
import numpy as np
import pytest

from bvh_amd import synth

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


class _Scene:
    def __init__(self, n_tris):
        import torch
        import bvh_amd
        self.tris = synth.soup(n_tris)
        d_tris = torch.from_numpy(self.tris).cuda()
        bb, cc = bvh_amd.tri_bounds(d_tris)
        self.bvh = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.Medium))
        self.prims = bvh_amd.precompute_tris(d_tris, self.bvh.device_prim_ids())
        self.lo, self.hi = synth.scene_bounds(self.tris)


@pytest.fixture(scope="module")
def scenes():
    return {n: _Scene(n) for n in (2_000, 20_000)}


def _rays(kind, n, lo, hi, seed):
    rays = synth.rays_closest(n, lo, hi, seed=seed)
    rng = np.random.default_rng(seed)
    ext = hi - lo
    if kind == "one_cell":                                   # one cell of the 128^3 key grid: one prefix holds every ray
        rays[:, 0:3] = lo + (0.3 + rng.random((n, 3)) / 256) * ext
    elif kind == "two_prefixes":                             # two of the eight top-level cubes
        org = lo + rng.random((n, 3)) * 0.5 * ext
        org[n // 3:, :] += 0.5 * ext
        rays[:, 0:3] = org
    elif kind == "outside":                                  # beyond the root box on every axis, half of them pointing at it
        rays[:, 0:3] = hi + (0.05 + rng.random((n, 3))) * ext
        rays[::2, 3:6] = -np.abs(rays[::2, 3:6])
    elif kind == "nan":                                      # 1 % NaN: origins, directions, tmin, tmax
        idx = rng.choice(n, n // 100, replace=False)
        rays[idx[0::4], rng.integers(0, 3)] = np.nan
        rays[idx[1::4], 3 + rng.integers(0, 3)] = np.nan
        rays[idx[2::4], 6] = np.nan
        rays[idx[3::4], 7] = np.nan
    else:
        assert kind == "uniform"
    return rays


def _sentinel_out(n, dtype):
    import torch
    return torch.full((n, 4 * np.dtype(dtype).itemsize), SENTINEL, dtype=torch.uint8, device="cuda").view(torch.float32 if dtype == np.float32 else torch.float64)


def _check(bvh, prims, rays, dtype=np.float32, leaf="tri", classes=(0, 1)):
    import torch
    import bvh_amd
    lib = bvh_amd._lib.load()
    n = len(rays)
    d_rays = torch.from_numpy(rays).cuda()
    try:
        lib.bvh_amd_experiment(b"one_shot", 0)
        want = bvh_amd.intersect(bvh, prims, d_rays, robust=True, leaf=leaf, sort_rays=False, out=_sentinel_out(n, dtype)).cpu().numpy()
        sentinel = np.full(4 * np.dtype(dtype).itemsize, SENTINEL, dtype=np.uint8).tobytes()
        assert not (want.view(np.uint8).reshape(n, -1) == np.frombuffer(sentinel, dtype=np.uint8)).all(axis=1).any()
        for key_classes in classes:
            lib.bvh_amd_experiment(b"key_class_bits", key_classes)
            got = bvh_amd.intersect(bvh, prims, d_rays, robust=True, leaf=leaf, sort_rays=True, out=_sentinel_out(n, dtype)).cpu().numpy()
            assert bvh.dim == 2 or lib.bvh_amd_last_launch_reordered() == 1      # (a 2D launch is traced as given: the refill is what it shares)
            assert got.tobytes() == want.tobytes(), f"classes={key_classes}: the reordered launch's hit records differ"
    finally:
        lib.bvh_amd_experiment(b"reset", 0)
    return want


@pytest.mark.parametrize("kind", ["uniform", "one_cell", "two_prefixes", "outside", "nan"])
@pytest.mark.parametrize("n_tris,n_rays", [(2_000, 65_536), (20_000, 65_537 + 63), (20_000, 1 << 18)])
def test_reordered_launch_equals_the_launch_as_given(scenes, kind, n_tris, n_rays):
    s = scenes[n_tris]
    want = _check(s.bvh, s.prims, _rays(kind, n_rays, s.lo, s.hi, seed=n_rays % 1000 + len(kind)))
    if kind in ("uniform", "one_cell", "two_prefixes"):
        assert (want.view(np.uint32)[:, 0] != 0xFFFFFFFF).any()          # something was hit


def test_tail_thresholds_and_equal_slices_give_the_same_records(scenes):
    """The developer knobs around the default: tail class off, only the rays without a chord, a wide tail; ranges as equal slices."""
    import torch
    import bvh_amd
    lib = bvh_amd._lib.load()
    s = scenes[20_000]
    n = 65_600
    rays = _rays("uniform", n, s.lo, s.hi, seed=3)
    d_rays = torch.from_numpy(rays).cuda()
    try:
        lib.bvh_amd_experiment(b"one_shot", 0)
        want = bvh_amd.intersect(s.bvh, s.prims, d_rays, robust=True, sort_rays=False).cpu().numpy().tobytes()
        lib.bvh_amd_experiment(b"key_class_bits", 1)
        for knob, value in ((b"key_tail", 0), (b"key_tail_permille", 0), (b"key_tail_permille", 400), (b"range_align", 0)):
            lib.bvh_amd_experiment(knob, value)
            got = bvh_amd.intersect(s.bvh, s.prims, d_rays, robust=True, sort_rays=True, out=_sentinel_out(n, np.float32)).cpu().numpy().tobytes()
            assert got == want, (knob, value)
            lib.bvh_amd_experiment(knob, -1)
    finally:
        lib.bvh_amd_experiment(b"reset", 0)


def test_f64_triangles_share_the_refill():
    import torch
    import bvh_amd
    tris = synth.soup(5_000, dtype=np.float64)
    d_tris = torch.from_numpy(tris).cuda()
    bb, cc = bvh_amd.tri_bounds(d_tris)
    bvh = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.Medium))
    prims = bvh_amd.precompute_tris(d_tris, bvh.device_prim_ids())
    lo, hi = synth.scene_bounds(tris)
    _check(bvh, prims, synth.rays_closest(65_600, lo, hi, seed=9, dtype=np.float64), dtype=np.float64)


def test_2d_circles_share_the_refill():
    import torch
    import bvh_amd
    circ = synth.circles(5_000)
    bvh = bvh_amd.DefaultBuilder.build(*bvh_amd.sphere_bounds(torch.from_numpy(circ).cuda()))
    assert bvh.dim == 2
    prims = torch.from_numpy(np.ascontiguousarray(circ[bvh.prim_ids.astype(np.int64)])).cuda()
    _check(bvh, prims, synth.rays_2d(65_600, seed=10), leaf="sphere", classes=(1,))
