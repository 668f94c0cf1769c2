"""-m gpu: the order sort of reordered ray / query batches (csrc/sort_emul.hip: radix_sort_order — keys narrowed to u16 / u8 between the
radix passes, the histogram scanned by one launch of a block per digit), through bvh_amd_radix_order_u32: the first histogram by a
key kernel, positions as values, narrow carry, keys dropped, exactly as launch_planned and query_order run it.

The order must be numpy's stable argsort bit for bit. Sizes: one key, below / at / above a wave, a last tile with one key (4097: the
general sort's tile, 8193: this sort's), one tile exactly and one short of it, several tiles with a ragged end, 2^17 + 5. Key widths: one
pass (3, 8), every hand-over of key types (9 and 16: u32 -> u8; 17 and 24: u32 -> u16 -> u8; 25 and 32: u32 -> u32 -> u16 -> u8). Keys:
random; all equal (255 digits empty in every tile, one digit holding every tile whole); one value per tile; descending; only the top
digit varying; only the bottom digit varying.

Then the two callers end to end: closest-hit rays and closest-point queries, reordered against as given, byte-equal records."""
import numpy as np
import pytest

from bvh_amd import synth

pytestmark = pytest.mark.gpu

TILE = 8192
SIZES = (1, 63, 64, 4097, 8191, 8192, 8193, 3 * 8192 + 17, (1 << 17) + 5)
BITS = (3, 8, 9, 16, 17, 24, 25, 32)


def _key_sets(n, bits, rng):
    mask = (1 << bits) - 1
    passes = (bits + 7) // 8
    top_shift = 8 * (passes - 1)
    i = np.arange(n, dtype=np.uint64)
    fixed = 0x5A5A5A5A & mask
    return {
        "random": rng.integers(0, mask + 1, n, dtype=np.uint64),
        "all_equal": np.full(n, fixed, dtype=np.uint64),
        "one_per_tile": ((i // TILE + 1) * 0x9E3779B1) & mask,
        "descending": mask - (i * (mask + 1)) // n,
        "top_digit": (rng.integers(0, (mask >> top_shift) + 1, n, dtype=np.uint64) << top_shift) | (fixed & ((1 << top_shift) - 1)),
        "bottom_digit": (fixed & ~0xFF) | rng.integers(0, min(mask, 0xFF) + 1, n, dtype=np.uint64),
    }


@pytest.mark.parametrize("bits", BITS)
def test_order_is_the_stable_argsort(bits):
    import bvh_amd
    rng = np.random.default_rng(100 + bits)
    for n in SIZES:
        for name, k64 in _key_sets(n, bits, rng).items():
            assert k64.max() < (1 << bits), (name, n, bits)
            keys = k64.astype(np.uint32)
            got = bvh_amd.radix_order(keys.view(np.int32), bits).cpu().numpy().view(np.uint32)
            want = np.argsort(keys, kind="stable").astype(np.uint32)
            assert got.tobytes() == want.tobytes(), (name, n, bits)


def test_key_sets_hit_what_they_are_built_for():
    """(no device work) a descending set really descends, one_per_tile leaves digits empty everywhere and fills one per tile."""
    rng = np.random.default_rng(1)
    sets = _key_sets(3 * TILE + 17, 24, rng)
    assert (np.diff(sets["descending"].astype(np.int64)) <= 0).all() and sets["descending"][0] > sets["descending"][-1]
    per_tile = sets["one_per_tile"][: 3 * TILE].reshape(3, TILE)
    assert (per_tile == per_tile[:, :1]).all() and len(set(per_tile[:, 0].tolist())) == 3
    assert len(np.unique(sets["top_digit"] & 0xFFFF)) == 1 and len(np.unique(sets["top_digit"] >> 16)) > 100
    assert len(np.unique(sets["bottom_digit"] >> 8)) == 1 and len(np.unique(sets["bottom_digit"] & 0xFF)) == 256


@pytest.fixture(scope="module")
def soup():
    import torch
    import bvh_amd

    class S:
        pass
    s = S()
    s.tris = synth.soup(20_000)
    d_tris = torch.from_numpy(s.tris).cuda()
    bb, cc = bvh_amd.tri_bounds(d_tris)
    s.bvh = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.Medium))
    s.prims = bvh_amd.precompute_tris(d_tris, s.bvh.device_prim_ids())
    s.lo, s.hi = synth.scene_bounds(s.tris)
    return s


def test_reordered_rays_give_the_hits_of_the_rays_as_given(soup):
    import torch
    import bvh_amd
    lib = bvh_amd._lib.load()
    n = 70_001
    d_rays = torch.from_numpy(synth.rays_closest(n, soup.lo, soup.hi, seed=21)).cuda()
    want = bvh_amd.intersect(soup.bvh, soup.prims, d_rays, robust=True, sort_rays=False).cpu().numpy()
    assert (want.view(np.uint32)[:, 0] != 0xFFFFFFFF).any()
    got = bvh_amd.intersect(soup.bvh, soup.prims, d_rays, robust=True, sort_rays=True).cpu().numpy()
    assert lib.bvh_amd_last_launch_reordered() == 1
    assert got.tobytes() == want.tobytes()
    try:
        lib.bvh_amd_experiment(b"key_class_bits", 1)
        again = bvh_amd.intersect(soup.bvh, soup.prims, d_rays, robust=True, sort_rays=True).cpu().numpy()
        assert lib.bvh_amd_last_launch_reordered() == 1
        assert again.tobytes() == want.tobytes()
    finally:
        lib.bvh_amd_experiment(b"reset", 0)


def test_reordered_closest_points_give_the_records_of_the_queries_as_given(soup):
    import torch
    import bvh_amd
    n = 70_001
    rng = np.random.default_rng(22)
    pts = (soup.lo + rng.random((n, 3)) * (soup.hi - soup.lo)).astype(np.float32)
    d_pts = torch.from_numpy(pts).cuda()
    want = bvh_amd.closest_points(soup.bvh, soup.prims, d_pts, sort_queries=False).cpu().numpy()
    assert (want.view(np.uint32)[:, 0] != 0xFFFFFFFF).all()
    got = bvh_amd.closest_points(soup.bvh, soup.prims, d_pts, sort_queries=True).cpu().numpy()
    assert got.tobytes() == want.tobytes()
