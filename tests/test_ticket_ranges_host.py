"""CPU: the ticket ranges of a reordered launch and its reordering key, from the device's own text compiled for the host
(tests/cpp/ticket_ranges_host.cpp: bvh_amd/csrc/trace_body.inc with TraceArgs::range_starts, bvh_amd/csrc/ray_key.h).

Ranges: with explicit range starts every ray is traced exactly once — the golden hit records come out (a skipped ray leaves its record
untouched) and the visit counters equal those of one range drawn by one block (a ray traced twice raises them) — on grids of 1..9 blocks,
stagger on and off, for equal ranges, very unequal ones, empty ranges at the front, in the middle and at the end, n not a multiple of 64,
n below one wave, and starts that are no multiples of 64; in ticket order and through an order array.

Key: on random rays the order by key is prefix -> long -> short -> tail, the prefix and the cell bits are those of the key without
classes, and rays that miss the root box, NaN origins / directions and zero direction components land in the classes ray_key.h names."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
from conftest import ROOT, load_golden, parse_stream
from test_kernel_body_host import _aligned, _ptr, pair_records


def _compile(tmp_path_factory, name, extra):
    out = str(tmp_path_factory.mktemp(name) / f"lib{name}.so")
    src = os.path.join(ROOT, "tests", "cpp", "ticket_ranges_host.cpp")
    cmd = ["g++", "-std=c++20", "-O1", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-strict-aliasing", *extra, "-Wall", "-Wextra", "-Wno-unused-parameter",
           "-Wno-unknown-pragmas", "-Werror", "-shared", "-fPIC", src, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    dll = C.CDLL(out)
    dll.ticket_ranges_host_trace.restype = C.c_int
    dll.ticket_ranges_host_trace.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    dll.ticket_ranges_host_keys.restype = None
    dll.ticket_ranges_host_keys.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p]
    return dll


@pytest.fixture(scope="module")
def lane(tmp_path_factory):
    """one emulated lane per block"""
    return _compile(tmp_path_factory, "ranges1", [])


@pytest.fixture(scope="module")
def wave(tmp_path_factory):
    """a full wavefront of 64 fibers per block, the real refill / leaf thresholds"""
    return _compile(tmp_path_factory, "ranges64", ["-DBVH_HOST_WAVE64"])


@pytest.fixture(scope="module")
def scene(_restatement):
    g = load_golden("soup2k")
    nodes, ids = parse_stream(g["bvh_parallel_high"].tobytes(), False)
    prims = _aligned(np.ascontiguousarray(_restatement.precompute_tris(g["prims"], ids)))
    pairs = _aligned(pair_records(nodes["bounds"], nodes["index"]))
    rays = _aligned(np.ascontiguousarray(g["rays_closest"]))
    return {"pairs": pairs, "root": int(nodes["index"][0]) & 0xFFFFFFFF, "prims": prims, "rays": rays, "hits": g["hits_parallel_high_closest_robust"],
            "counters": g["counters_parallel_high_closest_robust"], "bounds": nodes["bounds"][0]}


def _trace(dll, s, n, parts, starts, order=None, blocks=1, stagger=0):
    hits = _aligned(np.full(n, 0xAB, dtype=np.uint8).repeat(oracle.HITF.itemsize).view(oracle.HITF))       # sentinel: a ray nobody traced keeps it
    cnt = np.zeros(3, dtype=np.uint64)
    st = None if starts is None else np.ascontiguousarray(starts, dtype=np.uint32)
    od = None if order is None else np.ascontiguousarray(order, dtype=np.uint32)
    dll.trace_body_host_set_grid(blocks, stagger)
    try:
        rc = dll.ticket_ranges_host_trace(_ptr(s["pairs"]), s["root"], _ptr(s["prims"]), _ptr(s["rays"]), n, parts, None if st is None else _ptr(st),
                                          None if od is None else _ptr(od), _ptr(hits), _ptr(cnt))
    finally:
        dll.trace_body_host_set_grid(1, 0)
    assert rc == 0
    return hits, cnt


def _range_cases(n):
    """name -> the 9 starts of 8 ranges over n tickets"""
    c = lambda v: [min(n, max(0, int(x))) for x in v]                                   # noqa: E731
    a, b = n // 3 + 1, (2 * n) // 3 + 7
    return {
        "equal": [p * n // 8 for p in range(9)],                                         # (no multiples of 64 unless n is one of 512)
        "unequal": sorted(c([0, 1, 3, n // 2, n // 2 + 5, n - 70, n - 3, n - 1, n])),
        "empty_front_middle_end": c([0, 0, 0, a, a, a, b, n, n]),
        "all_in_one": [0, 0, 0, 0, n, n, n, n, n],
        "first_takes_all": [0, n, n, n, n, n, n, n, n],
    }


def test_explicit_ranges_trace_every_ray_once(lane, wave, scene):
    full = len(scene["rays"])
    assert full >= 1000
    odd = full if full % 64 else full - 27
    rng = np.random.default_rng(5)
    # One emulated lane per block on every grid of 1..9 blocks: the whole golden batch, 600 rays (several waves, no multiple of 64) and
    # 37 (less than one wave). The 64-fiber wavefront — the real refill threshold: tickets drawn 54..64 at a time, so that a draw
    # straddles a range's end — on two grids (its emulated blocks cost 60 ms each to set up whatever they trace).
    every = tuple(range(1, 10))
    plans = {odd: ((lane, every),), 600: ((lane, every), (wave, (1, 3))), 37: ((lane, every), (wave, (2,)))}
    for n, harnesses in plans.items():
        assert n % 64 != 0
        want_hits = scene["hits"][:n].tobytes()
        _, want_cnt = _trace(lane, scene, n, 1, None)                                    # one range, one block, one lane
        if n == full:
            assert (want_cnt == scene["counters"]).all()
        order = rng.permutation(n)
        for name, starts in _range_cases(n).items():
            assert starts[0] == 0 and starts[8] == n and all(starts[p] <= starts[p + 1] for p in range(8)), (name, starts)
            for dll, grids in harnesses:
                for blocks in grids:
                    # (the wavefront: one run per grid — the stagger only where there is a second block to stop early)
                    for stagger in (0, 40) if dll is lane else ((40,) if blocks > 1 else (0,)):
                        for od in (None, order) if dll is lane else ((order,) if blocks == 1 else (None,)):
                            hits, cnt = _trace(dll, scene, n, 8, starts, od, blocks, stagger)
                            what = (n, name, blocks, stagger, od is not None)
                            assert hits.tobytes() == want_hits, what
                            assert (cnt == want_cnt).all(), what


def test_null_starts_are_equal_slices(lane, scene):
    """TraceArgs::range_starts == nullptr: the equal slices of part_size tickets, as before."""
    n = 1000
    _, want_cnt = _trace(lane, scene, n, 1, None)
    for blocks in (1, 8):
        hits, cnt = _trace(lane, scene, n, 8, None, None, blocks, 40)
        assert hits.tobytes() == scene["hits"][:n].tobytes()
        assert (cnt == want_cnt).all()


# ---- the key ------------------------------------------------------------------------------------------------------------------------

CELLS, CLASS_SCALE, TAIL = 128, 5.0, 0.05          # ray_keys_kernel's defaults: 7 bits per axis, long = chord >= 1 / 5 diagonal, tail = chord < 0.05 diagonal


def _keys(dll, rays, lo, hi, hilbert_bits, class_bits, tail):
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    lo3 = np.ascontiguousarray(lo, dtype=np.float32)
    sc3 = (np.float32(CELLS) / (np.asarray(hi, dtype=np.float32) - lo3)).astype(np.float32)
    keys = np.zeros(len(rays), dtype=np.uint32)
    dll.ticket_ranges_host_keys(_ptr(rays), len(rays), _ptr(lo3), _ptr(sc3), CELLS, hilbert_bits, class_bits, CLASS_SCALE, tail, _ptr(keys))
    return keys


def _chord_over_diagonal(rays, lo, hi):
    """float64: length of the part of the ray inside [lo, hi] between tmin and tmax, over the box diagonal (0 where it misses)."""
    r = rays.astype(np.float64)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    with np.errstate(all="ignore"):
        inv = 1.0 / r[:, 3:6]
        a, b = (lo - r[:, 0:3]) * inv, (hi - r[:, 0:3]) * inv
        t0 = np.fmax(r[:, 6], np.nanmax(np.where(np.isnan(a) | np.isnan(b), -np.inf, np.minimum(a, b)), axis=1))
        t1 = np.fmin(r[:, 7], np.nanmin(np.where(np.isnan(a) | np.isnan(b), np.inf, np.maximum(a, b)), axis=1))
        length = np.where(t1 > t0, t1 - t0, 0.0) * np.linalg.norm(r[:, 3:6], axis=1)
    return length / np.linalg.norm(hi - lo)


LONG, SHORT, TAIL_CLASS = 0, 1, 2


@pytest.mark.parametrize("hilbert_bits", [7, 0])
def test_key_orders_prefix_long_short_tail(lane, hilbert_bits):
    rng = np.random.default_rng(11)
    n = 20000
    lo, hi = np.array([-1.0, 2.0, 0.5]), np.array([3.0, 4.0, 6.5])
    c, h = (lo + hi) / 2, (hi - lo) / 2
    rays = np.zeros((n, 8), dtype=np.float32)
    rays[:, 0:3] = c + (rng.random((n, 3)) * 2 - 1) * 1.1 * h                           # origins in the 1.1x box, as the bench's
    d = rng.standard_normal((n, 3))
    rays[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 7] = np.finfo(np.float32).max
    rays[::9, 7] = rng.random(len(rays[::9])) * 2                                        # some short [tmin, tmax]
    rays[::50, 4] = 0.0                                                                  # zero direction components, both signs
    rays[25::50, 5] = -0.0
    plain = _keys(lane, rays, lo, hi, hilbert_bits, 0, -1.0)
    keys = _keys(lane, rays, lo, hi, hilbert_bits, 1, TAIL)
    old = _keys(lane, rays, lo, hi, hilbert_bits, 1, -1.0)                               # tail class off: one class bit, long / short
    assert (keys < (1 << 24)).all() and (plain < (1 << 24)).all()
    prefix, cls, low, octant = keys >> 21, (keys >> 19) & 3, (keys >> 3) & 0xFFFF, keys & 7
    assert (prefix == plain >> 21).all()                                                 # the three top bits of the cell index
    assert (low == ((plain >> 3) & 0x3FFFF) >> 2).all()                                  # the cell index gives up its two lowest bits
    assert (octant == (plain & 7)).all()
    assert (cls <= TAIL_CLASS).all()
    rel = _chord_over_diagonal(rays, lo, hi)
    sure = (np.abs(rel - 1 / CLASS_SCALE) > 1e-4) & (np.abs(rel - TAIL) > 1e-4)          # (the key divides approximately: not at the thresholds)
    want = np.where(rel >= 1 / CLASS_SCALE, LONG, np.where(rel >= TAIL, SHORT, TAIL_CLASS))
    assert (cls[sure] == want[sure]).all()
    for k in (LONG, SHORT, TAIL_CLASS):
        assert (want == k).sum() > n // 20                                               # every class is there
    assert (rel == 0).sum() > n // 20                                                    # and so are rays that miss the box
    # the order by key: prefix, then long -> short -> tail, then the rest of the cell index
    by_key = np.argsort(keys, kind="stable")
    rank = prefix[by_key].astype(np.int64) * 4 + cls[by_key]
    assert (np.diff(rank) >= 0).all()
    assert (np.diff(((prefix.astype(np.int64) * 4 + cls) << 16 | low)[by_key]) >= 0).all()
    # without the tail class: [prefix][1 class bit][17 cell bits], long exactly where it is long with the tail class
    assert ((old >> 21) == prefix).all() and ((((old >> 20) & 1) == 0) == (cls == LONG)).all()
    assert (((old >> 3) & 0x1FFFF) == ((plain >> 3) & 0x3FFFF) >> 1).all()
    # threshold 0: only rays with no chord at all are tail
    only_missers = (_keys(lane, rays, lo, hi, hilbert_bits, 1, 0.0) >> 19) & 3
    assert ((only_missers == TAIL_CLASS) == (rel == 0))[sure & ((rel == 0) | (rel > 1e-4))].all()


def test_key_classes_of_degenerate_rays(lane):
    lo, hi = np.array([0.0, 0.0, 0.0]), np.array([1.0, 1.0, 1.0])
    big, nan = np.finfo(np.float32).max, np.nan
    rays = np.array([
        [0.5, 0.5, 0.5, 1, 0, 0, 0, big],             # 0 inside, along x (two zero components): chord 0.5 -> long
        [0.5, 0.5, 0.5, 0, -0.0, 1, 0, 0.01],         # 1 inside, a short [tmin, tmax]: chord 0.01 -> tail
        [2.0, 0.5, 0.5, 1, 0, 0, 0, big],             # 2 outside, pointing away: misses -> tail
        [2.0, 0.5, 0.5, 0, 1, 0, 0, big],             # 3 outside along an axis its direction does not move on: misses -> tail
        [-1.0, 0.5, 0.5, 1, 0, 0, 0, big],            # 4 outside, through the box: chord 1 -> long
        [0.5, 0.5, 0.5, 1, 0, 0, 1, 0.5],             # 5 tmax < tmin: empty -> tail
        [nan, 0.5, 0.5, 1, 0, 0, 0, big],             # 6 NaN origin component: that slab does not clip, chord 0.5 from y / z ... x clips nothing -> long
        [nan, nan, nan, 0.6, 0.0, 0.8, 0, big],       # 7 NaN origin: nothing clips, [tmin, tmax] itself -> long
        [0.5, 0.5, 0.5, nan, 0, 1, 0, big],           # 8 NaN direction component: the length is NaN -> tail
        [0.5, 0.5, 0.5, nan, nan, nan, 0, big],       # 9 NaN direction -> tail
        [0.5, 0.5, 0.5, 0, 0, 0, 0, big],             # 10 zero direction: length 0 -> tail
        [0.5, 0.5, 0.5, 1, 0, 0, nan, big],           # 11 NaN tmin: nothing compares greater than it, no chord -> tail
        [0.5, 0.5, 0.5, 1, 0, 0, 0, nan],             # 12 NaN tmax: the same -> tail
        [0.9, 0.5, 0.5, 1, 0, 0, 0, big],             # 13 chord 0.1 of a diagonal of 1.73: 0.058 -> short
    ], dtype=np.float32)
    want = [LONG, TAIL_CLASS, TAIL_CLASS, TAIL_CLASS, LONG, TAIL_CLASS, LONG, LONG, TAIL_CLASS, TAIL_CLASS, TAIL_CLASS, TAIL_CLASS, TAIL_CLASS, SHORT]
    for hilbert_bits in (7, 0):
        keys = _keys(lane, rays, lo, hi, hilbert_bits, 1, TAIL)
        assert (keys < (1 << 24)).all()
        assert ((keys >> 19) & 3).tolist() == want
        assert (keys[6:8] >> 21 == _keys(lane, rays[6:8], lo, hi, hilbert_bits, 0, -1.0) >> 21).all()      # NaN origins: cell 0 along that axis, as without classes
