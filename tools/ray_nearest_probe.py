"""Nearest-hits ray probe (bvh3X_intersect_rays_nearest_tri): one JSON line per pass.

    python tools/ray_nearest_probe.py [--log2n 22] [--calls 7] [--robust] [--ks 1,4,8,16]

The 1M-triangle soup (High tree built on the device) and the rays of tools/ray_hits_probe.py (synth.rays_closest, the same seed),
as given (UNSORTED) and reordered (SORTED). Passes:
    nearest    bvh3X_intersect_rays_nearest_tri at each k of --ks: rows and counts written
    closest    bvh3X_intersect_rays_tri on the same rays with the same flags: the floor, a walk that keeps one candidate
    all+sort   what a caller had before this entry point: bvh3X_intersect_rays_all_tri count pass, bvh_amd_offsets_from_counts, fill pass,
               then a segmented sort of the records by t on the device (two stable torch sorts: by t, then by ray; ties in t are left in
               walk order, which is less than the (t, prim) order the new call gives) and the gather of the records. The parts are
               reported beside the sum. Buffers are sized once, outside the timing; the ray index of every record
               (repeat_interleave) is part of the sort's time, since it depends on the counts.
The entry points are called directly on buffers allocated once, so a time is that of the library call (keys + sort included when
reordered), not of an allocation. Reported: median ms of --calls calls after two warm-up calls, timed with device events, clocks as
found; Mrays/s; P, T, L = pair records fetched, primitives tested and leaves visited per ray (a separate call with counters).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from closest_point_bench import scene, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=22)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--robust", action="store_true")
    ap.add_argument("--ks", default="1,4,8,16")
    args = ap.parse_args()
    import torch
    from bvh_amd import _lib, synth
    torch.cuda.set_device(0)
    lib = _lib.load()
    stream = lambda: torch.cuda.current_stream().cuda_stream
    n = 1 << args.log2n
    ks = [int(k) for k in args.ks.split(",")]
    raw, bvh, prims = scene("soup")
    lo, hi = synth.scene_bounds(raw)
    rays = torch.from_numpy(synth.rays_closest(n, lo, hi, seed=500 + args.log2n)).cuda()
    f_near, f_all, f_closest = lib.bvh3f_intersect_rays_nearest_tri, lib.bvh3f_intersect_rays_all_tri, lib.bvh3f_intersect_rays_tri
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    closest = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    rows = torch.empty((n, max(ks), 4), dtype=torch.float32, device="cuda")
    row_counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(3, dtype=torch.int64, device="cuda")
    ray_ids = torch.arange(n, dtype=torch.int64, device="cuda")
    robust = 2 if args.robust else 0

    def run_nearest(k, flags, counters=False):
        _lib.check(f_near(bvh._h, prims.data_ptr(), rays.data_ptr(), n, k, flags | robust, rows.data_ptr(), row_counts.data_ptr(),
                          cnt.data_ptr() if counters else None, stream()), "intersect_rays_nearest")

    def run_all(flags, offs=None, hits=None, counters=False):
        _lib.check(f_all(bvh._h, prims.data_ptr(), rays.data_ptr(), n, flags | robust, counts.data_ptr() if offs is None else None,
                         None if offs is None else offs.data_ptr(), None if hits is None else hits.data_ptr(), cnt.data_ptr() if counters else None, stream()),
                   "intersect_rays_all")

    def run_closest(flags, counters=False):
        _lib.check(f_closest(bvh._h, prims.data_ptr(), rays.data_ptr(), n, flags | robust, closest.data_ptr(), cnt.data_ptr() if counters else None, stream()),
                   "intersect_rays")

    run_all(16)
    _lib.check(lib.bvh_amd_offsets_from_counts(counts.data_ptr(), n, offsets.data_ptr(), stream()), "offsets")
    total = int(offsets[n].item())
    hits = torch.empty((max(total, 1), 4), dtype=torch.float32, device="cuda")
    common = {"scene": "soup", "n": n, "robust": bool(args.robust), "mean_len": round(total / n, 3), "max_len": int(counts.max().item())}

    def segmented_sort():
        seg = torch.repeat_interleave(ray_ids, counts.to(torch.int64), output_size=total)
        by_t = torch.sort(hits[:total, 1], stable=True).indices
        by_ray = torch.sort(seg[by_t], stable=True).indices
        return hits[:total][by_t[by_ray]]

    def caller_path(flags):
        run_all(flags)
        _lib.check(lib.bvh_amd_offsets_from_counts(counts.data_ptr(), n, offsets.data_ptr(), stream()), "offsets")
        run_all(flags, offsets, hits)
        return segmented_sort()

    def report(what, sort, ms, **more):
        c = cnt.cpu().numpy().astype(np.float64) / n
        line = dict(common, **{"pass": what, "sorted": sort, "ms": round(ms, 4), "mrays_per_s": round(n / ms / 1e3, 1),
                               "pairs_per_ray": round(float(c[0]), 2), "prims_per_ray": round(float(c[1]), 2), "leaves_per_ray": round(float(c[2]), 2)}, **more)
        print(json.dumps(line), flush=True)

    for sort in (False, True):
        flags = 4 if sort else 16
        for k in ks:
            ms = timed(lambda: run_nearest(k, flags), args.calls)
            run_nearest(k, flags, counters=True)
            report("nearest", sort, ms, k=k, full_rows=round(float((row_counts == k).double().mean()), 4))
        ms = timed(lambda: run_closest(flags), args.calls)
        run_closest(flags, counters=True)
        report("closest", sort, ms)
        ms_count = timed(lambda: run_all(flags), args.calls)
        ms_fill = timed(lambda: run_all(flags, offsets, hits), args.calls)
        ms_sort = timed(segmented_sort, args.calls)
        ms = timed(lambda: caller_path(flags), args.calls)
        run_all(flags, offsets, hits, counters=True)
        report("all+sort", sort, ms, ms_count=round(ms_count, 4), ms_fill=round(ms_fill, 4), ms_segmented_sort=round(ms_sort, 4))


if __name__ == "__main__":
    main()
