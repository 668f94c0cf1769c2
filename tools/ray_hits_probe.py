"""All-hits ray probe (bvh3X_intersect_rays_all_tri): one JSON line per pass.

    python tools/ray_hits_probe.py [--log2n 22] [--calls 7] [--robust]

The 1M-triangle soup (High tree built on the device), 2^log2n uniform rays (synth.rays_closest: origins in the scene box scaled 1.1x,
directions uniform on the sphere, tmax unbounded), as given (UNSORTED) and reordered (SORTED). Passes:
    count      bvh3X_intersect_rays_all_tri with d_counts only
    fill       the same entry point with the exact offsets of the count pass, records written
    closest    bvh3X_intersect_rays_tri on the same rays with the same flags: the yardstick from existing code. An all-hits walk cannot
               prune, so it is expected to be slower; how much slower is the number to learn.
The entry points are called directly on buffers allocated once, so a time is that of the library call (keys + sort included when
reordered), not of an allocation. Reported: median ms of --calls calls after two warm-up calls, timed with device events, clocks as
found; Mrays/s; Mhits/s (count and fill); mean and max list length; P and T = pair records fetched and primitives tested per ray
(a separate call with counters).
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
    args = ap.parse_args()
    import torch
    import bvh_amd
    from bvh_amd import _lib, synth
    torch.cuda.set_device(0)
    lib = _lib.load()
    stream = lambda: torch.cuda.current_stream().cuda_stream
    n = 1 << args.log2n
    raw, bvh, prims = scene("soup")
    lo, hi = synth.scene_bounds(raw)
    rays = torch.from_numpy(synth.rays_closest(n, lo, hi, seed=500 + args.log2n)).cuda()
    f_all, f_closest = lib.bvh3f_intersect_rays_all_tri, lib.bvh3f_intersect_rays_tri
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    closest = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(3, dtype=torch.int64, device="cuda")
    robust = 2 if args.robust else 0

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
    common = {"scene": "soup", "n": n, "robust": bool(args.robust), "mean_len": round(total / n, 3), "max_len": int(counts.max().item()),
              "rays_with_hits": round(float((counts > 0).double().mean()), 4)}

    def report(what, sort, ms, with_hits):
        c = cnt.cpu().numpy().astype(np.float64) / n
        line = dict(common, **{"pass": what, "sorted": sort, "ms": round(ms, 4), "mrays_per_s": round(n / ms / 1e3, 1),
                               "pairs_per_ray": round(float(c[0]), 2), "prims_per_ray": round(float(c[1]), 2)})
        if with_hits:
            line["mhits_per_s"] = round(total / ms / 1e3, 1)
        print(json.dumps(line), flush=True)

    for sort in (False, True):
        flags = 4 if sort else 16
        ms = timed(lambda: run_all(flags), args.calls)
        run_all(flags, counters=True)
        report("count", sort, ms, True)
        ms = timed(lambda: run_all(flags, offsets, hits), args.calls)
        run_all(flags, offsets, hits, counters=True)
        report("fill", sort, ms, True)
        ms = timed(lambda: run_closest(flags), args.calls)
        run_closest(flags, counters=True)
        report("closest", sort, ms, False)


if __name__ == "__main__":
    main()
