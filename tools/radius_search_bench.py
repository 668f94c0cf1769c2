"""Radius-query benchmark (bvh_amd.radius_count / radius_search): one JSON line per workload and pass.

    python tools/radius_search_bench.py [--scenes soup,terrain,spheres] [--log2n 24] [--calls 5] [--lengths 1,8,64] [--queries near]

Scenes: those of tools/closest_point_bench.py (1M-triangle soup, 1M-triangle terrain, 1M float64 spheres, High trees built on the
device). Queries: 2^log2n points near the surface (or uniform in the scene box). For each target mean list length the radius is found
by bisection on the mean count of the first 2^16 queries. Passes, each reordered and as given:
    count    bvhXX_radius_search_* with d_counts only
    fill     the same entry point with the exact offsets of the count pass, lists and distances written
    closest  bvhXX_closest_points_* at the same radius, for scale
The entry points are called directly on buffers allocated once, so a time is that of the library call (keys + sort included when
reordered), not of an allocation. Reported: median ms of --calls calls after two warm-up calls, timed with device events;
Mqueries/s; mean list length; P and T = pair records fetched and primitives tested per query (a separate call with counters); for
the fill pass also the list entries written per second. The offsets scan (bvh_amd_offsets_from_counts) is timed once per workload.
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

from closest_point_bench import queries, scene, timed  # noqa: E402


def find_radius(bvh, prims, sample, leaf, diag, target):
    """The radius at which the mean list length of `sample` is `target` (bisection; the mean grows with the radius)."""
    import bvh_amd
    lo, hi = 0.0, diag
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        mean = float(bvh_amd.radius_count(bvh, prims, sample, radius=mid, leaf=leaf).double().mean())
        if abs(mean - target) <= 0.02 * target:
            return mid
        lo, hi = (mid, hi) if mean < target else (lo, mid)
    return 0.5 * (lo + hi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="soup,terrain,spheres")
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--lengths", default="1,8,64")
    ap.add_argument("--queries", default="near", choices=["near", "uniform"])
    args = ap.parse_args()
    import torch
    import bvh_amd
    from bvh_amd import _lib, synth
    torch.cuda.set_device(0)
    lib = _lib.load()
    stream = lambda: torch.cuda.current_stream().cuda_stream
    n = 1 << args.log2n
    for name in args.scenes.split(","):
        raw, bvh, prims = scene(name)
        leaf = "sphere" if raw.shape[1] == 4 else "tri"
        dt = torch.float32 if raw.dtype == np.float32 else torch.float64
        lo, hi = synth.scene_bounds(raw)
        diag = float(np.linalg.norm(hi - lo))
        pts = torch.from_numpy(queries(raw, args.queries, n, seed=200 + args.log2n)).cuda()
        f_radius = getattr(lib, f"bvh{bvh._s}_radius_search_{leaf}")
        q = torch.empty((n, 4), dtype=dt, device="cuda")
        q[:, :3] = pts
        counts = torch.zeros(n, dtype=torch.int32, device="cuda")
        offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        hits = torch.empty((n, 4), dtype=dt, device="cuda")
        cnt = torch.zeros(3, dtype=torch.int64, device="cuda")
        for target in (float(x) for x in args.lengths.split(",")):
            r = find_radius(bvh, prims, pts[:1 << 16], leaf, diag, target)
            q[:, 3] = r

            def run(flags, offs=None, ids=None, dist=None, counters=False):
                _lib.check(f_radius(bvh._h, prims.data_ptr(), q.data_ptr(), n, flags, counts.data_ptr() if offs is None else None,
                                    None if offs is None else offs.data_ptr(), None if ids is None else ids.data_ptr(),
                                    None if dist is None else dist.data_ptr(), cnt.data_ptr() if counters else None, stream()), "radius_search")

            run(16)
            scan_ms = timed(lambda: _lib.check(lib.bvh_amd_offsets_from_counts(counts.data_ptr(), n, offsets.data_ptr(), stream()), "offsets"), args.calls)
            total = int(offsets[-1].item())
            ids = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")
            dist = torch.empty(max(total, 1), dtype=dt, device="cuda")
            common = {"scene": name, "queries": args.queries, "n": n, "target_len": target, "radius_over_diag": round(r / diag, 6),
                      "mean_len": round(total / n, 3), "max_len": int(counts.max().item()), "offsets_scan_ms": round(scan_ms, 4)}
            for sort in (True, False):
                flags = 4 if sort else 16
                for what in ("count", "fill", "closest"):
                    if what == "count":
                        ms = timed(lambda: run(flags), args.calls)
                        run(flags, counters=True)
                    elif what == "fill":
                        ms = timed(lambda: run(flags, offsets, ids, dist), args.calls)
                        run(flags, offsets, ids, dist, counters=True)
                    else:
                        ms = timed(lambda: bvh_amd.closest_points(bvh, prims, q, leaf=leaf, out=hits, sort_queries=sort), args.calls)
                        cnt.copy_(bvh_amd.closest_points(bvh, prims, q, leaf=leaf, out=hits, sort_queries=sort, counters=True)[1])
                    c = cnt.cpu().numpy().astype(np.float64) / n
                    line = dict(common, **{"pass": what, "sorted": sort, "ms": round(ms, 4), "mqueries_per_s": round(n / ms / 1e3, 1),
                                           "pairs_per_query": round(float(c[0]), 2), "prims_per_query": round(float(c[1]), 2),
                                           "leaves_per_query": round(float(c[2]), 2)})
                    if what == "fill":
                        line["mentries_per_s"] = round(total / ms / 1e3, 1)
                    print(json.dumps(line), flush=True)
            del ids, dist
            torch.cuda.empty_cache()
        del raw, bvh, prims, pts, q, counts, offsets, hits
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
