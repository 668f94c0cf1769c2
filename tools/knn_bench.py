"""k-nearest benchmark (bvh_amd.knn / bvhXX_knn_*): one JSON line per workload.

    python tools/knn_bench.py [--scenes soup,spheres] [--log2n 22] [--calls 5] [--ks 1,8,16,32,64] [--queries uniform,near]

Scenes: those of tools/closest_point_bench.py (1M-triangle soup in float32, 1M float64 spheres; High trees built on the device).
Queries: 2^log2n points uniform in the scene box, and as many near the surface; unbounded (max_distance = inf). Per scene and kind
of query, each reordered and as given:
    knn      bvhXX_knn_* for every k, ids + distances + counts written
    closest  bvhXX_closest_points_* on the same queries: the k = 1 baseline (the same walk without the candidate set)
    radius   for k = 8 and 32, what a caller without knn does: bvhXX_radius_search_* at the radius that gives a mean list of 2k (found
             by bisection on the first 2^16 queries), count pass + fill pass. The host-side sort of each list is NOT included: the sum
             of the two kernel times is a lower bound of the emulation.
The entry points are called directly on buffers allocated once, so a time is that of the library call (keys + sort included when
reordered), not of an allocation. Reported: median ms of --calls calls after two warm-up calls, timed with device events;
Mqueries/s; P, T, L = pair records fetched, primitives tested and leaves visited per query (a separate call with counters).
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
from radius_search_bench import find_radius  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="soup,spheres")
    ap.add_argument("--log2n", type=int, default=22)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--ks", default="1,8,16,32,64")
    ap.add_argument("--queries", default="uniform,near")
    ap.add_argument("--no-baselines", action="store_true")
    args = ap.parse_args()
    import torch
    import bvh_amd
    from bvh_amd import _lib, synth
    torch.cuda.set_device(0)
    lib = _lib.load()
    stream = lambda: torch.cuda.current_stream().cuda_stream
    n = 1 << args.log2n
    ks = [int(x) for x in args.ks.split(",")]
    for name in args.scenes.split(","):
        raw, bvh, prims = scene(name)
        leaf = "sphere" if raw.shape[1] == 4 else "tri"
        dt = torch.float32 if raw.dtype == np.float32 else torch.float64
        lo, hi = synth.scene_bounds(raw)
        diag = float(np.linalg.norm(hi - lo))
        f_knn = getattr(lib, f"bvh{bvh._s}_knn_{leaf}")
        f_radius = getattr(lib, f"bvh{bvh._s}_radius_search_{leaf}")
        q = torch.empty((n, 4), dtype=dt, device="cuda")
        ids = torch.empty(n * max(ks), dtype=torch.int32, device="cuda")
        dist = torch.empty(n * max(ks), dtype=dt, device="cuda")
        counts = torch.zeros(n, dtype=torch.int32, device="cuda")
        offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        hits = torch.empty((n, 4), dtype=dt, device="cuda")
        cnt = torch.zeros(3, dtype=torch.int64, device="cuda")

        def emit(common, what, ms, **extra):
            c = cnt.cpu().numpy().astype(np.float64) / n
            print(json.dumps(dict(common, **{"pass": what, "ms": round(ms, 4), "mqueries_per_s": round(n / ms / 1e3, 1), "pairs_per_query": round(float(c[0]), 2),
                                             "prims_per_query": round(float(c[1]), 2), "leaves_per_query": round(float(c[2]), 2)}, **extra)), flush=True)

        for kind in args.queries.split(","):
            q[:, :3] = torch.from_numpy(queries(raw, kind, n, seed=300 + args.log2n)).cuda()
            for sort in (True, False):
                flags = 4 if sort else 16
                common = {"scene": name, "queries": kind, "n": n, "sorted": sort}
                q[:, 3] = float("inf")
                for k in ks:
                    def run(counters=False):
                        _lib.check(f_knn(bvh._h, prims.data_ptr(), q.data_ptr(), n, k, flags, ids.data_ptr(), dist.data_ptr(), counts.data_ptr(),
                                         cnt.data_ptr() if counters else None, stream()), "knn")
                    ms = timed(run, args.calls)
                    run(counters=True)
                    emit(common, "knn", ms, k=k)
                if args.no_baselines:
                    continue
                ms = timed(lambda: bvh_amd.closest_points(bvh, prims, q, leaf=leaf, out=hits, sort_queries=sort), args.calls)
                cnt.copy_(bvh_amd.closest_points(bvh, prims, q, leaf=leaf, out=hits, sort_queries=sort, counters=True)[1])
                emit(common, "closest", ms, k=1)
                for k in (8, 32):
                    if k not in ks:
                        continue
                    r = find_radius(bvh, prims, q[:1 << 16, :3].contiguous(), leaf, diag, 2.0 * k)
                    q[:, 3] = r

                    def radius(offs=None, lst=None, dst=None, counters=False):
                        _lib.check(f_radius(bvh._h, prims.data_ptr(), q.data_ptr(), n, flags, counts.data_ptr() if offs is None else None,
                                            None if offs is None else offs.data_ptr(), None if lst is None else lst.data_ptr(),
                                            None if dst is None else dst.data_ptr(), cnt.data_ptr() if counters else None, stream()), "radius_search")
                    count_ms = timed(radius, args.calls)
                    _lib.check(lib.bvh_amd_offsets_from_counts(counts.data_ptr(), n, offsets.data_ptr(), stream()), "offsets")
                    total = int(offsets[-1].item())
                    short = float((counts < k).double().mean())
                    lst = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")
                    dst = torch.empty(max(total, 1), dtype=dt, device="cuda")
                    fill_ms = timed(lambda: radius(offsets, lst, dst), args.calls)
                    radius(offsets, lst, dst, counters=True)
                    emit(common, "radius", count_ms + fill_ms, k=k, count_ms=round(count_ms, 4), fill_ms=round(fill_ms, 4), radius_over_diag=round(r / diag, 6),
                         mean_len=round(total / n, 3), lists_shorter_than_k=round(short, 4))
                    del lst, dst
                    torch.cuda.empty_cache()
        del raw, bvh, prims, q, ids, dist, counts, offsets, hits
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
