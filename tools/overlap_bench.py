"""Box-overlap benchmark (bvh3X_overlap_boxes / bvh3X_overlap_self): one JSON line per workload and pass.

    python tools/overlap_bench.py [--scenes soup,terrain,spheres] [--log2n 22] [--calls 5] [--lengths 1,8,64] [--queries near]

Scenes: those of tools/closest_point_bench.py (1M-triangle soup, 1M-triangle terrain, 1M float64 spheres, High trees built on the
device); the primitives' boxes are tri_bounds' / sphere_bounds'. Queries: 2^log2n cubes centred on points near the surface (or uniform
in the scene box). For each target mean list length the cubes' edge is found by bisection on the mean count of the first 2^16
queries. Passes, each reordered and as given:
    count         bvh3X_overlap_boxes with d_counts only
    fill          the same entry point with the exact offsets of the count pass, lists written
    radius_count  bvhXX_radius_search_* (d_counts only) on the cubes' centres, at the radius that gives the same mean list length:
                  the nearest existing path, for scale
and once per scene
    self_count / self_fill   bvh3X_overlap_self (never reordered).
The entry points are called directly on buffers allocated once, so a time is that of the library call (keys + sort included when
reordered), not of an allocation. Reported: median ms of --calls calls after two warm-up calls, timed with device events; Mqueries/s;
mean list length; P and T = pair records fetched and primitive boxes (radius_count: primitives) tested per query (a separate call
with counters); for the fill passes also the list entries written per second.
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


def boxes_around(pts, edge):
    import torch
    h = 0.5 * edge
    return torch.cat([pts - h, pts + h], dim=1).contiguous()


def find_edge(bvh, bboxes, sample, diag, target):
    """The edge at which the mean list length of cubes around `sample` is `target` (bisection; the mean grows with the edge)."""
    import bvh_amd
    lo, hi = 0.0, diag
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        mean = float(bvh_amd.overlap_count(bvh, bboxes, boxes_around(sample, mid)).double().mean())
        if abs(mean - target) <= 0.02 * target:
            return mid
        lo, hi = (mid, hi) if mean < target else (lo, mid)
    return 0.5 * (lo + hi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="soup,terrain,spheres")
    ap.add_argument("--log2n", type=int, default=22)
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
        bb, _ = bvh_amd.sphere_bounds(raw) if leaf == "sphere" else bvh_amd.tri_bounds(raw)
        lo, hi = synth.scene_bounds(raw)
        diag = float(np.linalg.norm(hi - lo))
        pts = torch.from_numpy(queries(raw, args.queries, n, seed=300 + args.log2n)).cuda()
        f_boxes = getattr(lib, f"bvh{bvh._s}_overlap_boxes")
        f_self = getattr(lib, f"bvh{bvh._s}_overlap_self")
        f_radius = getattr(lib, f"bvh{bvh._s}_radius_search_{leaf}")
        counts = torch.zeros(max(n, bvh.prim_count), dtype=torch.int32, device="cuda")
        offsets = torch.zeros(max(n, bvh.prim_count) + 1, dtype=torch.int64, device="cuda")
        cnt = torch.zeros(3, dtype=torch.int64, device="cuda")
        q4 = torch.empty((n, 4), dtype=dt, device="cuda")
        q4[:, :3] = pts

        def report(common, what, sort, ms, m, total=None):
            c = cnt.cpu().numpy().astype(np.float64) / m
            line = dict(common, **{"pass": what, "sorted": sort, "ms": round(ms, 4), "mqueries_per_s": round(m / ms / 1e3, 1),
                                   "pairs_per_query": round(float(c[0]), 2), "prims_per_query": round(float(c[1]), 2),
                                   "leaves_per_query": round(float(c[2]), 2)})
            if total is not None:
                line["mentries_per_s"] = round(total / ms / 1e3, 1)
            print(json.dumps(line), flush=True)

        # self mode
        def run_self(offs=None, ids=None, counters=False):
            _lib.check(f_self(bvh._h, bb.data_ptr(), bb.shape[0], 0, counts.data_ptr() if offs is None else None, None if offs is None else offs.data_ptr(),
                              None if ids is None else ids.data_ptr(), cnt.data_ptr() if counters else None, stream()), "overlap_self")

        m = bvh.prim_count
        run_self()
        _lib.check(lib.bvh_amd_offsets_from_counts(counts.data_ptr(), m, offsets.data_ptr(), stream()), "offsets")
        total = int(offsets[m].item())
        ids = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")
        common = {"scene": name, "n": m, "mean_len": round(total / m, 3), "max_len": int(counts[:m].max().item())}
        ms = timed(lambda: run_self(), args.calls)
        run_self(counters=True)
        report(common, "self_count", False, ms, m)
        ms = timed(lambda: run_self(offsets, ids), args.calls)
        run_self(offsets, ids, counters=True)
        report(common, "self_fill", False, ms, m, total)
        del ids

        for target in (float(x) for x in args.lengths.split(",")):
            edge = find_edge(bvh, bb, pts[:1 << 16], diag, target)
            q = boxes_around(pts, edge)
            r = find_radius(bvh, prims, pts[:1 << 16], leaf, diag, target)
            q4[:, 3] = r

            def run(flags, offs=None, ids=None, counters=False):
                _lib.check(f_boxes(bvh._h, bb.data_ptr(), bb.shape[0], q.data_ptr(), n, flags, counts.data_ptr() if offs is None else None,
                                   None if offs is None else offs.data_ptr(), None if ids is None else ids.data_ptr(),
                                   cnt.data_ptr() if counters else None, stream()), "overlap_boxes")

            def run_radius(flags, counters=False):
                _lib.check(f_radius(bvh._h, prims.data_ptr(), q4.data_ptr(), n, flags, counts.data_ptr(), None, None, None,
                                    cnt.data_ptr() if counters else None, stream()), "radius_search")

            run_radius(16)
            radius_mean = float(counts[:n].double().mean())
            run(16)
            _lib.check(lib.bvh_amd_offsets_from_counts(counts.data_ptr(), n, offsets.data_ptr(), stream()), "offsets")
            total = int(offsets[n].item())
            ids = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")
            common = {"scene": name, "queries": args.queries, "n": n, "target_len": target, "edge_over_diag": round(edge / diag, 6),
                      "radius_over_diag": round(r / diag, 6), "mean_len": round(total / n, 3), "radius_mean_len": round(radius_mean, 3),
                      "max_len": int(counts[:n].max().item())}
            for sort in (True, False):
                flags = 4 if sort else 16
                ms = timed(lambda: run(flags), args.calls)
                run(flags, counters=True)
                report(common, "count", sort, ms, n)
                ms = timed(lambda: run(flags, offsets, ids), args.calls)
                run(flags, offsets, ids, counters=True)
                report(common, "fill", sort, ms, n, total)
                ms = timed(lambda: run_radius(flags), args.calls)
                run_radius(flags, counters=True)
                report(common, "radius_count", sort, ms, n)
            del ids, q
            torch.cuda.empty_cache()
        del raw, bvh, prims, pts, q4, counts, offsets, bb
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
