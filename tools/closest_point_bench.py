"""Closest-point query benchmark (bvh_amd.closest_points): one JSON line per workload.

    python tools/closest_point_bench.py [--scenes soup,terrain,spheres] [--log2n 24] [--calls 10] [--cpu]

Scenes: the 1M-triangle soup with a High tree built on the device (bench.py's scene), the 1M-triangle terrain (High), 1M float64
spheres (High). Queries: 2^log2n uniform in the scene box (1.1x) and near-surface (a random point of a random primitive plus a normal
offset of 1 % of the box), radius inf and 0.01 x diagonal, reordered and as given; then 2^16 and 2^20 uniform queries, radius inf,
reordered and as given (the reordering threshold). Reported: median ms of --calls calls after two warm-up calls, timed with device
events around the whole call (keys + sort included when reordered); Mqueries/s; P and T = pair records fetched and primitives tested
per query, from a separate call with counters; the modelled bytes per query (query + P records + T primitives + record:
f32 triangles 16 + 64 P + 48 T + 16, f64 spheres 32 + 128 P + 32 T + 32). --cpu adds the host harness (tests/cpp/closest_body_host.cpp,
the kernel's own text compiled by g++) on 16 threads over 2^16 queries of each scene as a CPU baseline.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene(name):
    import bvh_amd
    from bvh_amd import synth
    if name == "spheres":
        raw = synth.spheres(1 << 20)
        bb, cc = bvh_amd.sphere_bounds(raw)
    else:
        raw = synth.soup(1 << 20) if name == "soup" else synth.terrain(1 << 20)
        bb, cc = bvh_amd.tri_bounds(raw)
    bvh = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.High))
    prims = bvh_amd.gather(raw, bvh.device_prim_ids()) if name == "spheres" else bvh_amd.precompute_tris(raw, bvh.device_prim_ids())
    return raw, bvh, prims


def queries(raw, kind, n, seed):
    from bvh_amd import synth
    lo, hi = synth.scene_bounds(raw)
    sigma = 0.01 * float(np.max(hi - lo))
    if kind == "uniform":
        return synth.points_uniform(n, lo, hi, seed=seed, dtype=raw.dtype)
    if raw.shape[1] == 9:
        return synth.points_near_surface(raw, n, seed=seed, sigma=sigma)
    # spheres: a random point of a random sphere's surface plus the same isotropic offset
    pick = (synth.splitmix64(seed, n, 0) % np.uint64(len(raw))).astype(np.int64)
    g = synth.uniform01(seed, 3 * n, 1).reshape(n, 3) * 2 - 1
    d = g / np.maximum(np.linalg.norm(g, axis=1, keepdims=True), 1e-12)
    off = (synth.uniform01(seed, 3 * n, 2).reshape(n, 3) * 2 - 1) * sigma
    return (raw[pick, :3] + raw[pick, 3:4] * d + off).astype(raw.dtype)


def timed(fn, calls):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="soup,terrain,spheres")
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--cpu", action="store_true")
    args = ap.parse_args()
    import torch
    import bvh_amd
    torch.cuda.set_device(0)
    for name in args.scenes.split(","):
        raw, bvh, prims = scene(name)
        leaf = "sphere" if raw.shape[1] == 4 else "tri"
        dt = torch.float32 if raw.dtype == np.float32 else torch.float64
        from bvh_amd import synth
        lo, hi = synth.scene_bounds(raw)
        diag = float(np.linalg.norm(hi - lo))
        work = [(kind, args.log2n, r, s) for kind in ("uniform", "near") for r in ("inf", "0.01diag") for s in (True, False)]
        work += [("uniform", k, "inf", s) for k in (16, 20) for s in (True, False)]
        cache = {}
        for kind, log2n, rname, sort in work:
            n = 1 << log2n
            if (kind, n) not in cache:
                cache.clear()
                cache[(kind, n)] = torch.from_numpy(queries(raw, kind, n, seed=100 + log2n)).cuda()
            pts = cache[(kind, n)]
            r = float("inf") if rname == "inf" else 0.01 * diag
            q = torch.empty((n, 4), dtype=dt, device="cuda")
            q[:, :3] = pts
            q[:, 3] = r
            out = torch.empty((n, 4), dtype=dt, device="cuda")
            ms = timed(lambda: bvh_amd.closest_points(bvh, prims, q, leaf=leaf, out=out, sort_queries=sort), args.calls)
            _, cnt = bvh_amd.closest_points(bvh, prims, q, leaf=leaf, counters=True, sort_queries=sort)
            c = cnt.cpu().numpy().astype(np.float64) / n
            hits = bvh_amd.hits_to_numpy(out)
            if leaf == "tri":
                model = 16 + 64 * c[0] + 48 * c[1] + 16
            else:
                model = 32 + 128 * c[0] + 32 * c[1] + 32
            print(json.dumps({"scene": name, "queries": kind, "n": n, "radius": rname, "sorted": sort, "ms": round(ms, 4),
                              "mqueries_per_s": round(n / ms / 1e3, 1), "pairs_per_query": round(float(c[0]), 2),
                              "prims_per_query": round(float(c[1]), 2), "leaves_per_query": round(float(c[2]), 2),
                              "hit_fraction": round(float((hits["prim"] != bvh_amd.INVALID).mean()), 4),
                              "model_bytes_per_query": round(float(model), 1),
                              "model_gb_per_s": round(float(model) * n / ms / 1e6, 1)}), flush=True)
        if args.cpu:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import tempfile
            from test_closest_point_host import compile_harness, host_walk
            dll = compile_harness(tempfile.mkdtemp())
            n = 1 << 16
            pts = queries(raw, "uniform", n, seed=7)
            q = np.zeros((n, 4), dtype=raw.dtype)
            q[:, :3] = pts
            q[:, 3] = np.inf
            nodes = bvh.nodes
            p = prims.cpu().numpy()
            t0 = time.perf_counter()
            host_walk(dll, nodes["bounds"], nodes["index"], p, q, 1 if leaf == "sphere" else 0, threads=16)
            s = time.perf_counter() - t0
            print(json.dumps({"scene": name, "queries": "uniform", "n": n, "radius": "inf", "cpu_threads": 16, "ms": round(1e3 * s, 2),
                              "mqueries_per_s": round(n / s / 1e6, 2)}), flush=True)
        del raw, bvh, prims, cache
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
