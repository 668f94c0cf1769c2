"""Times the winding-number queries ("Winding numbers").

    python tools/bench_winding.py [--queries 4194304] [--stacks 512] [--soup 1048576] [--calls 20] [--warmup 3] [--json PATH]

Scenes: a closed UV sphere of 2 * stacks columns (512: 1 046 528 triangles) and synth.soup(--soup). Per scene:
  prepare:   bvh_amd.winding_prepare (the parents pass, the leaf fold and the climb; the output buffer reused);
  winding:   bvh_amd.winding_numbers at beta = 2 and beta = 3 over --queries points uniform in the scene's box scaled 1.5, the batch
             reordered inside the call as the library decides (the reorder is inside the timed pass), with the counters per query from
             one extra call;
  closest:   bvh_amd.closest_points on the same queries, as the yardstick.
Each figure is the median of `calls` calls after `warmup` warm-ups, timed with events on the call's stream. Needs the GPU; prints one
JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(torch, fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    return {"median": float(np.median(times)), "min": float(np.min(times)), "max": float(np.max(times))}


def uv_sphere(stacks, slices):
    """slices * (2 + 2 * (stacks - 2)) triangles with (p1 - p0) x (p2 - p0) outward, float32."""
    th = np.pi * np.arange(stacks + 1) / stacks
    ph = 2 * np.pi * (np.arange(slices + 1) % slices) / slices
    grid = np.stack([np.sin(th)[:, None] * np.cos(ph)[None, :], np.sin(th)[:, None] * np.sin(ph)[None, :],
                     np.broadcast_to(np.cos(th)[:, None], (stacks + 1, slices + 1))], axis=-1)
    a, b, c, d = grid[:-1, :-1], grid[1:, :-1], grid[1:, 1:], grid[:-1, 1:]
    upper = np.stack([a, b, c], axis=2)[:-1].reshape(-1, 9)      # (the last band's b = c = the south pole: degenerate, left out)
    lower = np.stack([a, c, d], axis=2)[1:].reshape(-1, 9)       # (the first band's a = d = the north pole: likewise)
    return np.ascontiguousarray(np.concatenate([upper, lower]).astype(np.float32))


def measure(torch, bvh_amd, name, tris, n_queries, calls, warmup):
    d_tris = torch.from_numpy(tris).cuda()
    bb, cc = bvh_amd.tri_bounds(d_tris)
    bvh = bvh_amd.DefaultBuilder.build(bb, cc)
    prims = bvh_amd.precompute_tris(d_tris, bvh.device_prim_ids())
    moments = bvh_amd.winding_prepare(bvh, prims)
    out = {"scene": name, "triangles": int(len(tris)), "nodes": int(bvh.node_count),
           "winding_prepare_ms": median_ms(torch, lambda: bvh_amd.winding_prepare(bvh, prims, out=moments), calls, warmup)}
    v = tris.reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    mid, half = (lo + hi) / 2, (hi - lo) / 2 * 1.5
    pts = (mid + (np.random.default_rng(5).random((n_queries, 3)) * 2 - 1) * half).astype(np.float32)
    q = torch.empty((n_queries, 4), dtype=torch.float32, device="cuda")
    q[:, :3] = torch.from_numpy(pts).cuda()
    q[:, 3] = float("inf")
    w = torch.empty(n_queries, dtype=torch.float32, device="cuda")
    hits = torch.empty((n_queries, 4), dtype=torch.float32, device="cuda")
    for beta in (2.0, 3.0):
        _, cnt = bvh_amd.winding_numbers(bvh, prims, moments, q, beta=beta, counters=True)
        cnt = cnt.cpu().numpy() / n_queries
        t = median_ms(torch, lambda: bvh_amd.winding_numbers(bvh, prims, moments, q, beta=beta, out=w), calls, warmup)
        out[f"winding_numbers_beta{beta:g}_ms"] = t
        out[f"winding_numbers_beta{beta:g}_mqueries_per_s"] = n_queries / t["median"] / 1e3
        out[f"winding_numbers_beta{beta:g}_per_query"] = {"pair_records": float(cnt[0]), "triangles": float(cnt[1]), "far_terms": float(cnt[2])}
        out[f"winding_numbers_beta{beta:g}_inside_fraction"] = float((w >= 0.5).float().mean().item())
    t = median_ms(torch, lambda: bvh_amd.closest_points(bvh, prims, q, out=hits), calls, warmup)
    out["closest_points_ms"] = t
    out["closest_points_mqueries_per_s"] = n_queries / t["median"] / 1e3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=1 << 22)
    ap.add_argument("--stacks", type=int, default=512)
    ap.add_argument("--soup", type=int, default=1 << 20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    import bvh_amd
    from bvh_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("bench_winding needs the GPU: nothing is measured without it")
    result = {"queries": args.queries, "calls": args.calls, "warmup": args.warmup,
              "scenes": [measure(torch, bvh_amd, "uv_sphere", uv_sphere(args.stacks, 2 * args.stacks), args.queries, args.calls, args.warmup),
                         measure(torch, bvh_amd, "soup", synth.soup(args.soup), args.queries, args.calls, args.warmup)]}
    line = json.dumps(result)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
