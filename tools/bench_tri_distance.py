"""Times the triangle-distance queries ("Triangle-distance queries").

    python tools/bench_tri_distance.py [--queries 1048576] [--tris 1048576] [--calls 10] [--warmup 2] [--json PATH]

Scenes: synth.soup(--tris) and synth.terrain(--tris), default build. One batch of --queries query triangles per scene, in random
order: copies of random triangles of the scene, shrunk to 30 % about their centroid and moved by a normal offset of 1 % of the
scene's diagonal per axis (so some cross the mesh and most lie a few triangle sizes away from it). Per scene, bvh_amd.tri_distance
with sort_queries True and False (the reorder is inside the timed pass) and max_distance infinite and 1 % of the diagonal, each
with the counters per query (pair records, triangles fetched, leaves) and the shares of hits and of zero distances from one extra
call. Each figure is the median of `calls` calls after `warmup` warm-ups, timed with events on the call's stream. Needs the GPU;
prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_winding import median_ms  # noqa: E402


def make_queries(torch, d_tris, n, diag, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    t = d_tris.view(-1, 3, 3)
    pick = torch.randint(0, t.shape[0], (n,), device="cuda", generator=g)
    src = t[pick]
    cen = src.mean(dim=1, keepdim=True)
    move = torch.randn((n, 1, 3), device="cuda", generator=g, dtype=t.dtype) * (0.01 * diag)
    return (cen + 0.3 * (src - cen) + move).reshape(n, 9).contiguous()


def measure(torch, bvh_amd, name, tris, n, calls, warmup):
    d_tris = torch.from_numpy(tris).cuda()
    bb, cc = bvh_amd.tri_bounds(d_tris)
    bvh = bvh_amd.DefaultBuilder.build(bb, cc)
    p = tris.reshape(-1, 3)
    diag = float(np.linalg.norm(p.max(axis=0).astype(np.float64) - p.min(axis=0).astype(np.float64)))
    q = make_queries(torch, d_tris, n, diag, 5)
    out = {"scene": name, "triangles": int(len(tris)), "nodes": int(bvh.node_count), "diagonal": diag, "queries": int(n), "runs": []}
    hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    for limit_name, limit in (("inf", float("inf")), ("1pct", 0.01 * diag)):
        for sort in (True, False):
            rec, cnt = bvh_amd.tri_distance(bvh, d_tris, q, limit, sort_queries=sort, counters=True)
            cnt = cnt.cpu().numpy() / n
            found = rec[:, 0].view(torch.int32) != -1
            t = median_ms(torch, lambda: bvh_amd.tri_distance(bvh, d_tris, q, limit, sort_queries=sort, out=hits), calls, warmup)
            out["runs"].append({"max_distance": limit_name, "sorted": sort, "ms": t, "mqueries_per_s": n / t["median"] / 1e3,
                                "per_query": {"pair_records": float(cnt[0]), "triangles": float(cnt[1]), "leaves": float(cnt[2])},
                                "hit_fraction": float(found.float().mean().item()),
                                "zero_fraction": float((found & (rec[:, 1] == 0)).float().mean().item())})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--tris", type=int, default=1 << 20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    import bvh_amd
    from bvh_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("bench_tri_distance needs the GPU: nothing is measured without it")
    result = {"calls": args.calls, "warmup": args.warmup,
              "scenes": [measure(torch, bvh_amd, "soup", synth.soup(args.tris), args.queries, args.calls, args.warmup),
                         measure(torch, bvh_amd, "terrain", synth.terrain(args.tris), args.queries, args.calls, args.warmup)]}
    line = json.dumps(result)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
