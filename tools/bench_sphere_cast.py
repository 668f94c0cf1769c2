"""Times the sphere-cast queries ("Sphere-cast queries").

    python tools/bench_sphere_cast.py [--rays 4194304] [--soup 1048576] [--calls 20] [--warmup 3] [--json PATH]

Scene: synth.soup(--soup), default build. Two batches of --rays rays: `coherent`, the primary rays of a pinhole camera outside the
scene looking at its centre (2048 x rays / 2048 pixels), and `uniform`, synth.rays_closest (origins and targets uniform in the scene's
box scaled 1.1). Per batch:
  sphere_cast:      bvh_amd.sphere_cast at radius 0, 0.1 % and 1 % of the scene's diagonal, the batch reordered inside the call as the
                    library decides (the reorder is inside the timed pass), with the counters per ray and the hit fraction from one
                    extra call;
  ray_hits_nearest: bvh_amd.ray_hits_nearest(k = 1) on the same rays, as the yardstick.
Each figure is the median of `calls` calls after `warmup` warm-ups, timed with events on the call's stream. Needs the GPU; prints one
JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_winding import median_ms  # noqa: E402


def measure(torch, bvh_amd, name, bvh, prims, rays, diag, calls, warmup):
    n = rays.shape[0]
    out = {"batch": name, "rays": int(n)}
    hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    for label, frac in (("r0", 0.0), ("r0.1pct", 0.001), ("r1pct", 0.01)):
        r = frac * diag
        rec, cnt = bvh_amd.sphere_cast(bvh, prims, rays, r, counters=True)
        cnt = cnt.cpu().numpy() / n
        t = median_ms(torch, lambda: bvh_amd.sphere_cast(bvh, prims, rays, r, out=hits), calls, warmup)
        out[f"sphere_cast_{label}"] = {"radius": r, "ms": t, "mrays_per_s": n / t["median"] / 1e3,
                                       "per_ray": {"pair_records": float(cnt[0]), "prim_tests": float(cnt[1]), "leaves": float(cnt[2])},
                                       "hit_fraction": float((rec[:, 0].view(torch.int32) != -1).float().mean().item())}
    t = median_ms(torch, lambda: bvh_amd.ray_hits_nearest(bvh, prims, rays, 1), calls, warmup)
    out["ray_hits_nearest_k1"] = {"ms": t, "mrays_per_s": n / t["median"] / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 22)
    ap.add_argument("--soup", type=int, default=1 << 20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    import bvh_amd
    from bvh_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("bench_sphere_cast needs the GPU: nothing is measured without it")
    tris = synth.soup(args.soup)
    d_tris = torch.from_numpy(tris).cuda()
    bb, cc = bvh_amd.tri_bounds(d_tris)
    bvh = bvh_amd.DefaultBuilder.build(bb, cc)
    prims = bvh_amd.precompute_tris(d_tris, bvh.device_prim_ids())
    lo, hi = synth.scene_bounds(tris)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    diag = float(np.linalg.norm(hi - lo))
    mid = (lo + hi) / 2
    width = 2048
    eye = mid + np.array([0.0, 0.0, 1.6]) * (hi - lo)
    coherent = bvh_amd.pinhole_rays(width, max(1, args.rays // width), eye, mid - eye, [0.0, 1.0, 0.0])
    uniform = torch.from_numpy(synth.rays_closest(args.rays, lo, hi)).cuda()
    result = {"triangles": int(len(tris)), "nodes": int(bvh.node_count), "diagonal": diag, "calls": args.calls, "warmup": args.warmup,
              "batches": [measure(torch, bvh_amd, "coherent", bvh, prims, coherent, diag, args.calls, args.warmup),
                          measure(torch, bvh_amd, "uniform", bvh, prims, uniform, diag, args.calls, args.warmup)]}
    line = json.dumps(result)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
