"""Times the instanced ray query against the flattened scene it replaces ("Instanced ray queries").

    python tools/instanced_bench.py [--rays 1048576] [--instances 1024] [--tris 2048] [--calls 20] [--warmup 3] [--json PATH]

Workload: closest-hit robust rays against `instances` placed copies of a `tris`-triangle soup.
  instanced:  bvh_amd.intersect_instanced through a top tree over the instances' boxes;
  flattened:  the same rays through bvh_amd.intersect(..., sort_rays=False) on one tree over every placed triangle;
  move:       instance_prepare + refit_boxes of the top tree, against refit_tris of the flattened tree.
Each figure is the median of `calls` calls after `warmup` warm-ups, timed with events on the call's stream. The two traces are compared
first: the same rays hit, at the same t up to the rounding of the transform, but for rays that graze an edge. Needs the GPU; prints one JSON line."""
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
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--instances", type=int, default=1024)
    ap.add_argument("--tris", type=int, default=2048)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    import bvh_amd
    from bvh_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("instanced_bench needs the GPU: nothing is measured without it")

    rng = np.random.default_rng(2024)
    soup = synth.soup(args.tris, seed=31, jitter=0.05) - np.float32(0.5)             # around the origin, in [-0.5, 0.5]^3
    n = args.instances
    side = float(np.cbrt(n)) * 1.5
    mats = np.zeros((n, 3, 4), dtype=np.float64)
    for k in range(n):
        q = rng.normal(size=4)
        w, x, y, z = q / np.linalg.norm(q)
        rot = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                        [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                        [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        mats[k, :, :3] = rot @ np.diag(rng.uniform(0.7, 1.3, size=3))
        mats[k, :, 3] = rng.uniform(0, side, size=3)
    mats = mats.astype(np.float32)

    # the geometry and the two-level scene
    d_soup = torch.from_numpy(soup).cuda()
    bb, cc = bvh_amd.tri_bounds(d_soup)
    geom = bvh_amd.DefaultBuilder.build(bb, cc)
    prims = bvh_amd.precompute_tris(d_soup, geom.device_prim_ids())
    geoms = [(geom, prims)]
    d_mats = torch.from_numpy(mats.reshape(n, 12)).cuda()
    w2o, ibb, icc = bvh_amd.instance_prepare(geoms, d_mats)
    top = bvh_amd.DefaultBuilder.build(ibb, icc)

    # the flattened scene: every triangle of every instance in world space
    verts = soup.reshape(-1, 3)
    flat = (np.einsum("kij,vj->kvi", mats[:, :, :3], verts) + mats[:, None, :, 3]).astype(np.float32).reshape(-1, 9)
    d_flat = torch.from_numpy(flat).cuda()
    fbb, fcc = bvh_amd.tri_bounds(d_flat)
    flat_bvh = bvh_amd.DefaultBuilder.build(fbb, fcc)
    flat_prims = bvh_amd.precompute_tris(d_flat, flat_bvh.device_prim_ids())

    lo, hi = synth.scene_bounds(flat)
    rays = torch.from_numpy(synth.rays_closest(args.rays, lo, hi)).cuda()

    hits_i, inst = bvh_amd.intersect_instanced(top, geoms, w2o, rays, robust=True)
    hits_f = bvh_amd.intersect(flat_bvh, flat_prims, rays, robust=True, sort_rays=False)
    hi_np, hf_np = bvh_amd.hits_to_numpy(hits_i), bvh_amd.hits_to_numpy(hits_f)
    both = (hi_np["prim"] != bvh_amd.INVALID) & (hf_np["prim"] != bvh_amd.INVALID)
    agree = float(((hi_np["prim"] != bvh_amd.INVALID) == (hf_np["prim"] != bvh_amd.INVALID)).mean())
    # (a ray that grazes an edge can take that triangle in one scene and the one behind it in the other: the two scenes round their
    #  vertices differently. So the difference in t is reported as its median and as the share of rays beyond 1e-4, not as a maximum.)
    rel_t = np.abs(hi_np["t"][both] - hf_np["t"][both]) / np.maximum(hf_np["t"][both], 1e-6) if both.any() else np.zeros(1)

    out_i = torch.empty_like(hits_i)
    out_f = torch.empty_like(hits_f)
    t_inst = median_ms(torch, lambda: bvh_amd.intersect_instanced(top, geoms, w2o, rays, robust=True, out=out_i), args.calls, args.warmup)
    t_flat = median_ms(torch, lambda: bvh_amd.intersect(flat_bvh, flat_prims, rays, robust=True, sort_rays=False, out=out_f), args.calls, args.warmup)

    def move_instanced():
        _, b, _ = bvh_amd.instance_prepare(geoms, d_mats)
        top.refit_boxes(b)

    t_move = median_ms(torch, move_instanced, args.calls, args.warmup)
    t_refit = median_ms(torch, lambda: flat_bvh.refit_tris(d_flat, out=flat_prims), args.calls, args.warmup)

    result = {"rays": args.rays, "instances": n, "tris_per_geometry": args.tris, "flattened_tris": int(len(flat)), "calls": args.calls, "warmup": args.warmup,
              "hit_fraction": float((hi_np["prim"] != bvh_amd.INVALID).mean()), "hit_miss_agreement": agree, "median_relative_t_difference": float(np.median(rel_t)), "share_of_hits_with_t_beyond_1e-4": float((rel_t > 1e-4).mean()),
              "intersect_instanced_ms": {"median": t_inst[0], "min": t_inst[1], "max": t_inst[2]},
              "intersect_flattened_unsorted_ms": {"median": t_flat[0], "min": t_flat[1], "max": t_flat[2]},
              "instance_prepare_plus_refit_boxes_ms": {"median": t_move[0], "min": t_move[1], "max": t_move[2]},
              "flattened_refit_tris_ms": {"median": t_refit[0], "min": t_refit[1], "max": t_refit[2]},
              "instanced_mrays_per_s": args.rays / t_inst[0] / 1e3, "flattened_mrays_per_s": args.rays / t_flat[0] / 1e3}
    line = json.dumps(result)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
