"""Triangle-intersection benchmark (bvh3X_intersect_tris / bvh3X_intersect_tris_self): one JSON line per workload and pass.

    python tools/tri_intersect_bench.py [--scenes soup,terrain] [--calls 5] [--shift 0.002]

Scenes: those of tools/closest_point_bench.py (1M-triangle soup, 1M-triangle terrain, High trees built on the device). Passes:
    self_count / self_fill              bvh3X_intersect_tris_self with BVH_AMD_TRI_SKIP_SHARED (what self_intersections runs), count pass
                                        and fill pass with the exact offsets
    overlap_self_count / _fill          bvh3X_overlap_self on the boxes of the same triangles and the same tree: the walk this one
                                        shares. The difference is the cost of the triangle fetches and the test
    mesh_count / mesh_fill              bvh3X_intersect_tris, the scene's own triangles moved by --shift of the scene's diagonal as
                                        queries, reordered (sorted: true) and as given
    overlap_mesh_count                  bvh3X_overlap_boxes on the boxes of those queries, for the same comparison
The entry points are called directly on buffers allocated once, so a time is that of the library call (keys + sort included when
reordered), not of an allocation. Reported: median ms of --calls calls after two warm-up calls, timed with device events; Mqueries/s;
mean list length; pair records fetched, primitives fetched and leaves visited per query (a separate call with counters); for the
triangle passes box_pairs_per_true_pair, the list entries of the box pass over those of the triangle pass.
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

SKIP_SHARED, SORTED, UNSORTED = 32, 4, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="soup,terrain")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--shift", type=float, default=0.002)
    args = ap.parse_args()
    import torch
    import bvh_amd
    from bvh_amd import _lib, synth
    torch.cuda.set_device(0)
    lib = _lib.load()
    stream = lambda: torch.cuda.current_stream().cuda_stream
    for name in args.scenes.split(","):
        raw, bvh, _ = scene(name)
        m = bvh.prim_count
        tris = torch.from_numpy(np.ascontiguousarray(raw)).cuda()
        bb, _ = bvh_amd.tri_bounds(raw)
        lo, hi = synth.scene_bounds(raw)
        diag = float(np.linalg.norm(hi - lo))
        rng = np.random.default_rng(7)
        move = torch.from_numpy((args.shift * diag * (2 * rng.random((m, 1, 3)) - 1)).astype(raw.dtype)).cuda()
        q = (tris.reshape(m, 3, 3) + move).reshape(m, 9).contiguous()
        qb, _ = bvh_amd.tri_bounds(q)
        f_tris, f_tris_self = getattr(lib, f"bvh{bvh._s}_intersect_tris"), getattr(lib, f"bvh{bvh._s}_intersect_tris_self")
        f_boxes, f_boxes_self = getattr(lib, f"bvh{bvh._s}_overlap_boxes"), getattr(lib, f"bvh{bvh._s}_overlap_self")
        counts = torch.zeros(m, dtype=torch.int32, device="cuda")
        cnt = torch.zeros(3, dtype=torch.int64, device="cuda")

        def out_args(offs, ids, counters):
            return (counts.data_ptr() if offs is None else None, None if offs is None else offs.data_ptr(), None if ids is None else ids.data_ptr(),
                    cnt.data_ptr() if counters else None, stream())

        calls = {
            "self": lambda flags, o=None, i=None, c=False: f_tris_self(bvh._h, tris.data_ptr(), m, SKIP_SHARED, *out_args(o, i, c)),
            "overlap_self": lambda flags, o=None, i=None, c=False: f_boxes_self(bvh._h, bb.data_ptr(), m, 0, *out_args(o, i, c)),
            "mesh": lambda flags, o=None, i=None, c=False: f_tris(bvh._h, tris.data_ptr(), m, q.data_ptr(), m, flags, *out_args(o, i, c)),
            "overlap_mesh": lambda flags, o=None, i=None, c=False: f_boxes(bvh._h, bb.data_ptr(), m, qb.data_ptr(), m, flags, *out_args(o, i, c)),
        }
        totals = {}

        def measure(kind, sort, fill=True):
            run = calls[kind]
            flags = 0 if sort is None else SORTED if sort else UNSORTED
            _lib.check(run(flags), kind)
            offsets = bvh_amd.offsets_from_counts(counts)
            total = int(offsets[m].item())
            totals[kind] = total
            common = {"scene": name, "n": m, "mean_len": round(total / m, 4), "max_len": int(counts.max().item())}
            if kind in ("self", "mesh"):
                common["box_pairs_per_true_pair"] = round(totals["overlap_" + kind] / max(total, 1), 2)
            passes = [("count", None, None)]
            if fill:
                passes.append(("fill", offsets, torch.empty(max(total, 1), dtype=torch.int32, device="cuda")))
            for what, offs, ids in passes:
                ms = timed(lambda: _lib.check(run(flags, offs, ids), kind), args.calls)
                _lib.check(run(flags, offs, ids, True), kind)
                c = cnt.cpu().numpy().astype(np.float64) / m
                line = dict(common, **{"pass": f"{kind}_{what}", "sorted": sort, "ms": round(ms, 4), "mqueries_per_s": round(m / ms / 1e3, 1),
                                       "pairs_per_query": round(float(c[0]), 2), "prims_per_query": round(float(c[1]), 2),
                                       "leaves_per_query": round(float(c[2]), 2)})
                if what == "fill":
                    line["mentries_per_s"] = round(total / ms / 1e3, 1)
                print(json.dumps(line), flush=True)

        measure("overlap_self", None)
        measure("self", None)
        for sort in (True, False):
            measure("overlap_mesh", sort, fill=False)
            measure("mesh", sort)
        del raw, bvh, tris, bb, q, qb, counts
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
