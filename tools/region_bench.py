"""Convex-region benchmark (bvh3X_region_tris): one JSON line per workload and pass.

    python tools/region_bench.py [--calls 5] [--baseline-frusta 510] [--baseline-boxes 10000]

Scene: the 1M-triangle soup of tools/closest_point_bench.py, a High tree built on the device. Workloads:
    tiles     the 8160 tile frusta of a 1920 x 1080 view in 16 x 16-pixel tiles (120 x 68), six planes each, submitted in screen order
              (row after row): tiled light or triangle culling
    boxes     100k randomly oriented boxes of six planes, half-extents 0.2 .. 1 % of the scene's diagonal, centred on the surface
Passes, each through the entry point on buffers allocated once: cull_count / cull_fill (with the inside flags) and exact_count /
exact_fill. Reported: median ms of --calls calls after two warm-up calls, timed with device events; regions per second; mean list
length; pair records fetched, triangles tested and leaves visited per region (a separate call with counters).
    baseline  what a caller did before this query existed: bvh3X_overlap_boxes with each region's bounding box (count, offsets, fill),
              the lists copied to the host, the plane-by-plane filter there in numpy. Wall-clock, on the first --baseline-frusta /
              --baseline-boxes regions of a shuffled order (a tile frustum's bounding box covers a good part of the scene: the whole
              batch would list billions of candidates), beside the wall-clock time of region_search (CULL, lists copied to the host) on
              the same regions, and their ratio.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from closest_point_bench import scene, timed  # noqa: E402

EXACT = 64


def camera(lo, hi):
    centre, diag = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    eye = centre + diag * np.array([0.35, 0.25, -0.9])
    return eye, centre - eye, np.array([0.0, 1.0, 0.0]), diag


def tile_frusta(lo, hi, width=1920, height=1080, tile=16, fov_y=np.radians(60.0), dtype=np.float32):
    """(tiles, 6, 4): near, far, left, right, bottom, top of every tile's frustum, row after row; outward normals; the last row of tiles
    is cut at the image's edge."""
    eye, direction, up, diag = camera(lo.astype(np.float64), hi.astype(np.float64))
    d = direction / np.linalg.norm(direction)
    r = np.cross(d, up)
    r /= np.linalg.norm(r)
    u = np.cross(r, d)
    ty = np.tan(fov_y / 2)
    tx = ty * width / height
    near, far = 0.01 * diag, 2.5 * diag
    out = []
    for y0 in range(0, height, tile):
        v0, v1 = (2 * y0 / height - 1) * ty, (2 * min(y0 + tile, height) / height - 1) * ty
        for x0 in range(0, width, tile):
            u0, u1 = (2 * x0 / width - 1) * tx, (2 * min(x0 + tile, width) / width - 1) * tx
            normals = [-d, d, -r + u0 * d, r - u1 * d, -u + v0 * d, u - v1 * d]
            consts = [d @ eye + near, -(d @ eye) - far] + [-(n @ eye) for n in normals[2:]]
            out.append(np.concatenate([np.stack(normals), np.asarray(consts)[:, None]], axis=1))
    return np.ascontiguousarray(np.stack(out).astype(dtype))


def random_boxes(raw, n, seed, dtype=np.float32):
    rng = np.random.default_rng(seed)
    pts = raw.reshape(-1, 3)
    diag = float(np.linalg.norm(pts.max(axis=0).astype(np.float64) - pts.min(axis=0)))
    c = pts[rng.integers(len(pts), size=n)].astype(np.float64)
    q, rr = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    axes = q * np.sign(np.diagonal(rr, axis1=1, axis2=2))[:, None, :]
    half = diag * (0.002 + 0.008 * rng.random((n, 3)))
    nrm = np.concatenate([axes.transpose(0, 2, 1), -axes.transpose(0, 2, 1)], axis=1)                # (n, 6, 3)
    dd = -np.einsum("nkc,nc->nk", nrm, c) - np.concatenate([half, half], axis=1)
    return np.ascontiguousarray(np.concatenate([nrm, dd[:, :, None]], axis=2).astype(dtype))


def region_bounds(planes):
    """(n, 6) {min, max}: the bounding boxes of bounded regions of three pairs of opposite planes (boxes, frusta): of their 8 corners."""
    p = planes.astype(np.float64)
    n = len(p)
    corners = []
    for a in (0, 1):
        for b in (2, 3):
            for c in (4, 5):
                A = p[:, [a, b, c], :3]
                corners.append(np.linalg.solve(A, -p[:, [a, b, c], 3][:, :, None])[:, :, 0])
    # (frusta: near, far / left, right / bottom, top; boxes: +-axis 0 are planes 0 and 3, and so on)
    corners = np.stack(corners, axis=1)
    assert corners.shape == (n, 8, 3)
    return np.ascontiguousarray(np.concatenate([corners.min(axis=1), corners.max(axis=1)], axis=1).astype(planes.dtype))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--baseline-frusta", type=int, default=510)
    ap.add_argument("--baseline-boxes", type=int, default=10000)
    args = ap.parse_args()
    import torch
    import bvh_amd
    from bvh_amd import _lib, synth
    torch.cuda.set_device(0)
    lib = _lib.load()
    stream = lambda: torch.cuda.current_stream().cuda_stream
    raw, bvh, _ = scene("soup")
    np_ = bvh.prim_count
    tris = torch.from_numpy(np.ascontiguousarray(raw)).cuda()
    bb, _ = bvh_amd.tri_bounds(raw)
    lo, hi = synth.scene_bounds(raw)
    boxes = random_boxes(raw, 100000, 7)
    boxes = np.ascontiguousarray(boxes[:, [0, 3, 1, 4, 2, 5]])                                   # opposite planes side by side
    workloads = (("tiles", tile_frusta(np.asarray(lo), np.asarray(hi)), args.baseline_frusta), ("boxes", boxes, args.baseline_boxes))
    f_region = getattr(lib, f"bvh{bvh._s}_region_tris")
    cnt = torch.zeros(3, dtype=torch.int64, device="cuda")
    for name, planes, n_base in workloads:
        n, m = planes.shape[0], planes.shape[1]
        q = torch.from_numpy(planes).cuda()
        counts = torch.zeros(n, dtype=torch.int32, device="cuda")

        def run(flags, offs=None, ids=None, ins=None, counters=False):
            return f_region(bvh._h, tris.data_ptr(), np_, q.data_ptr(), m, n, flags, counts.data_ptr() if offs is None else None,
                            None if offs is None else offs.data_ptr(), None if ids is None else ids.data_ptr(), None if ins is None else ins.data_ptr(),
                            cnt.data_ptr() if counters else None, stream())

        for kind, flags in (("cull", 0), ("exact", EXACT)):
            _lib.check(run(flags), kind)
            offsets = bvh_amd.offsets_from_counts(counts)
            total = int(offsets[n].item())
            ids = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")
            ins = torch.empty(max(total, 1), dtype=torch.uint8, device="cuda")
            for what, a in (("count", (None, None, None)), ("fill", (offsets, ids, ins))):
                ms = timed(lambda: _lib.check(run(flags, *a), kind), args.calls)
                _lib.check(run(flags, *a, counters=True), kind)
                c = cnt.cpu().numpy().astype(np.float64) / n
                line = {"workload": name, "pass": f"{kind}_{what}", "n": n, "planes": m, "ms": round(ms, 4), "kregions_per_s": round(n / ms, 1),
                        "mean_len": round(total / n, 2), "max_len": int(counts.max().item()), "pairs_per_region": round(float(c[0]), 1),
                        "tris_per_region": round(float(c[1]), 1), "leaves_per_region": round(float(c[2]), 1)}
                if what == "fill":
                    line["mentries_per_s"] = round(total / ms / 1e3, 1)
                    line["inside_fraction"] = round(float(ins[:total].sum(dtype=torch.int64).item()) / max(total, 1), 4)
                print(json.dumps(line), flush=True)
            del ids, ins

        # the baseline, and region_search, wall-clock to lists on the host, on a subset
        pick = np.sort(np.random.default_rng(3).permutation(n)[:min(n_base, n)])
        sub = np.ascontiguousarray(planes[pick])
        qb = region_bounds(sub)
        raw9 = np.ascontiguousarray(raw)
        ids_host = bvh.prim_ids.astype(np.int64)

        def baseline():
            off, lst = bvh_amd.overlap_search(bvh, bb, qb)
            off, lst = off.cpu().numpy(), lst.cpu().numpy()
            t = raw9[ids_host[lst]].reshape(-1, 3, 3)                                             # the candidates' triangles
            row = np.repeat(np.arange(len(sub)), np.diff(off))
            keep = np.ones(len(lst), dtype=bool)
            for p in range(m):
                pl = sub[row, p]
                val = ((pl[:, None, 0] * t[:, :, 0] + pl[:, None, 1] * t[:, :, 1]) + pl[:, None, 2] * t[:, :, 2]) + pl[:, None, 3]
                keep &= (val <= 0).any(axis=1)
            return len(lst), np.bincount(row[keep], minlength=len(sub)), lst[keep]

        def ours():
            off, lst = bvh_amd.region_search(bvh, tris, sub)
            return off.cpu().numpy(), lst.cpu().numpy()

        baseline(), ours()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        candidates, base_counts, base_list = baseline()
        t1 = time.perf_counter()
        off, lst = ours()
        t2 = time.perf_counter()
        # (the baseline lists box AND plane-by-plane: between EXACT's list and CULL's, which has no box)
        print(json.dumps({"workload": name, "pass": "baseline_vs_region_search", "n": len(sub), "candidates": candidates, "baseline_listed": int(len(base_list)), "listed": int(len(lst)),
                          "baseline_wall_ms": round(1e3 * (t1 - t0), 2), "region_search_wall_ms": round(1e3 * (t2 - t1), 2),
                          "ratio": round((t1 - t0) / max(t2 - t1, 1e-9), 1)}), flush=True)
        del q, counts
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
