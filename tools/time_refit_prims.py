"""Developer probe: what a frame of moving geometry costs on a resident tree (bvhXX_refit_boxes / bvh3X_refit_tris) against the
host-mirror refit it replaces and against a rebuild.   python tools/time_refit_prims.py [n_tris] [--reps R] [--no-frames] [--profile-run]

Host clock around work that ends in a device synchronise, after a warm-up; the sides of each comparison alternate within one
repetition, in one process. Per scene (1M soup, 1M Sponza proxy; f32, default pool-High tree):
  A  Bvh.refit() with the leaf boxes already in place (the old path: push + refit + re-layout + pull; it does LESS work than B..D)
  B  refit_boxes, steady state            C  tri_bounds + refit_boxes + precompute_tris(perm)            D  refit_tris
  Low / High rebuild + precompute_tris of the same triangles; traversal_cost and traced Mrays/s after 0, 1, 10, 50 frames of 1 %
  displacement. Also prints the bytes each new kernel must move (from shapes) for the share-of-peak figure; the kernel times come
  from a separate `rocprofv3 --kernel-trace --stats -- python tools/time_refit_prims.py --profile-run` run."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bvh_amd
from bvh_amd import synth

HBM_PEAK = 8.0e12                                             # bytes/s (spec); 6.29e12 measured for a float4 copy

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if args else 1_000_000
reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 20
frames_on = "--no-frames" not in sys.argv
profile_run = "--profile-run" in sys.argv


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def report(name, ts):
    ts = sorted(ts)
    print(f"  {name:<44} median {statistics.median(ts):8.3f} ms   min {ts[0]:8.3f}   max {ts[-1]:8.3f}   ({len(ts)} reps)", flush=True)


def displace(d_tris, frac, extent, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return d_tris + (torch.rand(d_tris.shape, generator=g, device="cuda", dtype=d_tris.dtype) - 0.5) * (2 * frac * extent)


for scene, make in (("soup", synth.soup), ("sponza_proxy", synth.sponza_proxy)):
    tris = make(n)
    lo, hi = synth.scene_bounds(tris)
    extent = float(np.max(hi - lo))
    d_tris = torch.from_numpy(tris).cuda()
    d_moved = displace(d_tris, 0.01, extent, 1)
    high = bvh_amd.Config(quality=bvh_amd.Quality.High)
    low = bvh_amd.Config(quality=bvh_amd.Quality.Low)
    pool = bvh_amd.ThreadPool()
    bb, cc = bvh_amd.tri_bounds(d_tris)
    old = bvh_amd.DefaultBuilder.build(bb, cc, high, thread_pool=pool)      # the tree the old path works on
    new = bvh_amd.DefaultBuilder.build(bb, cc, high, thread_pool=pool)      # ... and the new one: same tree, never touched by the host
    nodes, prims_n = new.node_count, new.prim_count
    out = torch.empty((prims_n, 12), dtype=torch.float32, device="cuda")
    d_bb = bvh_amd.tri_bounds(d_moved)[0]
    perm = new.device_prim_ids()
    print(f"{scene}: {n} triangles, {nodes} nodes, f32, DefaultBuilder(pool, High)", flush=True)

    def a_old():
        old.refit()

    def b_boxes():
        new.refit_boxes(d_bb)

    def c_three():
        new.refit_boxes(bvh_amd.tri_bounds(d_moved)[0])
        bvh_amd.precompute_tris(d_moved, perm)

    def d_tris_fused():
        new.refit_tris(d_moved, out=out)

    sides = (("A  Bvh.refit() (host-mirror path)", a_old), ("B  refit_boxes", b_boxes),
             ("C  tri_bounds + refit_boxes + precompute_tris", c_three), ("D  refit_tris", d_tris_fused))
    if profile_run:
        for _, fn in sides[1:]:
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        continue
    for _, fn in sides:                                       # warm-up: code objects, scratch cache, the one-offs of the first call
        for _ in range(3):
            fn()
    times = {name: [] for name, _ in sides}
    for _ in range(reps):
        for name, fn in sides:                                # alternated within a repetition
            times[name].append(timed(fn))
    for name, _ in sides:
        report(name, times[name])
    for name, cfg in (("Low rebuild + precompute_tris", low), ("High rebuild + precompute_tris", high)):
        def rebuild():
            b2, c2 = bvh_amd.tri_bounds(d_moved)
            t = bvh_amd.DefaultBuilder.build(b2, c2, cfg, thread_pool=pool)
            bvh_amd.precompute_tris(d_moved, t.device_prim_ids())
        rebuild()
        report(name, [timed(rebuild) for _ in range(max(3, reps // 4))])

    # bytes the new kernels must move, from shapes (reads + writes, every array once)
    node_b, rec_b = 28, 64
    climb = nodes * node_b * 2 + (nodes - 1) * rec_b // 2 + nodes * 4 * 2 * 2 + prims_n * 4      # nodes read + written, record halves, parent + arrived, prim ids
    parents = nodes * node_b + nodes * 4 * 2                  # nodes read, parent written (+ its memset)
    for kernel, bytes_ in (("k_refit_prims<float, 0> (boxes)", climb + prims_n * 24), ("k_refit_prims<float, 2> (tris)", climb + prims_n * 36),
                           ("k_refit_parents<float>", parents), ("precompute_kernel<float> (perm)", prims_n * (36 + 4 + 48))):
        print(f"  bytes {kernel:<40} {bytes_ / 1e6:8.1f} MB  -> {bytes_ / HBM_PEAK * 1e6:7.1f} us at the HBM peak of {HBM_PEAK / 1e12:.1f} TB/s", flush=True)

    if frames_on:
        rays = torch.from_numpy(synth.rays_closest(1 << 22, lo, hi, seed=9)).cuda()
        cur, done = d_tris, 0
        for upto in (0, 1, 10, 50):
            for f in range(done, upto):
                cur = displace(cur, 0.01, extent, 100 + f)
                new.refit_tris(cur, out=out)
            done = upto
            if upto == 0:
                new.refit_tris(cur, out=out)
            for _ in range(3):
                bvh_amd.intersect(new, out, rays, robust=True)
            ms = statistics.median(timed(lambda: bvh_amd.intersect(new, out, rays, robust=True)) for _ in range(5))
            b2, c2 = bvh_amd.tri_bounds(cur)
            fresh = bvh_amd.DefaultBuilder.build(b2, c2, high, thread_pool=pool)
            p2 = bvh_amd.precompute_tris(cur, fresh.device_prim_ids())
            for _ in range(3):
                bvh_amd.intersect(fresh, p2, rays, robust=True)
            ms2 = statistics.median(timed(lambda: bvh_amd.intersect(fresh, p2, rays, robust=True)) for _ in range(5))
            print(f"  after {upto:2d} frames of 1 % displacement: traversal_cost {new.traversal_cost():8.2f}, {rays.shape[0] / ms / 1e3:7.1f} Mrays/s refitted"
                  f"   |   rebuilt High: traversal_cost {fresh.traversal_cost():8.2f}, {rays.shape[0] / ms2 / 1e3:7.1f} Mrays/s", flush=True)
            del fresh, p2
    del old, new
