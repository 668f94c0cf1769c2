// Batched sphere-cast queries for gfx950: for every ray {org, dir, tmin, tmax} and radius r, the first t in [tmin, tmax] at which a
// ball of radius r centred at org + t dir touches a BVH-order primitive (PrecomputedTri or Sphere<T, 3>), as one hit record
// {prim, t, u, v}. The per-lane walk and the sweep test are sphere_cast_body.inc (shared with the host test harness,
// tests/cpp/sphere_cast_body_host.cpp) over nearest_walk.inc and the ray arithmetic of trace_device.h; the launch path is
// point_query.h's; this file holds the kernel and what is specific to the query.
//
// MI355X mapping (closest.hip's, with the ray walk of ray_nearest.hip in place of the point walk):
//   * one lane per query, one-shot grid of ceil(n / 256) blocks: no ticket counter, so no work slot of the tree is claimed and any
//     number of launches of one const tree may run at once;
//   * depth-first walk over the pair records, the child whose grown box the ray enters first taken first, the other stacked with its
//     entry t so that a popped entry is re-checked against the best contact before anything is fetched;
//   * the stack: kClosestLds entries in LDS ([depth][lane]), the rest of 64 in per-lane scratch, beyond 64 (deep trees) in HBM;
//   * the fast / robust slab test is one more compile-time choice of the kernel, as in ray_nearest.hip;
//   * optionally the batch is read in the order of the Hilbert cell of each origin in the root box and the octant of the direction
//     (query_order.h, all-hits' key). Records are always written in the caller's order, with streaming stores.
//
// Compiled with -ffp-contract=off; division and sqrt are the correctly rounded forms (bit-identical to the host harness).

#include "common.h"
#include "trace_device.h"
#include "ray_key.h"
#include "query_order.h"
#include "sphere_cast_body.inc"
#include "point_query.h"

namespace bvh_amd {

namespace {

template <typename T, int Leaf, bool Robust, bool Stats, bool Deep>
__global__ void __launch_bounds__(kBlock) sphere_cast_kernel(SphereCastArgs<T> a) {
    __shared__ uint32_t lds_node[kClosestLds * kBlock];
    __shared__ T lds_t[kClosestLds * kBlock];
    const int tid = threadIdx.x;
    const unsigned long long lane = static_cast<unsigned long long>(blockIdx.x) * kBlock + tid;
    unsigned long long cnt[3] = {0, 0, 0};
    if (lane < a.n) sphere_cast_lane<T, Leaf, Robust, Stats, Deep>(a, a.first + lane, lds_node, lds_t, tid, lane, cnt);
    if (Stats) add_counters(a.counters, cnt, tid);
}

} // namespace

template <typename T>
int launch_sphere_cast(const BvhImpl<T>& b, int leaf_kind, const T* d_prims, const T* d_rays, size_t n, T radius, const T* d_radii, unsigned flags,
                       typename HitOf<T>::Type* d_hits, bvh_amd_counters* d_counters, hipStream_t stream) {
    using Hit = typename HitOf<T>::Type;
    const bool aligned = !(misaligned(d_prims, 16) || misaligned(d_rays, 16) || misaligned(d_counters, 8) || misaligned(d_hits, sizeof(Hit)) ||
                           misaligned(d_radii, sizeof(T)));
    if (const int rc = point_query_check(b, n, flags, d_prims && d_rays && d_hits,
                                         aligned ? nullptr : "device pointers must be aligned (prims and rays 16 bytes, counters 8, radii to their scalar, hit records to their size)",
                                         "sphere_cast", BVH_AMD_RAY_ROBUST);
        rc || n == 0)
        return rc;
    const bool robust = (flags & BVH_AMD_RAY_ROBUST) != 0;
    return point_query_run<T, kQueryRays>(b, d_prims, d_rays, n, flags, d_counters, sizeof(uint32_t) + sizeof(T), kBlock, kPointSortMin, kPointKeyBits,
                                          "sphere_cast", stream, [&](const PointArgs<T>& args, T* deep_t) {
        const SphereCastArgs<T> a{args, d_hits, deep_t, d_radii, radius};
        return point_query_dispatch(leaf_kind, d_counters != nullptr, a.deep_cap != 0, [&](auto leaf, auto stats, auto deep) {
            return robust ? point_query_launch(sphere_cast_kernel<T, leaf(), true, stats(), deep()>, a, kBlock, 0, stream)
                          : point_query_launch(sphere_cast_kernel<T, leaf(), false, stats(), deep()>, a, kBlock, 0, stream);
        });
    });
}

template int launch_sphere_cast<float>(const BvhImpl<float>&, int, const float*, const float*, size_t, float, const float*, unsigned, bvh_hit3f*,
                                       bvh_amd_counters*, hipStream_t);
template int launch_sphere_cast<double>(const BvhImpl<double>&, int, const double*, const double*, size_t, double, const double*, unsigned, bvh_hit3d*,
                                        bvh_amd_counters*, hipStream_t);

} // namespace bvh_amd
