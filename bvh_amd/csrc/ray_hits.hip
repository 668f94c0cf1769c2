// Batched all-hits ray queries for gfx950: for every ray {org, dir, tmin, tmax}, how many BVH-order primitives (PrecomputedTri or
// Sphere<T, 3>) the unshortened ray crosses and, optionally, their hit records. The per-lane body is ray_hits_body.inc (shared with
// the host test harness, tests/cpp/ray_hits_body_host.cpp): the ray and its two tests — the slab test and the leaf tests of the ray
// walks (trace_device.h, tri_test.inc) — handed to the walk of the list queries, list_walk.inc (stack, descent, counts, segments;
// shared with radius.hip and overlap.hip); the launch path is point_query.h's; this file holds the kernel and what is specific to
// the query.
//
// MI355X mapping (radius.hip's, with the slab test in place of the distance to a box):
//   * one lane per ray, one-shot grid of ceil(n / 256) blocks: no ticket counter, so no work slot of the tree is claimed and any
//     number of launches of one const tree may run at once;
//   * depth-first walk over the 64 / 128-byte pair records, left child first, the right one stacked as a bare node word when the ray
//     meets both boxes. Nothing is pruned against what was found and nothing is ordered by distance: the list of a ray is fixed by
//     the tree;
//   * the stack: kRayHitsLds entries in LDS, the rest of 64 in per-lane scratch, beyond 64 (deep trees) in HBM (point_walk.inc);
//   * radius search's variable-length output: counts, segments [offsets[r], offsets[r + 1]), padding (the Fill = false kernels hold
//     no record store and no offset load); a record is one 16-byte (float) or two 16-byte (double) streaming stores;
//   * the fast / robust slab test is one more compile-time choice of the kernel, as in traverse.hip;
//   * optionally the batch is read in the order of the Hilbert cell of each origin in the root box and the octant of the direction
//     (query_order.h). Outputs are always in the caller's order.
//
// Compiled with -ffp-contract=off; division and sqrt are the correctly rounded forms (bit-identical to the host harness and to
// traverse.hip's records).

#include "common.h"
#include "trace_device.h"
#include "ray_key.h"
#include "query_order.h"
#include "ray_hits_body.inc"
#include "point_query.h"

namespace bvh_amd {

namespace {

template <typename T, int Leaf, bool Robust, bool Stats, bool Deep, bool Fill>
__global__ void __launch_bounds__(kBlock) ray_hits_kernel(RayHitsArgs<T> a) {
    __shared__ uint32_t lds_node[kRayHitsLds * kBlock];
    const int tid = threadIdx.x;
    const unsigned long long lane = static_cast<unsigned long long>(blockIdx.x) * kBlock + tid;
    unsigned long long cnt[3] = {0, 0, 0};
    if (lane < a.n) ray_hits_lane<T, Leaf, Robust, Stats, Deep, Fill>(a, a.first + lane, lds_node, tid, lane, cnt);
    if (Stats) add_counters(a.counters, cnt, tid);
}

} // namespace

template <typename T>
int launch_ray_hits(const BvhImpl<T>& b, int leaf_kind, const T* d_prims, const T* d_rays, size_t n, unsigned flags, uint32_t* d_counts,
                    const uint64_t* d_offsets, typename HitOf<T>::Type* d_list_hits, bvh_amd_counters* d_counters, hipStream_t stream) {
    using Hit = typename HitOf<T>::Type;
    const bool aligned = !(misaligned(d_prims, 16) || misaligned(d_rays, 16) || misaligned(d_offsets, 8) || misaligned(d_counters, 8) ||
                           misaligned(d_counts, 4) || misaligned(d_list_hits, sizeof(Hit)));
    const char* fault = !d_counts && !d_offsets   ? "at least one of d_counts and d_offsets is required"
                        : d_offsets && !d_list_hits ? "d_offsets needs d_list_hits"
                        : !d_offsets && d_list_hits ? "lists need d_offsets"
                                                    : nullptr;
    if (!fault && !aligned) fault = "device pointers must be aligned (prims and rays 16 bytes, offsets and counters 8, counts 4, hit records to their size)";
    if (const int rc = point_query_check(b, n, flags, d_prims && d_rays, fault, "intersect_rays_all", BVH_AMD_RAY_ROBUST); rc || n == 0) return rc;
    const bool robust = (flags & BVH_AMD_RAY_ROBUST) != 0;
    return point_query_run<T, kQueryRays>(b, d_prims, d_rays, n, flags, d_counters, sizeof(uint32_t), kBlock, kPointSortMin, kPointKeyBits, "intersect_rays_all",
                                          stream, [&](const PointArgs<T>& args, T*) {
        const RayHitsArgs<T> a{{args, d_counts, reinterpret_cast<const unsigned long long*>(d_offsets), nullptr}, d_list_hits};
        return list_query_dispatch(leaf_kind, d_counters != nullptr, a.deep_cap != 0, a.offsets != nullptr, [&](auto leaf, auto stats, auto deep, auto fill) {
            return robust ? point_query_launch(ray_hits_kernel<T, leaf(), true, stats(), deep(), fill()>, a, kBlock, 0, stream)
                          : point_query_launch(ray_hits_kernel<T, leaf(), false, stats(), deep(), fill()>, a, kBlock, 0, stream);
        });
    });
}

template int launch_ray_hits<float>(const BvhImpl<float>&, int, const float*, const float*, size_t, unsigned, uint32_t*, const uint64_t*, bvh_hit3f*,
                                    bvh_amd_counters*, hipStream_t);
template int launch_ray_hits<double>(const BvhImpl<double>&, int, const double*, const double*, size_t, unsigned, uint32_t*, const uint64_t*, bvh_hit3d*,
                                     bvh_amd_counters*, hipStream_t);

} // namespace bvh_amd
