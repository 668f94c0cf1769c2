// Batched closest-point queries for gfx950: for every query point {x, y, z, max_distance}, the BVH-order primitive nearest to it
// (PrecomputedTri or Sphere<T, 3>) within max_distance, and the distance. The per-lane walk is closest_body.inc (shared with the host
// test harness, tests/cpp/closest_body_host.cpp) over point_walk.inc (distance functions, stack); the launch path is point_query.h's;
// this file holds the kernel and what is specific to the query.
//
// MI355X mapping:
//   * one lane per query, one-shot grid of ceil(n / 256) blocks: no ticket counter, so no work slot of the tree is claimed and any
//     number of launches of one const tree may run at once;
//   * depth-first walk over the 64 / 128-byte pair records (common.h: PairNode), nearer child first, the farther one stacked with its
//     box distance^2 so that a popped entry is re-checked against the best distance before anything is fetched;
//   * the stack: kClosestLds entries in LDS, the rest of 64 in per-lane scratch, beyond 64 (deep trees) in HBM (point_walk.inc);
//   * optionally the batch is read in the order of the Hilbert cell of each point in the root box (ray_key.h, radix sort): neighbouring
//     lanes then walk the same records (query_order.h). Records are always written in the caller's order.
//
// Compiled with -ffp-contract=off; division and sqrt are the correctly rounded forms (bit-identical to the host harness).

#include "common.h"
#include "trace_device.h"
#include "ray_key.h"
#include "query_order.h"
#include "closest_body.inc"
#include "point_query.h"

namespace bvh_amd {

namespace {

template <typename T, int Leaf, bool Stats, bool Deep>
__global__ void __launch_bounds__(kBlock) closest_kernel(ClosestArgs<T> a) {
    __shared__ uint32_t lds_node[kClosestLds * kBlock];
    __shared__ T lds_d2[kClosestLds * kBlock];
    const int tid = threadIdx.x;
    const unsigned long long lane = static_cast<unsigned long long>(blockIdx.x) * kBlock + tid;
    unsigned long long cnt[3] = {0, 0, 0};
    if (lane < a.n) closest_lane<T, Leaf, Stats, Deep>(a, a.first + lane, lds_node, lds_d2, tid, lane, cnt);
    if (Stats) add_counters(a.counters, cnt, tid);
}

} // namespace

template <typename T>
int launch_closest(const BvhImpl<T>& b, int leaf_kind, const T* d_prims, const T* d_queries, size_t n, unsigned flags,
                   typename HitOf<T>::Type* d_hits, bvh_amd_counters* d_counters, hipStream_t stream) {
    const bool aligned = !(misaligned(d_prims, 16) || misaligned(d_queries, 16) || misaligned(d_hits, 16) || misaligned(d_counters, 8));
    if (const int rc = point_query_check(b, n, flags, d_prims && d_queries && d_hits,
                                         aligned ? nullptr : "device pointers must be 16-byte aligned (counters 8-byte)", "closest_points");
        rc || n == 0)
        return rc;
    static const size_t sort_min = static_cast<size_t>(std::max(0, BVH_DEV_INT("BVH_AMD_CLOSEST_SORT_MIN", static_cast<int>(kPointSortMin))));   // developer knob
    static const int cell_bits = std::max(1, std::min(8, BVH_DEV_INT("BVH_AMD_CLOSEST_KEY_BITS", kPointKeyBits)));                            // developer knob
    return point_query_run<T>(b, d_prims, d_queries, n, flags, d_counters, sizeof(uint32_t) + sizeof(T), kBlock, sort_min, cell_bits, "closest_points", stream,
                              [&](const PointArgs<T>& args, T* deep_d2) {
        const ClosestArgs<T> a{args, d_hits, deep_d2};
        return point_query_dispatch(leaf_kind, d_counters != nullptr, a.deep_cap != 0, [&](auto leaf, auto stats, auto deep) {
            return point_query_launch(closest_kernel<T, leaf(), stats(), deep()>, a, kBlock, 0, stream);
        });
    });
}

template int launch_closest<float>(const BvhImpl<float>&, int, const float*, const float*, size_t, unsigned, bvh_hit3f*, bvh_amd_counters*, hipStream_t);
template int launch_closest<double>(const BvhImpl<double>&, int, const double*, const double*, size_t, unsigned, bvh_hit3d*, bvh_amd_counters*, hipStream_t);

} // namespace bvh_amd
