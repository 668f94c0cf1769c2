// Batched nearest-hits ray queries for gfx950: for every ray {org, dir, tmin, tmax}, the first k BVH-order primitives (PrecomputedTri
// or Sphere<T, 3>) it crosses, front to back, as one row of k hit records in ascending (t, index) order. The per-lane walk and the
// candidate set are ray_nearest_body.inc (shared with the host test harness, tests/cpp/ray_nearest_body_host.cpp) over knn_heap.inc
// (the candidate heap in LDS, shared with knn.hip) and the ray arithmetic of trace_device.h / tri_test.inc; the launch path is
// point_query.h's; this file holds the kernel and what is specific to the query.
//
// MI355X mapping (knn.hip's, with the ray walk in place of the point walk):
//   * one lane per ray, one-shot grid: no ticket counter, so no work slot of the tree is claimed and any number of launches of one
//     const tree may run at once;
//   * the closest-hit walk (near child first, the far one stacked with its entry t), pruned against the worst of the k candidates
//     held instead of the best hit: the ray is shortened to its k-th crossing so far;
//   * the candidates: a binary max-heap of k {t, index} per lane in LDS, [slot][lane] arrays (a lane's bank does not depend on the
//     slot), the worst pair and the fill count in registers; heapsorted in place at the end. A full hit record per candidate would
//     not fit (16 / 32 bytes x 64 x 256 lanes against 160 KB): the leaf test runs again on the <= k winners and the row is written
//     with streaming stores, 16 bytes (float) or two of them (double) per record;
//   * k is a run-time argument: the LDS is dynamic, (k + kKnnLds) * (sizeof(T) + 4) bytes per lane, and a block has 256, 128 or 64
//     lanes, whichever keeps the most rays resident on a CU for that k (knn_lanes.h: knn_block_lanes);
//   * the stack: kKnnLds entries in LDS, the rest of 64 in per-lane scratch, beyond 64 (deep trees) in HBM (point_walk.inc);
//   * the fast / robust slab test is one more compile-time choice of the kernel, as in ray_hits.hip;
//   * optionally the batch is read in the order of the Hilbert cell of each origin in the root box and the octant of the direction
//     (query_order.h, all-hits' key). Rows are always written in the caller's order.
//
// Compiled with -ffp-contract=off; division and sqrt are the correctly rounded forms (bit-identical to the host harness and to
// traverse.hip's and ray_hits.hip's records).

#include "common.h"
#include "trace_device.h"
#include "ray_key.h"
#include "query_order.h"
#include "ray_nearest_body.inc"
#include "point_query.h"
#include "knn_lanes.h"

namespace bvh_amd {

namespace {

template <typename T, int Leaf, bool Robust, bool Stats, bool Deep>
__global__ void __launch_bounds__(kBlock) ray_nearest_kernel(RayNearestArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ray_nearest_lds_raw[];
    const uint32_t stride = blockDim.x;
    const KnnLds<T> lds = knn_lds_carve<T>(ray_nearest_lds_raw, a.k, stride);
    const int tid = threadIdx.x;
    const unsigned long long lane = static_cast<unsigned long long>(blockIdx.x) * stride + tid;
    unsigned long long cnt[3] = {0, 0, 0};
    if (lane < a.n) ray_nearest_lane<T, Leaf, Robust, Stats, Deep>(a, a.first + lane, lds, stride, tid, lane, cnt);
    if (Stats) add_counters(a.counters, cnt, tid);
}

} // namespace

template <typename T>
int launch_ray_nearest(const BvhImpl<T>& b, int leaf_kind, const T* d_prims, const T* d_rays, size_t n, unsigned k, unsigned flags,
                       typename HitOf<T>::Type* d_out_hits, uint32_t* d_counts, bvh_amd_counters* d_counters, hipStream_t stream) {
    using Hit = typename HitOf<T>::Type;
    if (k == 0 || k > BVH_AMD_RAY_NEAREST_MAX_K)
        return fail(BVH_AMD_ERR_ARG, "intersect_rays_nearest: k must be in [1, " + std::to_string(BVH_AMD_RAY_NEAREST_MAX_K) + "]");
    const bool aligned = !(misaligned(d_prims, 16) || misaligned(d_rays, 16) || misaligned(d_counters, 8) || misaligned(d_out_hits, sizeof(Hit)) ||
                           misaligned(d_counts, 4));
    if (const int rc = point_query_check(b, n, flags, d_prims && d_rays && d_out_hits,
                                         aligned ? nullptr : "device pointers must be aligned (prims and rays 16 bytes, counters 8, counts 4, hit records to their size)",
                                         "intersect_rays_nearest", BVH_AMD_RAY_ROBUST);
        rc || n == 0)
        return rc;
    const bool robust = (flags & BVH_AMD_RAY_ROBUST) != 0;
    const unsigned lanes = knn_block_lanes<T>(k);
    return point_query_run<T, kQueryRays>(b, d_prims, d_rays, n, flags, d_counters, sizeof(uint32_t) + sizeof(T), lanes, kPointSortMin, kPointKeyBits,
                                          "intersect_rays_nearest", stream, [&](const PointArgs<T>& args, T* deep_t) {
        const RayNearestArgs<T> a{args, d_out_hits, d_counts, deep_t, k};
        return point_query_dispatch(leaf_kind, d_counters != nullptr, a.deep_cap != 0, [&](auto leaf, auto stats, auto deep) {
            return robust ? point_query_launch(ray_nearest_kernel<T, leaf(), true, stats(), deep()>, a, lanes, knn_lds_bytes<T>(k, lanes), stream)
                          : point_query_launch(ray_nearest_kernel<T, leaf(), false, stats(), deep()>, a, lanes, knn_lds_bytes<T>(k, lanes), stream);
        });
    });
}

template int launch_ray_nearest<float>(const BvhImpl<float>&, int, const float*, const float*, size_t, unsigned, unsigned, bvh_hit3f*, uint32_t*,
                                       bvh_amd_counters*, hipStream_t);
template int launch_ray_nearest<double>(const BvhImpl<double>&, int, const double*, const double*, size_t, unsigned, unsigned, bvh_hit3d*, uint32_t*,
                                        bvh_amd_counters*, hipStream_t);

} // namespace bvh_amd
