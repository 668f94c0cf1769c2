// Batched k-nearest-primitive queries for gfx950: for every query point {x, y, z, max_distance}, the k BVH-order primitives
// (PrecomputedTri or Sphere<T, 3>) at the smallest (squared distance, index) within max_distance, in ascending order, as one row of k
// slots. The per-lane walk and the candidate set are knn_body.inc (shared with the host test harness, tests/cpp/knn_body_host.cpp)
// over point_walk.inc (distance functions, stack); the launch path is point_query.h's; this file holds the kernel and what is specific
// to the query.
//
// MI355X mapping:
//   * one lane per query, one-shot grid: no ticket counter, so no work slot of the tree is claimed and any number of launches of one
//     const tree may run at once;
//   * closest.hip's walk (nearer child first, the farther one stacked with its box distance^2), pruned against the worst of the k
//     candidates held instead of the best;
//   * the candidates: a binary max-heap of k {d2, index} per lane in LDS, [slot][lane] arrays (a lane's bank does not depend on the
//     slot), the worst pair and the fill count in registers; heapsorted in place at the end and written as one row;
//   * k is a run-time argument: the LDS is dynamic, (k + kKnnLds) * (sizeof(T) + 4) bytes per lane, and a block has 256, 128 or 64
//     lanes, whichever keeps the most queries resident on a CU for that k (knn_lanes.h: knn_block_lanes);
//   * the stack: kKnnLds entries in LDS, the rest of 64 in per-lane scratch, beyond 64 (deep trees) in HBM (point_walk.inc);
//   * optionally the batch is read in the order of the Hilbert cell of each point in the root box (query_order.h). Rows are always
//     written in the caller's order.
//
// Compiled with -ffp-contract=off; division and sqrt are the correctly rounded forms (bit-identical to the host harness).

#include "common.h"
#include "trace_device.h"
#include "ray_key.h"
#include "query_order.h"
#include "knn_body.inc"
#include "point_query.h"
#include "knn_lanes.h"

namespace bvh_amd {

namespace {

template <typename T, int Leaf, bool Stats, bool Deep>
__global__ void __launch_bounds__(kBlock) knn_kernel(KnnArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_lds_raw[];
    const uint32_t stride = blockDim.x;
    const KnnLds<T> lds = knn_lds_carve<T>(knn_lds_raw, a.k, stride);
    const int tid = threadIdx.x;
    const unsigned long long lane = static_cast<unsigned long long>(blockIdx.x) * stride + tid;
    unsigned long long cnt[3] = {0, 0, 0};
    if (lane < a.n) knn_lane<T, Leaf, Stats, Deep>(a, a.first + lane, lds, stride, tid, lane, cnt);
    if (Stats) add_counters(a.counters, cnt, tid);
}

} // namespace

template <typename T>
int launch_knn(const BvhImpl<T>& b, int leaf_kind, const T* d_prims, const T* d_queries, size_t n, unsigned k, unsigned flags, uint32_t* d_out_prims,
               T* d_out_dist, uint32_t* d_counts, bvh_amd_counters* d_counters, hipStream_t stream) {
    if (k == 0 || k > BVH_AMD_KNN_MAX_K) return fail(BVH_AMD_ERR_ARG, "knn: k must be in [1, " + std::to_string(BVH_AMD_KNN_MAX_K) + "]");
    const bool aligned = !(misaligned(d_prims, 16) || misaligned(d_queries, 16) || misaligned(d_counters, 8) || misaligned(d_out_prims, 4) ||
                           misaligned(d_out_dist, sizeof(T)) || misaligned(d_counts, 4));
    if (const int rc = point_query_check(b, n, flags, d_prims && d_queries && d_out_prims,
                                         aligned ? nullptr : "device pointers must be aligned (prims and queries 16 bytes, counters 8, the outputs to their element)",
                                         "knn");
        rc || n == 0)
        return rc;
    const unsigned lanes = knn_block_lanes<T>(k);
    return point_query_run<T>(b, d_prims, d_queries, n, flags, d_counters, sizeof(uint32_t) + sizeof(T), lanes, kPointSortMin, kPointKeyBits, "knn", stream,
                              [&](const PointArgs<T>& args, T* deep_d2) {
        const KnnArgs<T> a{args, d_out_prims, d_out_dist, d_counts, deep_d2, k};
        return point_query_dispatch(leaf_kind, d_counters != nullptr, a.deep_cap != 0, [&](auto leaf, auto stats, auto deep) {
            return point_query_launch(knn_kernel<T, leaf(), stats(), deep()>, a, lanes, knn_lds_bytes<T>(k, lanes), stream);
        });
    });
}

template int launch_knn<float>(const BvhImpl<float>&, int, const float*, const float*, size_t, unsigned, unsigned, uint32_t*, float*, uint32_t*,
                               bvh_amd_counters*, hipStream_t);
template int launch_knn<double>(const BvhImpl<double>&, int, const double*, const double*, size_t, unsigned, unsigned, uint32_t*, double*, uint32_t*,
                                bvh_amd_counters*, hipStream_t);

} // namespace bvh_amd
