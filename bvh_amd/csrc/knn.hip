// Batched k-nearest-primitive queries for gfx950: for every query point {x, y, z, max_distance}, the k BVH-order primitives
// (PrecomputedTri or Sphere<T, 3>) at the smallest (squared distance, index) within max_distance, in ascending order, as one row of k
// slots. The per-lane walk and the candidate set are knn_body.inc (shared with the host test harness, tests/cpp/knn_body_host.cpp),
// the distance functions are closest_body.inc's; this file holds the kernels and the launch.
//
// MI355X mapping:
//   * one lane per query, one-shot grid: no ticket counter, so no work slot of the tree is claimed and any number of launches of one
//     const tree may run at once;
//   * closest.hip's walk (nearer child first, the farther one stacked with its box distance^2), pruned against the worst of the k
//     candidates held instead of the best;
//   * the candidates: a binary max-heap of k {d2, index} per lane in LDS, [slot][lane] arrays (a lane's bank does not depend on the
//     slot), the worst pair and the fill count in registers; heapsorted in place at the end and written as one row;
//   * k is a run-time argument: the LDS is dynamic, (k + kKnnLds) * (sizeof(T) + 4) bytes per lane, and a block has 256, 128 or 64
//     lanes, whichever keeps the most queries resident on a CU for that k (knn_block_lanes);
//   * the stack: kKnnLds entries in LDS, the rest of 64 in per-lane scratch, beyond 64 (deep trees) in HBM;
//   * optionally the batch is read in the order of the Hilbert cell of each point in the root box (query_order.h). Rows are always
//     written in the caller's order.
//
// Compiled with -ffp-contract=off; division and sqrt are the correctly rounded forms (bit-identical to the host harness).

#include "common.h"
#include "trace_device.h"
#include "ray_key.h"
#include "query_order.h"
#include "knn_body.inc"

#include <algorithm>
#include <string>

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
    if (Stats) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            cnt[0] += __shfl_down(cnt[0], off);
            cnt[1] += __shfl_down(cnt[1], off);
            cnt[2] += __shfl_down(cnt[2], off);
        }
        if ((tid & (kWave - 1)) == 0) {
            atomicAdd(&a.counters->node_pairs, cnt[0]);
            atomicAdd(&a.counters->prim_tests, cnt[1]);
            atomicAdd(&a.counters->leaves, cnt[2]);
        }
    }
}

// Lanes per block: of 256 / 128 / 64, the size that keeps the most lanes resident on a CU — whole blocks of (k + kKnnLds) *
// (sizeof(T) + 4) bytes per lane in the 160 KB of LDS, a block within 64 KB, at most 8 waves per SIMD — ties to the larger block. The
// LDS a lane needs is fixed by k; the block size only decides how much of the CU's LDS the rounding to whole blocks wastes, so the
// choice is not monotonic in k: floats take 256 lanes at k = 1, 8, 17, 128 at k = 9, 32 and 64 at k = 16, 33 .. 64; doubles 256 at
// k = 5, 9, 128 at k = 7, 16, 17 and 64 at k = 1, 8, 32 .. 64 ("k-nearest queries", has the table).
constexpr size_t kKnnBlockLds = size_t{64} << 10;
constexpr size_t kKnnCuLds = size_t{160} << 10;
constexpr size_t kKnnCuLanes = 8 * 4 * kWave;
template <typename T>
unsigned knn_block_lanes(unsigned k) {
    unsigned best = kWave;
    size_t best_resident = 0;
    for (unsigned lanes = kBlock; lanes >= unsigned(kWave); lanes /= 2) {
        const size_t bytes = knn_lds_bytes<T>(k, lanes);
        if (bytes > kKnnBlockLds) continue;
        const size_t resident = std::min(kKnnCuLds / bytes * lanes, kKnnCuLanes);
        if (resident > best_resident) { best = lanes; best_resident = resident; }
    }
    return best;
}

// The thresholds of closest.hip (kClosestSortMin, kClosestDeepBytes, kClosestMaxLaunch), by the same reasoning.
constexpr size_t kKnnSortMin = size_t{1} << 20;
constexpr size_t kKnnDeepBytes = size_t{256} << 20;
constexpr size_t kKnnMaxLaunch = size_t{1} << 30;
constexpr int kKnnKeyBits = 7;

template <typename T, int Leaf, bool Stats, bool Deep>
int launch_knn_variant(const KnnArgs<T>& a, unsigned lanes, hipStream_t stream) {
    const unsigned long long blocks = (a.n + lanes - 1) / lanes;
    hipLaunchKernelGGL((knn_kernel<T, Leaf, Stats, Deep>), dim3(static_cast<unsigned>(blocks)), dim3(lanes), knn_lds_bytes<T>(a.k, lanes), stream, a);
    BVH_HIP_TRY(hipGetLastError(), BVH_AMD_ERR_HIP);
    return BVH_AMD_OK;
}

template <typename T, int Leaf>
int launch_knn_kind(const KnnArgs<T>& a, unsigned lanes, bool stats, bool deep, hipStream_t stream) {
    if (deep) return stats ? launch_knn_variant<T, Leaf, true, true>(a, lanes, stream) : launch_knn_variant<T, Leaf, false, true>(a, lanes, stream);
    return stats ? launch_knn_variant<T, Leaf, true, false>(a, lanes, stream) : launch_knn_variant<T, Leaf, false, false>(a, lanes, stream);
}

bool misaligned(const void* p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) != 0; }

} // namespace

template <typename T>
int launch_knn(const BvhImpl<T>& b, int leaf_kind, const T* d_prims, const T* d_queries, size_t n, unsigned k, unsigned flags, uint32_t* d_out_prims,
               T* d_out_dist, uint32_t* d_counts, bvh_amd_counters* d_counters, hipStream_t stream) {
    constexpr unsigned kAccepted = BVH_AMD_RAY_ORIGINAL_IDS | BVH_AMD_RAY_SORTED | BVH_AMD_RAY_UNSORTED;
    if (flags & ~kAccepted) return fail(BVH_AMD_ERR_ARG, "knn: unsupported flags (ORIGINAL_IDS, SORTED and UNSORTED only)");
    if (k == 0 || k > BVH_AMD_KNN_MAX_K) return fail(BVH_AMD_ERR_ARG, "knn: k must be in [1, " + std::to_string(BVH_AMD_KNN_MAX_K) + "]");
    if (n == 0) return BVH_AMD_OK;
    if (b.dim != 3) return fail(BVH_AMD_ERR_ARG, "knn: 3D trees only");
    if (!d_prims || !d_queries || !d_out_prims) return fail(BVH_AMD_ERR_ARG, "knn: null device pointer");
    if (misaligned(d_prims, 16) || misaligned(d_queries, 16) || misaligned(d_counters, 8) || misaligned(d_out_prims, 4) || misaligned(d_out_dist, sizeof(T)) ||
        misaligned(d_counts, 4))
        return fail(BVH_AMD_ERR_ARG, "knn: device pointers must be aligned (prims and queries 16 bytes, counters 8, the outputs to their element)");
    if (b.node_count == 0 || !b.d_work || (b.pair_count && !b.d_pairs)) return fail(BVH_AMD_ERR_ARG, "knn: BVH has no device copy");
    if ((flags & BVH_AMD_RAY_ORIGINAL_IDS) && !b.d_prim_ids) return fail(BVH_AMD_ERR_ARG, "knn: BVH has no device prim ids");

    StreamScope scope(stream);
    void* deep_mem = nullptr;
    void* sort_mem = nullptr;
    ScratchTag deep_tag, sort_tag;
    auto release = [&](int rc) {
        if (deep_mem) scratch_free(deep_mem, deep_tag);
        if (sort_mem) scratch_free(sort_mem, sort_tag);
        return rc;
    };
    if (d_counters) BVH_HIP_TRY(hipMemsetAsync(d_counters, 0, sizeof(bvh_amd_counters), stream), BVH_AMD_ERR_HIP);

    KnnArgs<T> a{};
    a.pairs = b.d_pairs; a.prims = d_prims; a.queries = d_queries;
    a.out_prims = d_out_prims; a.out_dist = d_out_dist; a.counts = d_counts; a.k = k;
    a.order = nullptr; a.prim_ids = (flags & BVH_AMD_RAY_ORIGINAL_IDS) ? b.d_prim_ids : nullptr;
    a.counters = d_counters; a.root_index = b.root_index;
    a.deep_nodes = nullptr; a.deep_d2 = nullptr; a.deep_cap = 0;
    const unsigned lanes = knn_block_lanes<T>(k);

    // trees of more than 64 levels: an HBM spill of (depth - 64 + 1) entries per lane, launches cut to whole blocks that fit kKnnDeepBytes
    size_t per_launch = std::min(n, kKnnMaxLaunch);
    {
        const int rc = tree_depth<T>(b, stream);
        if (rc) return release(rc);
        const int max_depth = b.max_depth.load();
        if (max_depth > kKnnSmall) {
            const size_t cap = static_cast<size_t>(max_depth - kKnnSmall + 1);
            const size_t entry = sizeof(uint32_t) + sizeof(T);
            per_launch = std::max<size_t>(lanes, kKnnDeepBytes / (cap * entry) / lanes * lanes);
            per_launch = std::min(per_launch, (std::min(n, kKnnMaxLaunch) + lanes - 1) / lanes * lanes);
            const hipError_t e = scratch_alloc(&deep_mem, per_launch * cap * entry, &deep_tag);
            if (e != hipSuccess) { deep_mem = nullptr; return release(fail(BVH_AMD_ERR_HIP, std::string("knn: stack spill buffer: ") + hipGetErrorString(e))); }
            a.deep_d2 = static_cast<T*>(deep_mem);                                     // (T first: keeps the doubles 8-byte aligned)
            a.deep_nodes = reinterpret_cast<uint32_t*>(a.deep_d2 + per_launch * cap);
            a.deep_cap = static_cast<uint32_t>(cap);
        }
    }

    const bool reorder = n < (size_t{1} << 31) && ((flags & BVH_AMD_RAY_SORTED) ? n > 1 : (flags & BVH_AMD_RAY_UNSORTED) ? false : n >= kKnnSortMin);
    if (reorder) {
        const int rc = query_order<T>(b, d_queries, n, kKnnKeyBits, "knn", stream, &sort_mem, &sort_tag, &a.order);
        if (rc) return release(rc);
    }

    const bool stats = d_counters != nullptr, deep = a.deep_cap != 0;
    for (size_t first = 0; first < n; first += per_launch) {
        a.first = first;
        a.n = std::min(per_launch, n - first);
        const int rc = leaf_kind == LEAF_TRIANGLE ? launch_knn_kind<T, LEAF_TRIANGLE>(a, lanes, stats, deep, stream)
                                                  : launch_knn_kind<T, LEAF_SPHERE>(a, lanes, stats, deep, stream);
        if (rc) return release(rc);
    }
    return release(BVH_AMD_OK);
}

template int launch_knn<float>(const BvhImpl<float>&, int, const float*, const float*, size_t, unsigned, unsigned, uint32_t*, float*, uint32_t*,
                               bvh_amd_counters*, hipStream_t);
template int launch_knn<double>(const BvhImpl<double>&, int, const double*, const double*, size_t, unsigned, unsigned, uint32_t*, double*, uint32_t*,
                                bvh_amd_counters*, hipStream_t);

} // namespace bvh_amd
