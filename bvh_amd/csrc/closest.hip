// Batched closest-point queries for gfx950: for every query point {x, y, z, max_distance}, the BVH-order primitive nearest to it
// (PrecomputedTri or Sphere<T, 3>) within max_distance, and the distance. The per-lane walk and the distance functions are
// closest_body.inc (shared with the host test harness, tests/cpp/closest_body_host.cpp); this file holds the kernels and the launch.
//
// MI355X mapping:
//   * one lane per query, one-shot grid of ceil(n / 256) blocks: no ticket counter, so no work slot of the tree is claimed and any
//     number of launches of one const tree may run at once;
//   * depth-first walk over the 64 / 128-byte pair records (common.h: PairNode), nearer child first, the farther one stacked with its
//     box distance^2 so that a popped entry is re-checked against the best distance before anything is fetched;
//   * the stack: kClosestLds entries in LDS, the rest of 64 in per-lane scratch, beyond 64 (deep trees) in HBM;
//   * optionally the batch is read in the order of the Hilbert cell of each point in the root box (ray_key.h, radix sort): neighbouring
//     lanes then walk the same records (query_order.h). Records are always written in the caller's order.
//
// Compiled with -ffp-contract=off; division and sqrt are the correctly rounded forms (bit-identical to the host harness).

#include "common.h"
#include "trace_device.h"
#include "ray_key.h"
#include "query_order.h"
#include "closest_body.inc"

#include <algorithm>
#include <string>

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

// Reordering a batch costs a key pass and three radix passes (~0.03 ns per query) and pays once the batch is large enough for
// neighbouring queries to share records ("Closest-point queries": measured on the 1M soup / terrain / f64 spheres).
constexpr size_t kClosestSortMin = size_t{1} << 20;
// The HBM spill of trees deeper than 64 levels is sized per lane of a launch: batches are cut into launches of at most this many bytes of
// spill, or of one block when a single block needs more (a chain of 10^6 levels: ~2 GB).
constexpr size_t kClosestDeepBytes = size_t{256} << 20;
// Queries per launch: a grid stays below the runtime's 2^32 work-items (larger batches are cut into several launches).
constexpr size_t kClosestMaxLaunch = size_t{1} << 30;

template <typename T, int Leaf, bool Stats, bool Deep>
int launch_closest_variant(const ClosestArgs<T>& a, hipStream_t stream) {
    const unsigned long long blocks = (a.n + kBlock - 1) / kBlock;
    hipLaunchKernelGGL((closest_kernel<T, Leaf, Stats, Deep>), dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, stream, a);
    BVH_HIP_TRY(hipGetLastError(), BVH_AMD_ERR_HIP);
    return BVH_AMD_OK;
}

template <typename T, int Leaf>
int launch_closest_kind(const ClosestArgs<T>& a, bool stats, bool deep, hipStream_t stream) {
    if (deep) return stats ? launch_closest_variant<T, Leaf, true, true>(a, stream) : launch_closest_variant<T, Leaf, false, true>(a, stream);
    return stats ? launch_closest_variant<T, Leaf, true, false>(a, stream) : launch_closest_variant<T, Leaf, false, false>(a, stream);
}

bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }

} // namespace

template <typename T>
int launch_closest(const BvhImpl<T>& b, int leaf_kind, const T* d_prims, const T* d_queries, size_t n, unsigned flags,
                   typename HitOf<T>::Type* d_hits, bvh_amd_counters* d_counters, hipStream_t stream) {
    constexpr unsigned kAccepted = BVH_AMD_RAY_ORIGINAL_IDS | BVH_AMD_RAY_SORTED | BVH_AMD_RAY_UNSORTED;
    if (flags & ~kAccepted) return fail(BVH_AMD_ERR_ARG, "closest_points: unsupported flags (ORIGINAL_IDS, SORTED and UNSORTED only)");
    if (n == 0) return BVH_AMD_OK;
    if (b.dim != 3) return fail(BVH_AMD_ERR_ARG, "closest_points: 3D trees only");
    if (!d_prims || !d_queries || !d_hits) return fail(BVH_AMD_ERR_ARG, "closest_points: null device pointer");
    if (misaligned(d_prims) || misaligned(d_queries) || misaligned(d_hits) || (d_counters && (reinterpret_cast<uintptr_t>(d_counters) & 7u)))
        return fail(BVH_AMD_ERR_ARG, "closest_points: device pointers must be 16-byte aligned (counters 8-byte)");
    if (b.node_count == 0 || !b.d_work || (b.pair_count && !b.d_pairs)) return fail(BVH_AMD_ERR_ARG, "closest_points: BVH has no device copy");
    if ((flags & BVH_AMD_RAY_ORIGINAL_IDS) && !b.d_prim_ids) return fail(BVH_AMD_ERR_ARG, "closest_points: BVH has no device prim ids");

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

    ClosestArgs<T> a{};
    a.pairs = b.d_pairs; a.prims = d_prims; a.queries = d_queries; a.hits = d_hits;
    a.order = nullptr; a.prim_ids = (flags & BVH_AMD_RAY_ORIGINAL_IDS) ? b.d_prim_ids : nullptr;
    a.counters = d_counters; a.root_index = b.root_index;
    a.deep_nodes = nullptr; a.deep_d2 = nullptr; a.deep_cap = 0;

    // trees of more than 64 levels: an HBM spill of (depth - 64 + 1) entries per lane, launches cut to fit kClosestDeepBytes
    size_t per_launch = std::min(n, kClosestMaxLaunch);
    {
        const int rc = tree_depth<T>(b, stream);
        if (rc) return release(rc);
        const int max_depth = b.max_depth.load();
        if (max_depth > kClosestSmall) {
            const size_t cap = static_cast<size_t>(max_depth - kClosestSmall + 1);
            const size_t entry = sizeof(uint32_t) + sizeof(T);
            per_launch = std::max<size_t>(kBlock, kClosestDeepBytes / (cap * entry) / kBlock * kBlock);
            per_launch = std::min(per_launch, (std::min(n, kClosestMaxLaunch) + kBlock - 1) / kBlock * kBlock);
            const hipError_t e = scratch_alloc(&deep_mem, per_launch * cap * entry, &deep_tag);
            if (e != hipSuccess) { deep_mem = nullptr; return release(fail(BVH_AMD_ERR_HIP, std::string("closest_points: stack spill buffer: ") + hipGetErrorString(e))); }
            a.deep_d2 = static_cast<T*>(deep_mem);                                     // (T first: keeps the doubles 8-byte aligned)
            a.deep_nodes = reinterpret_cast<uint32_t*>(a.deep_d2 + per_launch * cap);
            a.deep_cap = static_cast<uint32_t>(cap);
        }
    }

    static const size_t sort_min = static_cast<size_t>(std::max(0, BVH_DEV_INT("BVH_AMD_CLOSEST_SORT_MIN", static_cast<int>(kClosestSortMin))));   // developer knob
    const bool reorder = n < (size_t{1} << 31) && ((flags & BVH_AMD_RAY_SORTED) ? n > 1 : (flags & BVH_AMD_RAY_UNSORTED) ? false : n >= sort_min);
    if (reorder) {
        static const int cell_bits = std::max(1, std::min(8, BVH_DEV_INT("BVH_AMD_CLOSEST_KEY_BITS", 7)));       // developer knob
        const int rc = query_order<T>(b, d_queries, n, cell_bits, "closest_points", stream, &sort_mem, &sort_tag, &a.order);
        if (rc) return release(rc);
    }

    const bool stats = d_counters != nullptr, deep = a.deep_cap != 0;
    for (size_t first = 0; first < n; first += per_launch) {
        a.first = first;
        a.n = std::min(per_launch, n - first);
        const int rc = leaf_kind == LEAF_TRIANGLE ? launch_closest_kind<T, LEAF_TRIANGLE>(a, stats, deep, stream)
                                                  : launch_closest_kind<T, LEAF_SPHERE>(a, stats, deep, stream);
        if (rc) return release(rc);
    }
    return release(BVH_AMD_OK);
}

template int launch_closest<float>(const BvhImpl<float>&, int, const float*, const float*, size_t, unsigned, bvh_hit3f*, bvh_amd_counters*, hipStream_t);
template int launch_closest<double>(const BvhImpl<double>&, int, const double*, const double*, size_t, unsigned, bvh_hit3d*, bvh_amd_counters*, hipStream_t);

} // namespace bvh_amd
