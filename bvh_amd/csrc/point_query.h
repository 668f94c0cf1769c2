// The launch path of the batched point, box, triangle, region and ray list / row queries (closest.hip, radius.hip, knn.hip, overlap.hip,
// tri_intersect.hip, tri_distance.hip, region.hip, winding.hip, ray_hits.hip, ray_nearest.hip, sphere_cast.hip; instanced.hip takes
// its thresholds, misaligned, the launch and the counter epilogue), once: the thresholds, the
// argument checks they share, the driver (counters, depth pass, HBM spill, reading order, launches), the output check and the Fill
// switch of the list queries, and the kernels' counter epilogue. Expects common.h,
// trace_device.h, ray_key.h, query_order.h and the kind's body (point_walk.inc: PointArgs) to have been included.
#pragma once

#include <algorithm>
#include <string>
#include <type_traits>

namespace bvh_amd {

namespace {

// Reordering a batch costs a key pass and three radix passes (~0.03 ns per query) and pays once the batch is large enough for
// neighbouring queries to share records ("Closest-point queries": measured on the 1M soup / terrain / f64 spheres; not
// measured for radius and k-nearest queries, which take the same threshold).
constexpr size_t kPointSortMin = size_t{1} << 20;
constexpr int kPointKeyBits = 7;                              // 2^7 Hilbert cells per axis of the root box
// The HBM spill of trees deeper than 64 levels is sized per lane of a launch: batches are cut into launches of at most this many bytes of
// spill, or of one block when a single block needs more (a chain of 10^6 levels: ~2 GB).
constexpr size_t kPointDeepBytes = size_t{256} << 20;
// Queries per launch: a grid stays below the runtime's 2^32 work-items (larger batches are cut into several launches).
constexpr size_t kPointMaxLaunch = size_t{1} << 30;

inline bool misaligned(const void* p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) != 0; }

// The checks of a point query `who`, in their order: the flags, (an empty batch is accepted here: the caller returns when rc || n == 0,)
// the tree's dimension, `required` (the pointers the kind cannot do without are there), `fault` (what the kind's own checks of its
// pointers found, or null), the tree's device copy. `more_flags`: bits this kind alone accepts (ray_hits.hip: BVH_AMD_RAY_ROBUST).
template <typename T>
int point_query_check(const BvhImpl<T>& b, size_t n, unsigned flags, bool required, const char* fault, const std::string& who, unsigned more_flags = 0u) {
    constexpr unsigned kAccepted = BVH_AMD_RAY_ORIGINAL_IDS | BVH_AMD_RAY_SORTED | BVH_AMD_RAY_UNSORTED;
    if (flags & ~(kAccepted | more_flags))
        return fail(BVH_AMD_ERR_ARG, who + (more_flags & BVH_AMD_RAY_ROBUST ? ": unsupported flags (ROBUST, ORIGINAL_IDS, SORTED and UNSORTED only)"
                                                                            : ": unsupported flags (ORIGINAL_IDS, SORTED and UNSORTED only)"));
    if (n == 0) return BVH_AMD_OK;
    if (b.dim != 3) return fail(BVH_AMD_ERR_ARG, who + ": 3D trees only");
    if (!required) return fail(BVH_AMD_ERR_ARG, who + ": null device pointer");
    if (fault) return fail(BVH_AMD_ERR_ARG, who + ": " + fault);
    if (b.node_count == 0 || !b.d_work || (b.pair_count && !b.d_pairs)) return fail(BVH_AMD_ERR_ARG, who + ": BVH has no device copy");
    if ((flags & BVH_AMD_RAY_ORIGINAL_IDS) && !b.d_prim_ids) return fail(BVH_AMD_ERR_ARG, who + ": BVH has no device prim ids");
    return BVH_AMD_OK;
}

// Runs a checked, non-empty batch: zeroes the counters, sizes the HBM spill of a tree deeper than kPointSmall levels (`entry` bytes
// per stack entry: a node word and whatever the kind keeps beside it; launches are cut to whole blocks of `lanes`), sorts the batch
// when asked to or, left to itself, from sort_min queries on, and calls launch(args, deep_d2) for every slice: args holds what the
// kinds share, deep_d2 the spill's other array (entry - 4 bytes per entry; null for a shallow tree). Owns the scratch behind both.
// kQueryBoxes (overlap.hip): a query is a box of 6 scalars, ordered by the cell of its centre; d_queries may then be null when the batch is
// not reordered (self mode: the lanes take their boxes from d_prims). kQueryRays (ray_hits.hip): a query is a ray of 8 scalars, ordered
// by the cell of its origin and the octant of its direction. kQueryTris (tri_intersect.hip): a query is a triangle of 9 scalars, ordered by the
// cell of its box's centre; self mode as for kQueryBoxes.
template <typename T, int Kind = kQueryPoints, typename Launch>
int point_query_run(const BvhImpl<T>& b, const T* d_prims, const T* d_queries, size_t n, unsigned flags, bvh_amd_counters* d_counters, size_t entry,
                    size_t lanes, size_t sort_min, int key_bits, const char* who, hipStream_t stream, Launch launch) {
    StreamScope scope(stream);
    set_last_query_launches(0);                               // (bvh_amd_last_query_launches: counted below, one per launch)
    void* deep_mem = nullptr;
    void* sort_mem = nullptr;
    ScratchTag deep_tag, sort_tag;
    auto release = [&](int rc) {
        if (deep_mem) scratch_free(deep_mem, deep_tag);
        if (sort_mem) scratch_free(sort_mem, sort_tag);
        return rc;
    };
    if (d_counters) BVH_HIP_TRY(hipMemsetAsync(d_counters, 0, sizeof(bvh_amd_counters), stream), BVH_AMD_ERR_HIP);

    PointArgs<T> a{};
    a.pairs = b.d_pairs; a.prims = d_prims; a.queries = d_queries;
    a.prim_ids = (flags & BVH_AMD_RAY_ORIGINAL_IDS) ? b.d_prim_ids : nullptr;
    a.counters = d_counters; a.root_index = b.root_index;

    // trees of more than 64 levels: an HBM spill of (depth - 64 + 1) entries per lane, launches cut to fit kPointDeepBytes
    size_t per_launch = std::min(n, kPointMaxLaunch);
    const int rc_depth = tree_depth<T>(b, stream);
    if (rc_depth) return release(rc_depth);
    const int max_depth = b.max_depth.load();
    if (max_depth > kPointSmall) {
        const size_t cap = static_cast<size_t>(max_depth - kPointSmall + 1);
        per_launch = std::max<size_t>(lanes, kPointDeepBytes / (cap * entry) / lanes * lanes);
        per_launch = std::min(per_launch, (std::min(n, kPointMaxLaunch) + lanes - 1) / lanes * lanes);
        const hipError_t e = scratch_alloc(&deep_mem, per_launch * cap * entry, &deep_tag);
        if (e != hipSuccess) { deep_mem = nullptr; return release(fail(BVH_AMD_ERR_HIP, std::string(who) + ": stack spill buffer: " + hipGetErrorString(e))); }
        // (the other array first: keeps doubles 8-byte aligned)
        a.deep_nodes = reinterpret_cast<uint32_t*>(static_cast<char*>(deep_mem) + per_launch * cap * (entry - sizeof(uint32_t)));
        a.deep_cap = static_cast<uint32_t>(cap);
    }

    const bool reorder = n < (size_t{1} << 31) && ((flags & BVH_AMD_RAY_SORTED) ? n > 1 : (flags & BVH_AMD_RAY_UNSORTED) ? false : n >= sort_min);
    if (reorder) {
        const int rc = query_order<T, Kind>(b, d_queries, n, key_bits, who, stream, &sort_mem, &sort_tag, &a.order);
        if (rc) return release(rc);
    }

    int launches = 0;
    for (size_t first = 0; first < n; first += per_launch) {
        a.first = first;
        a.n = std::min(per_launch, n - first);
        const int rc = launch(a, static_cast<T*>(deep_mem));
        if (rc) return release(rc);
        set_last_query_launches(++launches);
    }
    return release(BVH_AMD_OK);
}

// The Stats / Deep / leaf ladder of one slice: calls f(leaf, stats, deep) with the three run-time choices as compile-time constants
// (std::integral_constant), for f to launch the kind's kernel <T, leaf(), stats(), deep()> with point_query_launch.
template <typename F>
int point_query_dispatch(int leaf_kind, bool stats, bool deep, F f) {
    auto leaf = [&](auto s, auto d) {
        return leaf_kind == LEAF_TRIANGLE ? f(std::integral_constant<int, LEAF_TRIANGLE>{}, s, d) : f(std::integral_constant<int, LEAF_SPHERE>{}, s, d);
    };
    if (deep) return stats ? leaf(std::true_type{}, std::true_type{}) : leaf(std::false_type{}, std::true_type{});
    return stats ? leaf(std::true_type{}, std::false_type{}) : leaf(std::false_type{}, std::false_type{});
}

// The list queries (radius.hip, overlap.hip, ray_hits.hip) have one more choice: f(leaf, stats, deep, fill), fill = the launch has offsets and
// writes lists (the kernels <..., Fill = true>).
template <typename F>
int list_query_dispatch(int leaf_kind, bool stats, bool deep, bool fill, F f) {
    return point_query_dispatch(leaf_kind, stats, deep, [&](auto leaf, auto s, auto d) {
        return fill ? f(leaf, s, d, std::true_type{}) : f(leaf, s, d, std::false_type{});
    });
}

// What is wrong with the output pointers of a list query, or null: `fault` of point_query_check, ahead of the kind's own alignment
// message. list_extra: the kind's other list array (radius search's distances), or null.
inline const char* list_output_fault(const void* d_counts, const void* d_offsets, const void* d_list_prims, const void* list_extra) {
    return !d_counts && !d_offsets                     ? "at least one of d_counts and d_offsets is required"
           : d_offsets && !d_list_prims                ? "d_offsets needs d_list_prims"
           : !d_offsets && (d_list_prims || list_extra) ? "lists need d_offsets"
                                                       : nullptr;
}

template <typename Args>
int point_query_launch(void (*kernel)(Args), const Args& a, unsigned lanes, size_t lds_bytes, hipStream_t stream) {
    const unsigned long long blocks = (a.n + lanes - 1) / lanes;
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(blocks)), dim3(lanes), lds_bytes, stream, a);
    BVH_HIP_TRY(hipGetLastError(), BVH_AMD_ERR_HIP);
    return BVH_AMD_OK;
}

// The end of a Stats kernel: cnt = {pair records fetched, primitives tested, leaves visited} of this lane, summed over the wave, one
// atomic per counter and wave.
__device__ inline void add_counters(bvh_amd_counters* counters, unsigned long long (&cnt)[3], int tid) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        cnt[0] += __shfl_down(cnt[0], off);
        cnt[1] += __shfl_down(cnt[1], off);
        cnt[2] += __shfl_down(cnt[2], off);
    }
    if ((tid & (kWave - 1)) == 0) {
        atomicAdd(&counters->node_pairs, cnt[0]);
        atomicAdd(&counters->prim_tests, cnt[1]);
        atomicAdd(&counters->leaves, cnt[2]);
    }
}

} // namespace

} // namespace bvh_amd
