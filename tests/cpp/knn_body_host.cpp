// TEST INFRASTRUCTURE (CPU, no GPU): compiles the text of the k-nearest kernel — bvh_amd/csrc/knn_body.inc (over point_walk.inc,
// which has the distance functions) with the device helpers of bvh_amd/csrc/trace_device.h — for the HOST and runs it with
// one emulated lane per query (the queries of a batch one after another, or split over host threads), at any lane stride of the LDS
// arrays. What it can show: the walk of the very source the device runs returns the rows a brute force over the same distance
// functions returns, sorted and padded as the contract says; the device's rows, counts and counters must equal these bit for bit.
// What it cannot show: anything that needs the hardware. tests/test_knn_host.py drives it; tests/test_gpu_knn.py uses it too.
//
// Built by the tests with: g++ -std=c++20 -O1 -mavx2 -mfma -ffp-contract=off -fno-strict-aliasing -shared -fPIC -pthread.
#include <atomic>

#include "host_lane_prelude.h"
#include "../../bvh_amd/csrc/knn_body.inc"

namespace {

using namespace bvh_amd;

// One lane at a time, sitting at column (slot mod stride) of a block's LDS arrays: the other columns are never touched.
// The block's LDS is allocated at exactly knn_lds_bytes between two zones of sentinel words: false if a lane wrote outside it.
constexpr size_t kLdsGuardWords = 64;
constexpr unsigned long long kLdsSentinel = 0xA5A5A5A5A5A5A5A5ull;

template <typename T, int Leaf, bool Deep>
bool walk_range(const KnnArgs<T>& a0, uint32_t stride, unsigned long long begin, unsigned long long end, unsigned long long (&cnt)[3]) {
    KnnArgs<T> a = a0;
    const size_t words = knn_lds_bytes<T>(a.k, stride) / 8;                  // (a multiple of 8 bytes: stride is even)
    std::vector<unsigned long long> raw(words + 2 * kLdsGuardWords, kLdsSentinel);
    const KnnLds<T> lds = knn_lds_carve<T>(raw.data() + kLdsGuardWords, a.k, stride);
    std::vector<uint32_t> deep_nodes(Deep ? a.deep_cap : 1);
    std::vector<T> deep_d2(Deep ? a.deep_cap : 1);
    a.deep_nodes = deep_nodes.data();                                        // lane 0's spill
    a.deep_d2 = deep_d2.data();
    for (unsigned long long s = begin; s < end; ++s) knn_lane<T, Leaf, true, Deep>(a, s, lds, stride, int(s % stride), 0, cnt);
    for (size_t w = 0; w < kLdsGuardWords; ++w)
        if (raw[w] != kLdsSentinel || raw[kLdsGuardWords + words + w] != kLdsSentinel) return false;
    return true;
}

template <typename T, int Leaf>
int walk(const void* pairs, uint32_t root_index, const void* prims, const void* queries, size_t n, uint32_t k, uint32_t stride, const uint32_t* order,
         const uint32_t* prim_ids, uint32_t deep_cap, int threads, uint32_t* out_prims, void* out_dist, uint32_t* counts, unsigned long long* counters3) {
    if (k == 0 || k > BVH_AMD_KNN_MAX_K || stride == 0 || stride % 2 != 0) return 1;
    KnnArgs<T> a{};
    a.pairs = static_cast<const PairNode<T>*>(pairs); a.prims = static_cast<const T*>(prims); a.queries = static_cast<const T*>(queries);
    a.out_prims = out_prims; a.out_dist = static_cast<T*>(out_dist); a.counts = counts; a.k = k;
    a.n = n; a.first = 0; a.order = order; a.prim_ids = prim_ids; a.counters = nullptr;
    a.deep_cap = deep_cap; a.root_index = root_index;
    const int nt = std::max(1, threads);
    std::vector<std::thread> pool;
    std::vector<unsigned long long> sums(3 * size_t(nt), 0);
    std::atomic<bool> lds_overrun{false};
    for (int t = 0; t < nt; ++t) {
        const unsigned long long b = n * t / nt, e = n * (t + 1) / nt;
        pool.emplace_back([&, t, b, e] {
            unsigned long long cnt[3] = {0, 0, 0};
            const bool ok = deep_cap ? walk_range<T, Leaf, true>(a, stride, b, e, cnt) : walk_range<T, Leaf, false>(a, stride, b, e, cnt);
            if (!ok) lds_overrun = true;
            for (int j = 0; j < 3; ++j) sums[3 * size_t(t) + j] = cnt[j];
        });
    }
    for (auto& th : pool) th.join();
    for (int j = 0; j < 3; ++j) { counters3[j] = 0; for (int t = 0; t < nt; ++t) counters3[j] += sums[3 * size_t(t) + j]; }
    return lds_overrun ? 2 : 0;
}

// One launch of a sliced batch as the device runs it (prelude: GuardedSpill, run_slice): both spill arrays sized for the launch's
// lanes, one block's LDS (`stride` lanes wide, between its sentinels) shared by the launch.
template <typename T, int Leaf>
long long walk_slice(const void* pairs, uint32_t root_index, const void* prims, const void* queries, size_t first, size_t n, size_t launch_lanes, uint32_t k,
                     uint32_t stride, const uint32_t* order, const uint32_t* prim_ids, uint32_t deep_cap, uint32_t* out_prims, void* out_dist, uint32_t* counts,
                     unsigned long long* counters3) {
    if (k == 0 || k > BVH_AMD_KNN_MAX_K || stride == 0 || stride % 2 != 0 || deep_cap == 0 || n > launch_lanes) return kSliceBadArgs;
    KnnArgs<T> a{};
    a.pairs = static_cast<const PairNode<T>*>(pairs); a.prims = static_cast<const T*>(prims); a.queries = static_cast<const T*>(queries);
    a.out_prims = out_prims; a.out_dist = static_cast<T*>(out_dist); a.counts = counts; a.k = k;
    a.n = n; a.first = first; a.order = order; a.prim_ids = prim_ids; a.counters = nullptr;
    a.deep_cap = deep_cap; a.root_index = root_index;
    GuardedSpill<uint32_t> deep_nodes(first, launch_lanes, deep_cap);
    GuardedSpill<T> deep_d2(first, launch_lanes, deep_cap);
    a.deep_nodes = deep_nodes.data(); a.deep_d2 = deep_d2.data();
    const size_t words = knn_lds_bytes<T>(k, stride) / 8;
    std::vector<unsigned long long> raw(words + 2 * kLdsGuardWords, kLdsSentinel);
    const KnnLds<T> lds = knn_lds_carve<T>(raw.data() + kLdsGuardWords, k, stride);
    run_slice(n, stride, counters3, [&](unsigned long long lane, int tid, unsigned long long (&cnt)[3]) {
        knn_lane<T, Leaf, true, true>(a, first + lane, lds, stride, tid, lane, cnt);
    });
    for (size_t w = 0; w < kLdsGuardWords; ++w)
        if (raw[w] != kLdsSentinel || raw[kLdsGuardWords + words + w] != kLdsSentinel) return kSliceGuardBroken;
    if (!deep_nodes.guards_intact() || !deep_d2.guards_intact()) return kSliceGuardBroken;
    return deep_nodes.overwritten() + deep_d2.overwritten();
}

} // namespace

extern "C" {

// The kernel's walk for n queries {x, y, z, max_distance} (slot s reads query order[s], or s), k slots per row, the LDS arrays
// `stride` lanes wide; leaf 0 = triangles, 1 = spheres; prim_ids (optional) = BVH_AMD_RAY_ORIGINAL_IDS; deep_cap > 0: the HBM spill of
// trees deeper than 64 levels, deep_cap entries. out_prims (n x k), out_dist (optional), counts (optional) as in the C ABI;
// counters3 = {pairs fetched, primitives tested, leaves visited}. Returns 0 (1: k or stride out of range; 2: a lane wrote outside the
// block's LDS).
int knn_host_walk(int is_double, int leaf, const void* pairs, uint32_t root_index, const void* prims, const void* queries, size_t n, uint32_t k,
                  uint32_t stride, const uint32_t* order, const uint32_t* prim_ids, uint32_t deep_cap, int threads, uint32_t* out_prims, void* out_dist,
                  uint32_t* counts, unsigned long long* counters3) {
    if (is_double) {
        if (leaf == LEAF_SPHERE) return walk<double, LEAF_SPHERE>(pairs, root_index, prims, queries, n, k, stride, order, prim_ids, deep_cap, threads, out_prims, out_dist, counts, counters3);
        return walk<double, LEAF_TRIANGLE>(pairs, root_index, prims, queries, n, k, stride, order, prim_ids, deep_cap, threads, out_prims, out_dist, counts, counters3);
    }
    if (leaf == LEAF_SPHERE) return walk<float, LEAF_SPHERE>(pairs, root_index, prims, queries, n, k, stride, order, prim_ids, deep_cap, threads, out_prims, out_dist, counts, counters3);
    return walk<float, LEAF_TRIANGLE>(pairs, root_index, prims, queries, n, k, stride, order, prim_ids, deep_cap, threads, out_prims, out_dist, counts, counters3);
}

// One launch of a batch that point_query_run cut into slices (deep_cap > 0): slots [first, first + n) as the device walks them —
// a.first = first, slot = first + lane, lane = 0 .. n-1 indexing spill arrays of launch_lanes * deep_cap entries that the launch's
// lanes share, tid = lane % stride in one block's LDS. queries, order and the outputs are the whole batch's. Returns the spill
// entries the launch overwrote (both arrays), -1 if a guard zone around a spill array or the LDS was written to, -2 for arguments
// out of range (k, stride, deep_cap == 0, n > launch_lanes).
long long knn_host_walk_slice(int is_double, int leaf, const void* pairs, uint32_t root_index, const void* prims, const void* queries, size_t first, size_t n,
                              size_t launch_lanes, uint32_t k, uint32_t stride, const uint32_t* order, const uint32_t* prim_ids, uint32_t deep_cap,
                              uint32_t* out_prims, void* out_dist, uint32_t* counts, unsigned long long* counters3) {
    if (is_double) {
        if (leaf == LEAF_SPHERE) return walk_slice<double, LEAF_SPHERE>(pairs, root_index, prims, queries, first, n, launch_lanes, k, stride, order, prim_ids, deep_cap, out_prims, out_dist, counts, counters3);
        return walk_slice<double, LEAF_TRIANGLE>(pairs, root_index, prims, queries, first, n, launch_lanes, k, stride, order, prim_ids, deep_cap, out_prims, out_dist, counts, counters3);
    }
    if (leaf == LEAF_SPHERE) return walk_slice<float, LEAF_SPHERE>(pairs, root_index, prims, queries, first, n, launch_lanes, k, stride, order, prim_ids, deep_cap, out_prims, out_dist, counts, counters3);
    return walk_slice<float, LEAF_TRIANGLE>(pairs, root_index, prims, queries, first, n, launch_lanes, k, stride, order, prim_ids, deep_cap, out_prims, out_dist, counts, counters3);
}

} // extern "C"
