// TEST INFRASTRUCTURE (CPU, no GPU): compiles the text of the radius-query kernel — bvh_amd/csrc/radius_body.inc (over list_walk.inc, the walk it
// shares with the overlap query, and point_walk.inc, which has the distance functions) with the device helpers of bvh_amd/csrc/trace_device.h — for the HOST and runs it with
// one emulated lane per query (the queries of a batch one after another, or split over host threads). What it can show: the walk of
// the very source the device runs lists the primitives a brute force over the same distance functions lists, in the tree's order, and
// keeps to its segment; the device's counts, lists and distances must equal these bit for bit. What it cannot show: anything that
// needs the hardware. tests/test_radius_search_host.py drives it; tests/test_gpu_radius_search.py uses it too.
//
// Built by the tests with: g++ -std=c++20 -O1 -mavx2 -mfma -ffp-contract=off -fno-strict-aliasing -shared -fPIC -pthread.
#include "host_lane_prelude.h"
#include "../../bvh_amd/csrc/radius_body.inc"

namespace {

using namespace bvh_amd;

template <typename T, int Leaf, bool Deep>
void walk_range(const RadiusArgs<T>& a0, unsigned long long begin, unsigned long long end, unsigned long long (&cnt)[3]) {
    RadiusArgs<T> a = a0;
    std::vector<uint32_t> lds_node(size_t(kRadiusLds) * kBlock);
    std::vector<uint32_t> deep_nodes(Deep ? a.deep_cap : 1);
    a.deep_nodes = deep_nodes.data();                                        // one lane at a time: lane 0's spill
    for (unsigned long long s = begin; s < end; ++s) {
        if (a.offsets) radius_lane<T, Leaf, true, Deep, true>(a, s, lds_node.data(), 0, 0, cnt);
        else radius_lane<T, Leaf, true, Deep, false>(a, s, lds_node.data(), 0, 0, cnt);
    }
}

template <typename T, int Leaf>
int walk(const void* pairs, uint32_t root_index, const void* prims, const void* queries, size_t n, const uint32_t* order, const uint32_t* prim_ids,
         uint32_t deep_cap, int threads, uint32_t* counts, const uint64_t* offsets, uint32_t* list_prims, void* list_dist, unsigned long long* counters3) {
    RadiusArgs<T> a{};
    a.pairs = static_cast<const PairNode<T>*>(pairs); a.prims = static_cast<const T*>(prims); a.queries = static_cast<const T*>(queries);
    a.counts = counts; a.offsets = reinterpret_cast<const unsigned long long*>(offsets); a.list_prims = list_prims; a.list_dist = static_cast<T*>(list_dist);
    a.n = n; a.first = 0; a.order = order; a.prim_ids = prim_ids; a.counters = nullptr;
    a.deep_cap = deep_cap; a.root_index = root_index;
    run_lanes(n, threads, counters3, [&](unsigned long long b, unsigned long long e, unsigned long long (&cnt)[3]) {
        if (deep_cap) walk_range<T, Leaf, true>(a, b, e, cnt); else walk_range<T, Leaf, false>(a, b, e, cnt);
    });
    return 0;
}

// One launch of a sliced batch as the device runs it (prelude: GuardedSpill, run_slice): the spill sized for the launch's lanes.
template <typename T, int Leaf>
long long walk_slice(const void* pairs, uint32_t root_index, const void* prims, const void* queries, size_t first, size_t n, size_t launch_lanes,
                     const uint32_t* order, const uint32_t* prim_ids, uint32_t deep_cap, uint32_t* counts, const uint64_t* offsets, uint32_t* list_prims,
                     void* list_dist, unsigned long long* counters3) {
    if (deep_cap == 0 || n > launch_lanes) return kSliceBadArgs;
    RadiusArgs<T> a{};
    a.pairs = static_cast<const PairNode<T>*>(pairs); a.prims = static_cast<const T*>(prims); a.queries = static_cast<const T*>(queries);
    a.counts = counts; a.offsets = reinterpret_cast<const unsigned long long*>(offsets); a.list_prims = list_prims; a.list_dist = static_cast<T*>(list_dist);
    a.n = n; a.first = first; a.order = order; a.prim_ids = prim_ids; a.counters = nullptr;
    a.deep_cap = deep_cap; a.root_index = root_index;
    GuardedSpill<uint32_t> deep_nodes(first, launch_lanes, deep_cap);
    a.deep_nodes = deep_nodes.data();
    std::vector<uint32_t> lds_node(size_t(kRadiusLds) * kBlock);
    run_slice(n, kBlock, counters3, [&](unsigned long long lane, int tid, unsigned long long (&cnt)[3]) {
        if (a.offsets) radius_lane<T, Leaf, true, true, true>(a, first + lane, lds_node.data(), tid, lane, cnt);
        else radius_lane<T, Leaf, true, true, false>(a, first + lane, lds_node.data(), tid, lane, cnt);
    });
    if (!deep_nodes.guards_intact()) return kSliceGuardBroken;
    return deep_nodes.overwritten();
}

template <typename T, int Leaf>
T prim_dist2(const T* prims, size_t i, const T (&q)[3]) {
    T u = T(0), v = T(0);
    if (Leaf == LEAF_TRIANGLE) { T p[12]; std::memcpy(p, prims + 12 * i, sizeof(p)); return tri_dist2(p, q, u, v); }
    T s[4]; std::memcpy(s, prims + 4 * i, sizeof(s)); return sphere_dist2(s, q);
}

// every query against every primitive through the kernel's distance function: out_d2[k * n_prims + i]
template <typename T, int Leaf>
void brute(const T* prims, size_t n_prims, const T* queries, size_t n, T* out_d2, int threads) {
    const int nt = std::max(1, threads);
    std::vector<std::thread> pool;
    for (int t = 0; t < nt; ++t) {
        pool.emplace_back([=] {
            for (size_t k = n * t / nt; k < n * (t + 1) / nt; ++k) {
                const T q[3] = { queries[4 * k], queries[4 * k + 1], queries[4 * k + 2] };
                for (size_t i = 0; i < n_prims; ++i) out_d2[k * n_prims + i] = prim_dist2<T, Leaf>(prims, i, q);
            }
        });
    }
    for (auto& th : pool) th.join();
}

} // namespace

extern "C" {

// out_d2 (n x n_prims scalars of the primitives' type) = the kernel's squared distance of every query to every BVH-order primitive
void radius_host_brute(int is_double, int leaf, const void* prims, size_t n_prims, const void* queries, size_t n, void* out_d2, int threads) {
    if (is_double) {
        if (leaf == LEAF_SPHERE) brute<double, LEAF_SPHERE>(static_cast<const double*>(prims), n_prims, static_cast<const double*>(queries), n, static_cast<double*>(out_d2), threads);
        else brute<double, LEAF_TRIANGLE>(static_cast<const double*>(prims), n_prims, static_cast<const double*>(queries), n, static_cast<double*>(out_d2), threads);
    } else {
        if (leaf == LEAF_SPHERE) brute<float, LEAF_SPHERE>(static_cast<const float*>(prims), n_prims, static_cast<const float*>(queries), n, static_cast<float*>(out_d2), threads);
        else brute<float, LEAF_TRIANGLE>(static_cast<const float*>(prims), n_prims, static_cast<const float*>(queries), n, static_cast<float*>(out_d2), threads);
    }
}

// The kernel's walk for n queries {x, y, z, max_distance} (slot s reads query order[s], or s); leaf 0 = triangles, 1 = spheres;
// prim_ids (optional) = BVH_AMD_RAY_ORIGINAL_IDS; deep_cap > 0: the HBM spill of trees deeper than 64 levels, deep_cap entries.
// counts (optional), offsets (optional: NULL = the count-pass variant), list_prims, list_dist (optional) as in the C ABI;
// counters3 = {pairs fetched, primitives tested, leaves visited}. With threads > 1 the queries' segments must not overlap. Returns 0.
int radius_host_walk(int is_double, int leaf, const void* pairs, uint32_t root_index, const void* prims, const void* queries, size_t n,
                     const uint32_t* order, const uint32_t* prim_ids, uint32_t deep_cap, int threads, uint32_t* counts, const uint64_t* offsets,
                     uint32_t* list_prims, void* list_dist, unsigned long long* counters3) {
    if (is_double) {
        if (leaf == LEAF_SPHERE) return walk<double, LEAF_SPHERE>(pairs, root_index, prims, queries, n, order, prim_ids, deep_cap, threads, counts, offsets, list_prims, list_dist, counters3);
        return walk<double, LEAF_TRIANGLE>(pairs, root_index, prims, queries, n, order, prim_ids, deep_cap, threads, counts, offsets, list_prims, list_dist, counters3);
    }
    if (leaf == LEAF_SPHERE) return walk<float, LEAF_SPHERE>(pairs, root_index, prims, queries, n, order, prim_ids, deep_cap, threads, counts, offsets, list_prims, list_dist, counters3);
    return walk<float, LEAF_TRIANGLE>(pairs, root_index, prims, queries, n, order, prim_ids, deep_cap, threads, counts, offsets, list_prims, list_dist, counters3);
}

// One launch of a batch that point_query_run cut into slices (deep_cap > 0): slots [first, first + n) as the device walks them —
// a.first = first, slot = first + lane, lane = 0 .. n-1 indexing a spill of launch_lanes * deep_cap entries that the launch's lanes
// share, tid = lane % 256 in one LDS stand-in. queries, order, counts, offsets and the lists are the whole batch's. Returns the spill
// entries the launch overwrote, -1 if a guard zone around the spill was written to, -2 for deep_cap == 0 or n > launch_lanes.
long long radius_host_walk_slice(int is_double, int leaf, const void* pairs, uint32_t root_index, const void* prims, const void* queries, size_t first,
                                 size_t n, size_t launch_lanes, const uint32_t* order, const uint32_t* prim_ids, uint32_t deep_cap, uint32_t* counts,
                                 const uint64_t* offsets, uint32_t* list_prims, void* list_dist, unsigned long long* counters3) {
    if (is_double) {
        if (leaf == LEAF_SPHERE) return walk_slice<double, LEAF_SPHERE>(pairs, root_index, prims, queries, first, n, launch_lanes, order, prim_ids, deep_cap, counts, offsets, list_prims, list_dist, counters3);
        return walk_slice<double, LEAF_TRIANGLE>(pairs, root_index, prims, queries, first, n, launch_lanes, order, prim_ids, deep_cap, counts, offsets, list_prims, list_dist, counters3);
    }
    if (leaf == LEAF_SPHERE) return walk_slice<float, LEAF_SPHERE>(pairs, root_index, prims, queries, first, n, launch_lanes, order, prim_ids, deep_cap, counts, offsets, list_prims, list_dist, counters3);
    return walk_slice<float, LEAF_TRIANGLE>(pairs, root_index, prims, queries, first, n, launch_lanes, order, prim_ids, deep_cap, counts, offsets, list_prims, list_dist, counters3);
}

} // extern "C"
