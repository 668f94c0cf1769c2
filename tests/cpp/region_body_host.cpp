// TEST INFRASTRUCTURE (CPU, no GPU): compiles the text of the convex-region kernel — bvh_amd/csrc/region_body.inc (over list_walk.inc, the
// walk it shares with the radius and overlap queries, and point_walk.inc) with the device helpers of bvh_amd/csrc/trace_device.h — for
// the HOST and runs it with one emulated lane per query (the queries of a batch one after another, or split over host threads). What
// it can show: the walk of the very source the device runs lists exactly the primitives a brute force of the stated tests lists, in
// the tree's order, and keeps to its segment; the EXACT predicate, called on bare (triangle, region) pairs, equals exact clipping
// where the arithmetic is exact; the device's counts, lists, flags and counters must equal these byte for byte. What it cannot show:
// anything that needs the hardware. tests/test_region_host.py drives it; tests/test_gpu_region.py uses it too.
//
// Built by the tests with: g++ -std=c++20 -O1 -mavx2 -mfma -ffp-contract=off -fno-strict-aliasing -shared -fPIC -pthread.
#include "host_lane_prelude.h"
#include "../../bvh_amd/csrc/region_body.inc"

namespace {

using namespace bvh_amd;

template <typename T, bool Deep, int Leaf, bool Exact>
void lane(const RegionArgs<T>& a, unsigned long long slot, uint32_t* lds, int tid, unsigned long long ln, unsigned long long (&cnt)[3]) {
    if (a.offsets) region_lane<T, true, Deep, true, Leaf, Exact>(a, slot, lds, tid, ln, cnt);
    else region_lane<T, true, Deep, false, Leaf, Exact>(a, slot, lds, tid, ln, cnt);
}

template <typename T, bool Deep>
void lane_kind(const RegionArgs<T>& a, int leaf, int exact, unsigned long long slot, uint32_t* lds, int tid, unsigned long long ln,
               unsigned long long (&cnt)[3]) {
    if (leaf == LEAF_SPHERE) lane<T, Deep, LEAF_SPHERE, false>(a, slot, lds, tid, ln, cnt);
    else if (exact) lane<T, Deep, LEAF_TRIANGLE, true>(a, slot, lds, tid, ln, cnt);
    else lane<T, Deep, LEAF_TRIANGLE, false>(a, slot, lds, tid, ln, cnt);
}

template <typename T>
RegionArgs<T> make_args(const void* pairs, uint32_t root_index, const void* prims, const uint32_t* ids, const void* planes, uint32_t m, size_t first,
                        size_t n, int original_ids, uint32_t deep_cap, uint32_t* counts, const uint64_t* offsets, uint32_t* list_prims,
                        uint8_t* list_inside) {
    RegionArgs<T> a{};
    a.pairs = static_cast<const PairNode<T>*>(pairs); a.prims = static_cast<const T*>(prims); a.queries = static_cast<const T*>(planes);
    a.ids = ids; a.m = m; a.counts = counts; a.offsets = reinterpret_cast<const unsigned long long*>(offsets); a.list_prims = list_prims;
    a.list_inside = list_inside; a.n = n; a.first = first; a.order = nullptr; a.prim_ids = original_ids ? ids : nullptr; a.counters = nullptr;
    a.deep_cap = deep_cap; a.root_index = root_index;
    return a;
}

template <typename T>
int walk(const void* pairs, uint32_t root_index, const void* prims, const uint32_t* ids, int leaf, int exact, const void* planes, uint32_t m, size_t n,
         int original_ids, uint32_t deep_cap, int threads, uint32_t* counts, const uint64_t* offsets, uint32_t* list_prims, uint8_t* list_inside,
         unsigned long long* counters3) {
    const RegionArgs<T> a0 = make_args<T>(pairs, root_index, prims, ids, planes, m, 0, n, original_ids, deep_cap, counts, offsets, list_prims, list_inside);
    run_lanes(n, threads, counters3, [&](unsigned long long b, unsigned long long e, unsigned long long (&cnt)[3]) {
        RegionArgs<T> a = a0;
        std::vector<uint32_t> lds_node(size_t(kRegionLds) * kBlock);
        std::vector<uint32_t> deep_nodes(deep_cap ? deep_cap : 1);
        a.deep_nodes = deep_nodes.data();                                    // one lane at a time: lane 0's spill
        for (unsigned long long s = b; s < e; ++s) {
            if (deep_cap) lane_kind<T, true>(a, leaf, exact, s, lds_node.data(), 0, 0, cnt);
            else lane_kind<T, false>(a, leaf, exact, s, lds_node.data(), 0, 0, cnt);
        }
    });
    return 0;
}

// One launch of a sliced batch as the device runs it (prelude: GuardedSpill, run_slice): the spill sized for the launch's lanes.
template <typename T>
long long walk_slice(const void* pairs, uint32_t root_index, const void* prims, const uint32_t* ids, int leaf, int exact, const void* planes, uint32_t m,
                     size_t first, size_t n, size_t launch_lanes, int original_ids, uint32_t deep_cap, uint32_t* counts, const uint64_t* offsets,
                     uint32_t* list_prims, uint8_t* list_inside, unsigned long long* counters3) {
    if (deep_cap == 0 || n > launch_lanes) return kSliceBadArgs;
    RegionArgs<T> a = make_args<T>(pairs, root_index, prims, ids, planes, m, first, n, original_ids, deep_cap, counts, offsets, list_prims, list_inside);
    GuardedSpill<uint32_t> deep_nodes(first, launch_lanes, deep_cap);
    a.deep_nodes = deep_nodes.data();
    std::vector<uint32_t> lds_node(size_t(kRegionLds) * kBlock);
    run_slice(n, kBlock, counters3, [&](unsigned long long ln, int tid, unsigned long long (&cnt)[3]) {
        lane_kind<T, true>(a, leaf, exact, first + ln, lds_node.data(), tid, ln, cnt);
    });
    if (!deep_nodes.guards_intact()) return kSliceGuardBroken;
    return deep_nodes.overwritten();
}

// The primitive tests alone, pair k = (primitive k, region k): out[k] = bit 0 CULL, bit 1 EXACT (triangles), bit 2 wholly inside.
template <typename T>
void pair_tests(int leaf, const void* prims, const void* planes, uint32_t m, size_t n, uint8_t* out) {
    const T* pr = static_cast<const T*>(prims);
    const T* q = static_cast<const T*>(planes);
    for (size_t k = 0; k < n; ++k) {
        T pl[kRegionMaxPlanes][4] = {};
        const bool valid = load_planes(q + 4ull * m * k, m, pl);
        bool inside = false, in2 = false;
        uint8_t r = 0;
        if (valid && leaf == LEAF_TRIANGLE) {
            if (tri_in_region<T, false>(pr + 9 * k, pl, m, inside)) r |= 1;
            if (tri_in_region<T, true>(pr + 9 * k, pl, m, in2)) r |= 2;
        } else if (valid) {
            T len[kRegionMaxPlanes] = {};
            plane_lengths(pl, m, len);
            if (sphere_in_region(pr + 4 * k, pl, len, m, inside)) r |= 1;
        }
        if ((r & 1) && inside) r |= 4;
        out[k] = r;
    }
}

} // namespace

extern "C" {

// The kernel's walk for n regions of m planes {nx, ny, nz, d}. prims: triangles (9 scalars) or spheres (4) by original id (leaf: 0 =
// triangles, 1 = spheres), ids: BVH-order index -> original id; exact != 0 = BVH_AMD_REGION_EXACT; original_ids != 0 =
// BVH_AMD_RAY_ORIGINAL_IDS; deep_cap > 0: the HBM spill of trees deeper than 64 levels, deep_cap entries. counts (optional), offsets
// (optional: NULL = the count-pass variant), list_prims and list_inside (optional) as in the C ABI; counters3 = {pairs fetched,
// primitives tested, leaves visited}. With threads > 1 the queries' segments must not overlap. Returns 0.
int region_host_walk(int is_double, const void* pairs, uint32_t root_index, const void* prims, const uint32_t* ids, int leaf, int exact, const void* planes,
                     uint32_t m, size_t n, int original_ids, uint32_t deep_cap, int threads, uint32_t* counts, const uint64_t* offsets, uint32_t* list_prims,
                     uint8_t* list_inside, unsigned long long* counters3) {
    if (m < 1 || m > uint32_t(kRegionMaxPlanes) || (exact && leaf != LEAF_TRIANGLE)) return 1;
    if (is_double) return walk<double>(pairs, root_index, prims, ids, leaf, exact, planes, m, n, original_ids, deep_cap, threads, counts, offsets, list_prims, list_inside, counters3);
    return walk<float>(pairs, root_index, prims, ids, leaf, exact, planes, m, n, original_ids, deep_cap, threads, counts, offsets, list_prims, list_inside, counters3);
}

// One launch of a batch that point_query_run cut into slices (deep_cap > 0): slots [first, first + n) as the device walks them —
// a.first = first, slot = first + lane, lane = 0 .. n-1 indexing a spill of launch_lanes * deep_cap entries that the launch's lanes
// share, tid = lane % 256 in one LDS stand-in. planes, counts, offsets and the lists are the whole batch's. Returns the spill entries
// the launch overwrote, -1 if a guard zone around the spill was written to, -2 for deep_cap == 0 or n > launch_lanes.
long long region_host_walk_slice(int is_double, const void* pairs, uint32_t root_index, const void* prims, const uint32_t* ids, int leaf, int exact,
                                 const void* planes, uint32_t m, size_t first, size_t n, size_t launch_lanes, int original_ids, uint32_t deep_cap,
                                 uint32_t* counts, const uint64_t* offsets, uint32_t* list_prims, uint8_t* list_inside, unsigned long long* counters3) {
    if (m < 1 || m > uint32_t(kRegionMaxPlanes) || (exact && leaf != LEAF_TRIANGLE)) return kSliceBadArgs;
    if (is_double) return walk_slice<double>(pairs, root_index, prims, ids, leaf, exact, planes, m, first, n, launch_lanes, original_ids, deep_cap, counts, offsets, list_prims, list_inside, counters3);
    return walk_slice<float>(pairs, root_index, prims, ids, leaf, exact, planes, m, first, n, launch_lanes, original_ids, deep_cap, counts, offsets, list_prims, list_inside, counters3);
}

// The kernel's primitive tests on n bare pairs (primitive k against region k, m planes each): out[k] = 1 (CULL passes) | 2 (EXACT
// passes, triangles only) | 4 (wholly inside). A region with a NaN or infinite component: 0. Returns 0.
int region_host_pairs(int is_double, int leaf, const void* prims, const void* planes, uint32_t m, size_t n, uint8_t* out) {
    if (m < 1 || m > uint32_t(kRegionMaxPlanes)) return 1;
    if (is_double) pair_tests<double>(leaf, prims, planes, m, n, out);
    else pair_tests<float>(leaf, prims, planes, m, n, out);
    return 0;
}

} // extern "C"
