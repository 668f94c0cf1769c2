// TEST INFRASTRUCTURE (CPU, no GPU): compiles the text of the box-overlap kernel — bvh_amd/csrc/overlap_body.inc (over list_walk.inc, the
// walk it shares with the radius query, and point_walk.inc) with the device helpers of bvh_amd/csrc/trace_device.h — for the HOST and runs it with one emulated lane per query (the queries of
// a batch one after another, or split over host threads). What it can show: the walk of the very source the device runs lists
// exactly the primitives a numpy brute force over the same closed-interval test lists, in the tree's order, and keeps to its
// segment; the device's counts, lists and counters must equal these byte for byte. What it cannot show: anything that needs the
// hardware. tests/test_overlap_host.py drives it; tests/test_gpu_overlap.py uses it too.
//
// Built by the tests with: g++ -std=c++20 -O1 -mavx2 -mfma -ffp-contract=off -fno-strict-aliasing -shared -fPIC -pthread.
#include "host_lane_prelude.h"
#include "../../bvh_amd/csrc/overlap_body.inc"

namespace {

using namespace bvh_amd;

template <typename T, bool Deep, bool Self>
void walk_range(const OverlapArgs<T>& a0, unsigned long long begin, unsigned long long end, unsigned long long (&cnt)[3]) {
    OverlapArgs<T> a = a0;
    std::vector<uint32_t> lds_node(size_t(kOverlapLds) * kBlock);
    std::vector<uint32_t> deep_nodes(Deep ? a.deep_cap : 1);
    a.deep_nodes = deep_nodes.data();                                        // one lane at a time: lane 0's spill
    for (unsigned long long s = begin; s < end; ++s) {
        if (a.offsets) overlap_lane<T, true, Deep, true, Self>(a, s, lds_node.data(), 0, 0, cnt);
        else overlap_lane<T, true, Deep, false, Self>(a, s, lds_node.data(), 0, 0, cnt);
    }
}

template <typename T>
int walk(const void* pairs, uint32_t root_index, const void* bboxes, const uint32_t* box_ids, const void* queries, size_t n, const uint32_t* order,
         int original_ids, uint32_t deep_cap, int threads, uint32_t* counts, const uint64_t* offsets, uint32_t* list_prims, unsigned long long* counters3) {
    OverlapArgs<T> a{};
    a.pairs = static_cast<const PairNode<T>*>(pairs); a.prims = static_cast<const T*>(bboxes); a.queries = static_cast<const T*>(queries);
    a.box_ids = box_ids; a.counts = counts; a.offsets = reinterpret_cast<const unsigned long long*>(offsets); a.list_prims = list_prims;
    a.n = n; a.first = 0; a.order = order; a.prim_ids = original_ids ? box_ids : nullptr; a.counters = nullptr;
    a.deep_cap = deep_cap; a.root_index = root_index;
    const bool self = queries == nullptr;
    run_lanes(n, threads, counters3, [&](unsigned long long b, unsigned long long e, unsigned long long (&cnt)[3]) {
        if (deep_cap) { if (self) walk_range<T, true, true>(a, b, e, cnt); else walk_range<T, true, false>(a, b, e, cnt); }
        else { if (self) walk_range<T, false, true>(a, b, e, cnt); else walk_range<T, false, false>(a, b, e, cnt); }
    });
    return 0;
}

// One launch of a sliced batch as the device runs it (prelude: GuardedSpill, run_slice): the spill sized for the launch's lanes.
template <typename T>
long long walk_slice(const void* pairs, uint32_t root_index, const void* bboxes, const uint32_t* box_ids, const void* queries, size_t first, size_t n,
                     size_t launch_lanes, const uint32_t* order, int original_ids, uint32_t deep_cap, uint32_t* counts, const uint64_t* offsets,
                     uint32_t* list_prims, unsigned long long* counters3) {
    if (deep_cap == 0 || n > launch_lanes) return kSliceBadArgs;
    OverlapArgs<T> a{};
    a.pairs = static_cast<const PairNode<T>*>(pairs); a.prims = static_cast<const T*>(bboxes); a.queries = static_cast<const T*>(queries);
    a.box_ids = box_ids; a.counts = counts; a.offsets = reinterpret_cast<const unsigned long long*>(offsets); a.list_prims = list_prims;
    a.n = n; a.first = first; a.order = order; a.prim_ids = original_ids ? box_ids : nullptr; a.counters = nullptr;
    a.deep_cap = deep_cap; a.root_index = root_index;
    GuardedSpill<uint32_t> deep_nodes(first, launch_lanes, deep_cap);
    a.deep_nodes = deep_nodes.data();
    std::vector<uint32_t> lds_node(size_t(kOverlapLds) * kBlock);
    const bool self = queries == nullptr, fill = offsets != nullptr;
    run_slice(n, kBlock, counters3, [&](unsigned long long lane, int tid, unsigned long long (&cnt)[3]) {
        if (self) {
            if (fill) overlap_lane<T, true, true, true, true>(a, first + lane, lds_node.data(), tid, lane, cnt);
            else overlap_lane<T, true, true, false, true>(a, first + lane, lds_node.data(), tid, lane, cnt);
        } else {
            if (fill) overlap_lane<T, true, true, true, false>(a, first + lane, lds_node.data(), tid, lane, cnt);
            else overlap_lane<T, true, true, false, false>(a, first + lane, lds_node.data(), tid, lane, cnt);
        }
    });
    if (!deep_nodes.guards_intact()) return kSliceGuardBroken;
    return deep_nodes.overwritten();
}

} // namespace

extern "C" {

// The kernel's walk for n query boxes {min.xyz, max.xyz} (slot s reads query order[s], or s); queries == NULL: self mode, query q is
// BVH-order primitive q (n = the primitive count) and lists only i > q. bboxes: boxes by original id, box_ids: BVH-order index ->
// original id; original_ids != 0 = BVH_AMD_RAY_ORIGINAL_IDS; deep_cap > 0: the HBM spill of trees deeper than 64 levels, deep_cap
// entries. counts (optional), offsets (optional: NULL = the count-pass variant), list_prims as in the C ABI; counters3 = {pairs
// fetched, primitive boxes tested, leaves visited}. With threads > 1 the queries' segments must not overlap. Returns 0.
int overlap_host_walk(int is_double, const void* pairs, uint32_t root_index, const void* bboxes, const uint32_t* box_ids, const void* queries, size_t n,
                      const uint32_t* order, int original_ids, uint32_t deep_cap, int threads, uint32_t* counts, const uint64_t* offsets,
                      uint32_t* list_prims, unsigned long long* counters3) {
    if (is_double) return walk<double>(pairs, root_index, bboxes, box_ids, queries, n, order, original_ids, deep_cap, threads, counts, offsets, list_prims, counters3);
    return walk<float>(pairs, root_index, bboxes, box_ids, queries, n, order, original_ids, deep_cap, threads, counts, offsets, list_prims, counters3);
}

// One launch of a batch that point_query_run cut into slices (deep_cap > 0): slots [first, first + n) as the device walks them —
// a.first = first, slot = first + lane (in self mode: BVH-order primitive first + lane), lane = 0 .. n-1 indexing a spill of
// launch_lanes * deep_cap entries that the launch's lanes share, tid = lane % 256 in one LDS stand-in. queries, order, counts, offsets
// and the list are the whole batch's. Returns the spill entries the launch overwrote, -1 if a guard zone around the spill was written
// to, -2 for deep_cap == 0 or n > launch_lanes.
long long overlap_host_walk_slice(int is_double, const void* pairs, uint32_t root_index, const void* bboxes, const uint32_t* box_ids, const void* queries,
                                  size_t first, size_t n, size_t launch_lanes, const uint32_t* order, int original_ids, uint32_t deep_cap, uint32_t* counts,
                                  const uint64_t* offsets, uint32_t* list_prims, unsigned long long* counters3) {
    if (is_double) return walk_slice<double>(pairs, root_index, bboxes, box_ids, queries, first, n, launch_lanes, order, original_ids, deep_cap, counts, offsets, list_prims, counters3);
    return walk_slice<float>(pairs, root_index, bboxes, box_ids, queries, first, n, launch_lanes, order, original_ids, deep_cap, counts, offsets, list_prims, counters3);
}

} // extern "C"
