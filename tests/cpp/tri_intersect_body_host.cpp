// TEST INFRASTRUCTURE (CPU, no GPU): compiles the text of the triangle-intersection kernel — bvh_amd/csrc/tri_intersect_body.inc (over
// overlap_body.inc's box tests, list_walk.inc and point_walk.inc) with the device helpers of bvh_amd/csrc/trace_device.h — for the HOST
// and runs it with one emulated lane per query (the queries of a batch one after another, or split over host threads). What it can
// show: the pair test of the very source the device runs equals an exact integer reference wherever the inputs make its arithmetic
// exact; the walk lists exactly the primitives a brute force over that pair test lists, in the tree's order, and keeps to its
// segment; the device's counts, lists and counters must equal these byte for byte. What it cannot show: anything that needs the
// hardware. tests/test_tri_intersect_host.py drives it; tests/test_gpu_tri_intersect.py uses it too.
//
// Built by the tests with: g++ -std=c++20 -O1 -mavx2 -mfma -ffp-contract=off -fno-strict-aliasing -shared -fPIC -pthread.
#include "host_lane_prelude.h"
#include "../../bvh_amd/csrc/tri_intersect_body.inc"

namespace {

using namespace bvh_amd;

template <typename T>
TriIntersectArgs<T> make_args(const void* pairs, uint32_t root_index, const void* tris9, const uint32_t* tri_ids, const void* queries, size_t first, size_t n,
                              const uint32_t* order, int original_ids, int skip_shared, uint32_t deep_cap, uint32_t* counts, const uint64_t* offsets,
                              uint32_t* list_prims) {
    TriIntersectArgs<T> a{};
    a.pairs = static_cast<const PairNode<T>*>(pairs); a.prims = static_cast<const T*>(tris9); a.queries = static_cast<const T*>(queries);
    a.tri_ids = tri_ids; a.skip_shared = skip_shared ? 1u : 0u;
    a.counts = counts; a.offsets = reinterpret_cast<const unsigned long long*>(offsets); a.list_prims = list_prims;
    a.n = n; a.first = first; a.order = order; a.prim_ids = original_ids ? tri_ids : nullptr; a.counters = nullptr;
    a.deep_cap = deep_cap; a.root_index = root_index;
    return a;
}

template <typename T, bool Deep, bool Self>
void walk_range(const TriIntersectArgs<T>& a0, unsigned long long begin, unsigned long long end, unsigned long long (&cnt)[3]) {
    TriIntersectArgs<T> a = a0;
    std::vector<uint32_t> lds_node(size_t(kTriIntersectLds) * kBlock);
    std::vector<uint32_t> deep_nodes(Deep ? a.deep_cap : 1);
    a.deep_nodes = deep_nodes.data();                                        // one lane at a time: lane 0's spill
    for (unsigned long long s = begin; s < end; ++s) {
        if (a.offsets) tri_intersect_lane<T, true, Deep, true, Self>(a, s, lds_node.data(), 0, 0, cnt);
        else tri_intersect_lane<T, true, Deep, false, Self>(a, s, lds_node.data(), 0, 0, cnt);
    }
}

template <typename T>
int walk(const void* pairs, uint32_t root_index, const void* tris9, const uint32_t* tri_ids, const void* queries, size_t n, const uint32_t* order,
         int original_ids, int skip_shared, uint32_t deep_cap, int threads, uint32_t* counts, const uint64_t* offsets, uint32_t* list_prims,
         unsigned long long* counters3) {
    const TriIntersectArgs<T> a = make_args<T>(pairs, root_index, tris9, tri_ids, queries, 0, n, order, original_ids, skip_shared, deep_cap, counts, offsets, list_prims);
    const bool self = queries == nullptr;
    run_lanes(n, threads, counters3, [&](unsigned long long b, unsigned long long e, unsigned long long (&cnt)[3]) {
        if (deep_cap) { if (self) walk_range<T, true, true>(a, b, e, cnt); else walk_range<T, true, false>(a, b, e, cnt); }
        else { if (self) walk_range<T, false, true>(a, b, e, cnt); else walk_range<T, false, false>(a, b, e, cnt); }
    });
    return 0;
}

// One launch of a sliced batch as the device runs it (prelude: GuardedSpill, run_slice): the spill sized for the launch's lanes.
template <typename T>
long long walk_slice(const void* pairs, uint32_t root_index, const void* tris9, const uint32_t* tri_ids, const void* queries, size_t first, size_t n,
                     size_t launch_lanes, const uint32_t* order, int original_ids, int skip_shared, uint32_t deep_cap, uint32_t* counts,
                     const uint64_t* offsets, uint32_t* list_prims, unsigned long long* counters3) {
    if (deep_cap == 0 || n > launch_lanes) return kSliceBadArgs;
    TriIntersectArgs<T> a = make_args<T>(pairs, root_index, tris9, tri_ids, queries, first, n, order, original_ids, skip_shared, deep_cap, counts, offsets, list_prims);
    GuardedSpill<uint32_t> deep_nodes(first, launch_lanes, deep_cap);
    a.deep_nodes = deep_nodes.data();
    std::vector<uint32_t> lds_node(size_t(kTriIntersectLds) * kBlock);
    const bool self = queries == nullptr, fill = offsets != nullptr;
    run_slice(n, kBlock, counters3, [&](unsigned long long lane, int tid, unsigned long long (&cnt)[3]) {
        if (self) {
            if (fill) tri_intersect_lane<T, true, true, true, true>(a, first + lane, lds_node.data(), tid, lane, cnt);
            else tri_intersect_lane<T, true, true, false, true>(a, first + lane, lds_node.data(), tid, lane, cnt);
        } else {
            if (fill) tri_intersect_lane<T, true, true, true, false>(a, first + lane, lds_node.data(), tid, lane, cnt);
            else tri_intersect_lane<T, true, true, false, false>(a, first + lane, lds_node.data(), tid, lane, cnt);
        }
    });
    if (!deep_nodes.guards_intact()) return kSliceGuardBroken;
    return deep_nodes.overwritten();
}

// The pair test as a lane applies it: a is prepared like a lane's query (box, normal; unusable: intersects nothing), b is a candidate.
template <typename T>
int pair(const T* a9, const T* b9, int skip_shared) {
    T a[9], b[9], lo[3], hi[3], na[3];
    load_tri9(a9, a);
    load_tri9(b9, b);
    tri_box(a, lo, hi);
    tri_normal(a, na);
    if (!normal_usable(na)) return 0;
    return tri_pair_intersects(a, lo, hi, na, b, skip_shared != 0) ? 1 : 0;
}

} // namespace

extern "C" {

// Whether triangle a9 {p0.xyz, p1.xyz, p2.xyz} as a query intersects triangle b9 as a primitive (floats, or doubles when is_double).
int tri_tri_intersects(int is_double, const void* a9, const void* b9, int skip_shared) {
    if (is_double) return pair<double>(static_cast<const double*>(a9), static_cast<const double*>(b9), skip_shared);
    return pair<float>(static_cast<const float*>(a9), static_cast<const float*>(b9), skip_shared);
}

// m[i * nb + j] = tri_tri_intersects(a[i], b[j]) for every pair of two arrays of triangles (the tests' brute force).
void tri_tri_matrix(int is_double, const void* a9, size_t na, const void* b9, size_t nb, int skip_shared, unsigned char* m) {
    const size_t scalar = is_double ? sizeof(double) : sizeof(float);
    for (size_t i = 0; i < na; ++i)
        for (size_t j = 0; j < nb; ++j)
            m[i * nb + j] = static_cast<unsigned char>(tri_tri_intersects(is_double, static_cast<const char*>(a9) + 9 * scalar * i,
                                                                          static_cast<const char*>(b9) + 9 * scalar * j, skip_shared));
}

// The kernel's walk for n query triangles of 9 scalars (slot s reads query order[s], or s); queries == NULL: self mode, query q is
// BVH-order primitive q (n = the primitive count) and lists only i > q. tris9: triangles by original id, tri_ids: BVH-order index ->
// original id; original_ids != 0 = BVH_AMD_RAY_ORIGINAL_IDS, skip_shared != 0 = BVH_AMD_TRI_SKIP_SHARED; deep_cap > 0: the HBM spill of
// trees deeper than 64 levels, deep_cap entries. counts (optional), offsets (optional: NULL = the count-pass variant), list_prims as
// in the C ABI; counters3 = {pairs fetched, triangles fetched, leaves visited}. With threads > 1 the queries' segments must not
// overlap. Returns 0.
int tri_intersect_host_walk(int is_double, const void* pairs, uint32_t root_index, const void* tris9, const uint32_t* tri_ids, const void* queries, size_t n,
                            const uint32_t* order, int original_ids, int skip_shared, uint32_t deep_cap, int threads, uint32_t* counts,
                            const uint64_t* offsets, uint32_t* list_prims, unsigned long long* counters3) {
    if (is_double) return walk<double>(pairs, root_index, tris9, tri_ids, queries, n, order, original_ids, skip_shared, deep_cap, threads, counts, offsets, list_prims, counters3);
    return walk<float>(pairs, root_index, tris9, tri_ids, queries, n, order, original_ids, skip_shared, deep_cap, threads, counts, offsets, list_prims, counters3);
}

// One launch of a batch that point_query_run cut into slices (deep_cap > 0): slots [first, first + n) as the device walks them —
// a.first = first, slot = first + lane (in self mode: BVH-order primitive first + lane), lane = 0 .. n-1 indexing a spill of
// launch_lanes * deep_cap entries that the launch's lanes share, tid = lane % 256 in one LDS stand-in. queries, order, counts, offsets
// and the list are the whole batch's. Returns the spill entries the launch overwrote, -1 if a guard zone around the spill was written
// to, -2 for deep_cap == 0 or n > launch_lanes.
long long tri_intersect_host_walk_slice(int is_double, const void* pairs, uint32_t root_index, const void* tris9, const uint32_t* tri_ids, const void* queries,
                                        size_t first, size_t n, size_t launch_lanes, const uint32_t* order, int original_ids, int skip_shared,
                                        uint32_t deep_cap, uint32_t* counts, const uint64_t* offsets, uint32_t* list_prims, unsigned long long* counters3) {
    if (is_double) return walk_slice<double>(pairs, root_index, tris9, tri_ids, queries, first, n, launch_lanes, order, original_ids, skip_shared, deep_cap, counts, offsets, list_prims, counters3);
    return walk_slice<float>(pairs, root_index, tris9, tri_ids, queries, first, n, launch_lanes, order, original_ids, skip_shared, deep_cap, counts, offsets, list_prims, counters3);
}

} // extern "C"
