// Batched triangle-intersection queries for gfx950: for every query triangle {p0, p1, p2}, how many BVH-order primitives have a
// triangle that intersects it (closed sets) and, optionally, which ones; and the self-intersections of a tree's own triangles (the
// narrow phase of a collision test, inside the walk of the broad phase). The primitives' triangles are the caller's array indexed by
// original primitive id, the one bvh3X_refit_tris takes, read through the tree's prim ids. The per-lane body is
// tri_intersect_body.inc (shared with the host test harness, tests/cpp/tri_intersect_body_host.cpp): the query triangle and the
// sign-only pair test (tri_pair.inc), handed to the walk overlap.hip and radius.hip use, list_walk.inc (stack, descent, counts, segments), over
// point_walk.inc (stack tiers, streaming stores); the launch path is point_query.h's.
//
// MI355X mapping (overlap.hip's, with a triangle test behind the primitive's box test):
//   * one lane per query, one-shot grid of ceil(n / 256) blocks: no ticket counter, so no work slot of the tree is claimed and any
//     number of launches of one const tree may run at once;
//   * a lane holds its query for the whole walk: nine coordinates, their box, the normal (computed once);
//   * depth-first walk over the 64 / 128-byte pair records, left child first, the right one stacked as a bare node word when both
//     boxes overlap the query's box. Nothing is pruned against what was found;
//   * the stack: kTriIntersectLds entries in LDS, the rest of 64 in per-lane scratch, beyond 64 (deep trees) in HBM (point_walk.inc);
//   * a leaf's primitives one at a time: prim id, then the 36 / 72 bytes of its triangle; its box against the query's, the shared-vertex
//     filter if asked for, the plane-side signs (where most pairs leave), then the interval or the coplanar step. The permutations of
//     the interval step are selects, so that lanes with different sign patterns run one instruction stream;
//   * radius search's variable-length output: counts, segments [offsets[q], offsets[q + 1]), padding (the Fill = false kernels hold
//     no list store and no offset load);
//   * query triangles are optionally read in the order of the Hilbert cell of their box's centre in the root box (query_order.h).
//     Self mode never reorders: lane q is BVH-order primitive q, and BVH order is the tree's own spatial order.

#include "common.h"
#include "trace_device.h"
#include "ray_key.h"
#include "query_order.h"
#include "tri_intersect_body.inc"
#include "point_query.h"

namespace bvh_amd {

namespace {

template <typename T, bool Stats, bool Deep, bool Fill, bool Self>
__global__ void __launch_bounds__(kBlock) tri_intersect_kernel(TriIntersectArgs<T> a) {
    __shared__ uint32_t lds_node[kTriIntersectLds * kBlock];
    const int tid = threadIdx.x;
    const unsigned long long lane = static_cast<unsigned long long>(blockIdx.x) * kBlock + tid;
    unsigned long long cnt[3] = {0, 0, 0};
    if (lane < a.n) tri_intersect_lane<T, Stats, Deep, Fill, Self>(a, a.first + lane, lds_node, tid, lane, cnt);
    if (Stats) add_counters(a.counters, cnt, tid);
}

} // namespace

// d_queries9 == nullptr with self = true: the queries are the tree's own triangles, n = b.prim_count.
template <typename T>
int launch_tri_intersect(const BvhImpl<T>& b, bool self, const T* d_tris9, size_t n_tris, const T* d_queries9, size_t n, unsigned flags,
                         uint32_t* d_counts, const uint64_t* d_offsets, uint32_t* d_list_prims, bvh_amd_counters* d_counters, hipStream_t stream) {
    const char* who = self ? "intersect_tris_self" : "intersect_tris";
    if (self && (flags & ~unsigned(BVH_AMD_RAY_ORIGINAL_IDS | BVH_AMD_TRI_SKIP_SHARED)))
        return fail(BVH_AMD_ERR_ARG, std::string(who) + ": unsupported flags (ORIGINAL_IDS and TRI_SKIP_SHARED only: self mode walks in BVH order and never reorders)");
    if (flags & ~unsigned(BVH_AMD_RAY_ORIGINAL_IDS | BVH_AMD_RAY_SORTED | BVH_AMD_RAY_UNSORTED | BVH_AMD_TRI_SKIP_SHARED))
        return fail(BVH_AMD_ERR_ARG, std::string(who) + ": unsupported flags (ORIGINAL_IDS, SORTED, UNSORTED and TRI_SKIP_SHARED only)");
    const unsigned walk_flags = flags & ~unsigned(BVH_AMD_TRI_SKIP_SHARED);      // what the shared launch path knows
    const bool aligned = !(misaligned(d_tris9, sizeof(T)) || misaligned(d_queries9, sizeof(T)) || misaligned(d_offsets, 8) || misaligned(d_counters, 8) ||
                           misaligned(d_counts, 4) || misaligned(d_list_prims, 4));
    const char* fault = list_output_fault(d_counts, d_offsets, d_list_prims, nullptr);
    if (!fault && !aligned) fault = "device pointers must be aligned (triangles and queries to their scalar, offsets and counters 8 bytes, counts and list prims 4)";
    if (const int rc = point_query_check(b, n, walk_flags, d_tris9 && (self || d_queries9), fault, who); rc || n == 0) return rc;
    if (const int rc = source_array_check(b, n_tris, "triangles", who, stream)) return rc;
    const unsigned run_flags = self ? walk_flags | BVH_AMD_RAY_UNSORTED : walk_flags;
    const uint32_t skip_shared = (flags & BVH_AMD_TRI_SKIP_SHARED) ? 1u : 0u;
    // (kPointSortMin: the threshold measured for closest-point queries; not measured for this kind, which takes it as radius and
    //  k-nearest queries do. tools/tri_intersect_bench.py times SORTED against UNSORTED.)
    return point_query_run<T, kQueryTris>(b, d_tris9, d_queries9, n, run_flags, d_counters, sizeof(uint32_t), kBlock, kPointSortMin, kPointKeyBits, who, stream,
                                   [&](const PointArgs<T>& args, T*) {
        const TriIntersectArgs<T> a{{args, d_counts, reinterpret_cast<const unsigned long long*>(d_offsets), d_list_prims}, b.d_prim_ids, skip_shared};
        // (the ladder's leaf kind is unused here: a triangle is a triangle)
        return list_query_dispatch(LEAF_TRIANGLE, d_counters != nullptr, a.deep_cap != 0, a.offsets != nullptr, [&](auto, auto stats, auto deep, auto fill) {
            return self ? point_query_launch(tri_intersect_kernel<T, stats(), deep(), fill(), true>, a, kBlock, 0, stream)
                        : point_query_launch(tri_intersect_kernel<T, stats(), deep(), fill(), false>, a, kBlock, 0, stream);
        });
    });
}

template int launch_tri_intersect<float>(const BvhImpl<float>&, bool, const float*, size_t, const float*, size_t, unsigned, uint32_t*, const uint64_t*, uint32_t*,
                                         bvh_amd_counters*, hipStream_t);
template int launch_tri_intersect<double>(const BvhImpl<double>&, bool, const double*, size_t, const double*, size_t, unsigned, uint32_t*, const uint64_t*,
                                          uint32_t*, bvh_amd_counters*, hipStream_t);

} // namespace bvh_amd
