// Batched box-overlap queries for gfx950: for every query box {min.xyz, max.xyz}, how many BVH-order primitives have a box that
// overlaps it (closed intervals) and, optionally, which ones; and the self-overlap pairs of a tree's own primitives (the broad phase of
// a collision test). The primitives' boxes are the caller's array indexed by original primitive id, the one bvhXX_build_device and
// bvhXX_refit_boxes take, read through the tree's prim ids. The per-lane body is overlap_body.inc (shared with the host test harness,
// tests/cpp/overlap_body_host.cpp): the query box and its tests, handed to the walk radius.hip uses too, list_walk.inc (stack,
// descent, counts, segments), over point_walk.inc (stack tiers, streaming stores); the launch path is point_query.h's.
//
// MI355X mapping (radius.hip's, with the overlap test in place of the distance to a box):
//   * one lane per query, one-shot grid of ceil(n / 256) blocks: no ticket counter, so no work slot of the tree is claimed and any
//     number of launches of one const tree may run at once;
//   * depth-first walk over the 64 / 128-byte pair records, left child first, the right one stacked as a bare node word when both
//     boxes overlap the query. Nothing is pruned against what was found: the list of a query is fixed by the tree and the boxes;
//   * the stack: kOverlapLds entries in LDS, the rest of 64 in per-lane scratch, beyond 64 (deep trees) in HBM (point_walk.inc);
//   * a leaf's primitives one at a time: prim id, then the 24 / 48 bytes of its box;
//   * radius search's variable-length output: counts, segments [offsets[q], offsets[q + 1]), padding (the Fill = false kernels hold
//     no list store and no offset load);
//   * query boxes are optionally read in the order of the Hilbert cell of their centre in the root box (query_order.h). Self mode
//     never reorders: lane q is BVH-order primitive q, and BVH order is the tree's own spatial order.

#include "common.h"
#include "trace_device.h"
#include "ray_key.h"
#include "query_order.h"
#include "overlap_body.inc"
#include "point_query.h"

namespace bvh_amd {

namespace {

template <typename T, bool Stats, bool Deep, bool Fill, bool Self>
__global__ void __launch_bounds__(kBlock) overlap_kernel(OverlapArgs<T> a) {
    __shared__ uint32_t lds_node[kOverlapLds * kBlock];
    const int tid = threadIdx.x;
    const unsigned long long lane = static_cast<unsigned long long>(blockIdx.x) * kBlock + tid;
    unsigned long long cnt[3] = {0, 0, 0};
    if (lane < a.n) overlap_lane<T, Stats, Deep, Fill, Self>(a, a.first + lane, lds_node, tid, lane, cnt);
    if (Stats) add_counters(a.counters, cnt, tid);
}

} // namespace

// d_queries6 == nullptr with self = true: the queries are the tree's own primitives, n = b.prim_count.
template <typename T>
int launch_overlap(const BvhImpl<T>& b, bool self, const T* d_bboxes, size_t n_boxes, const T* d_queries6, size_t n, unsigned flags,
                   uint32_t* d_counts, const uint64_t* d_offsets, uint32_t* d_list_prims, bvh_amd_counters* d_counters, hipStream_t stream) {
    const char* who = self ? "overlap_self" : "overlap_boxes";
    if (self && (flags & ~unsigned(BVH_AMD_RAY_ORIGINAL_IDS)))
        return fail(BVH_AMD_ERR_ARG, std::string(who) + ": unsupported flags (ORIGINAL_IDS only: self mode walks in BVH order and never reorders)");
    const bool aligned = !(misaligned(d_bboxes, sizeof(T)) || misaligned(d_queries6, sizeof(T)) || misaligned(d_offsets, 8) || misaligned(d_counters, 8) ||
                           misaligned(d_counts, 4) || misaligned(d_list_prims, 4));
    const char* fault = list_output_fault(d_counts, d_offsets, d_list_prims, nullptr);
    if (!fault && !aligned) fault = "device pointers must be aligned (boxes and queries to their scalar, offsets and counters 8 bytes, counts and list prims 4)";
    if (const int rc = point_query_check(b, n, flags, d_bboxes && (self || d_queries6), fault, who); rc || n == 0) return rc;
    if (const int rc = source_array_check(b, n_boxes, "boxes", who, stream)) return rc;
    const unsigned run_flags = self ? flags | BVH_AMD_RAY_UNSORTED : flags;
    return point_query_run<T, kQueryBoxes>(b, d_bboxes, d_queries6, n, run_flags, d_counters, sizeof(uint32_t), kBlock, kPointSortMin, kPointKeyBits, who, stream,
                                    [&](const PointArgs<T>& args, T*) {
        const OverlapArgs<T> a{{args, d_counts, reinterpret_cast<const unsigned long long*>(d_offsets), d_list_prims}, b.d_prim_ids};
        // (the ladder's leaf kind is unused here: a box is a box)
        return list_query_dispatch(LEAF_TRIANGLE, d_counters != nullptr, a.deep_cap != 0, a.offsets != nullptr, [&](auto, auto stats, auto deep, auto fill) {
            return self ? point_query_launch(overlap_kernel<T, stats(), deep(), fill(), true>, a, kBlock, 0, stream)
                        : point_query_launch(overlap_kernel<T, stats(), deep(), fill(), false>, a, kBlock, 0, stream);
        });
    });
}

template int launch_overlap<float>(const BvhImpl<float>&, bool, const float*, size_t, const float*, size_t, unsigned, uint32_t*, const uint64_t*, uint32_t*,
                                   bvh_amd_counters*, hipStream_t);
template int launch_overlap<double>(const BvhImpl<double>&, bool, const double*, size_t, const double*, size_t, unsigned, uint32_t*, const uint64_t*, uint32_t*,
                                    bvh_amd_counters*, hipStream_t);

} // namespace bvh_amd
