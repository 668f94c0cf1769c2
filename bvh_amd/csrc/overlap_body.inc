// Per-lane body of the batched box-overlap query (overlap.hip): every BVH-order primitive whose box overlaps a query box, as a count
// and, optionally, a list in the query's segment of a caller-sized buffer. The boxes are the caller's array indexed by ORIGINAL
// primitive id (what bvhXX_build_device and bvhXX_refit_boxes take): the box of BVH-order primitive i is bboxes[box_ids[i]], so the
// query does not care what kind of primitive the tree was built over. In self mode the query IS BVH-order primitive `slot` and only
// i > slot is listed: every unordered overlapping pair once.
// The box tests (load_box6, node_overlaps, box_overlaps) are point_walk.inc's, where tri_pair.inc and tri_intersect_body.inc find them too.
// Kept as an include so that tests/cpp/overlap_body_host.cpp compiles the very same text for the host (one emulated lane per query).
// Expects what point_walk.inc expects.
#pragma once

#include "list_walk.inc"

namespace bvh_amd {

namespace {

constexpr int kOverlapLds = kListLds;          // the kernel and the harness size their LDS array by this name

template <typename T>
struct OverlapArgs : ListArgs<T> {           // prims = the boxes, n_boxes x {min.xyz, max.xyz} by original id; queries = n x the same (null: self mode)
    const uint32_t* box_ids;                   // BVH-order index -> original id (always; prim_ids is set only to REPORT original ids)
};

// One query, one lane: list_walk (which has the order of the walk and the shape of the output), a child entered iff its box overlaps
// the query, every primitive whose box overlaps a match, the unused rest of a segment padded with BVH_AMD_INVALID.
// Self: the query is the box of BVH-order primitive qi = slot, primitives i <= qi are skipped before their box is fetched.
// Slot `slot` of the launch (query order[slot], or slot itself); `lane` indexes the HBM spill (Deep), `tid` the LDS array.
// cnt += {pair records fetched, primitive boxes tested, leaves visited}.
template <typename T, bool Stats, bool Deep, bool Fill, bool Self>
__device__ inline void overlap_lane(const OverlapArgs<T>& a, unsigned long long slot, uint32_t* lds_node, int tid, unsigned long long lane,
                                    unsigned long long (&cnt)[3]) {
    const unsigned long long qi = !Self && a.order ? a.order[slot] : slot;
    T lo[3], hi[3];
    load_box6(Self ? a.prims + 6ull * a.box_ids[qi] : a.queries + 6ull * qi, lo, hi);
    const bool valid = lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2];     // a NaN component, min > max: an empty list

    list_walk<T, Stats, Deep, Fill>(a, qi, valid, lds_node, tid, lane, cnt,
        [&](const T (&box)[6]) { return node_overlaps(box, lo, hi); },
        [&](uint32_t i, unsigned long long at, bool room) {
            if (Self && i <= qi) return false;
            if (Stats) ++cnt[1];
            const uint32_t id = a.box_ids[i];
            T bl[3], bh[3];
            load_box6(a.prims + 6ull * id, bl, bh);
            if (!box_overlaps(bl, bh, lo, hi)) return false;
            if (room) store_stream(a.list_prims + at, a.prim_ids ? id : i);
            return true;
        },
        [&](unsigned long long at) { store_stream(a.list_prims + at, BVH_AMD_INVALID); });
}

} // namespace

} // namespace bvh_amd
