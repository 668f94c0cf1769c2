// Per-lane body of the batched box-overlap query (overlap.hip): every BVH-order primitive whose box overlaps a query box, as a count
// and, optionally, a list in the query's segment of a caller-sized buffer. The boxes are the caller's array indexed by ORIGINAL
// primitive id (what bvhXX_build_device and bvhXX_refit_boxes take): the box of BVH-order primitive i is bboxes[box_ids[i]], so the
// query does not care what kind of primitive the tree was built over. In self mode the query IS BVH-order primitive `slot` and only
// i > slot is listed: every unordered overlapping pair once.
// Kept as an include so that tests/cpp/overlap_body_host.cpp compiles the very same text for the host (one emulated lane per query).
// Expects what point_walk.inc expects.
#pragma once

#include "point_walk.inc"

namespace bvh_amd {

namespace {

// Stack entries of a lane held in LDS: bare node words in one [depth][lane] array, as radius_body.inc keeps them (16 KB per block).
constexpr int kOverlapLds = 16;

template <typename T>
struct OverlapArgs : PointArgs<T> {            // prims = the boxes, n_boxes x {min.xyz, max.xyz} by original id; queries = n x the same (null: self mode)
    const uint32_t* box_ids;                   // BVH-order index -> original id (always; prim_ids is set only to REPORT original ids)
    uint32_t* counts;                          // optional: overlapping primitives per query (never truncated), caller order
    const unsigned long long* offsets;         // Fill kernels only: query q owns [offsets[q], offsets[q + 1]) of list_prims
    uint32_t* list_prims;                      // Fill kernels only
};

// A box {min.xyz, max.xyz} of the caller's arrays (aligned to its scalar only).
template <typename T>
__device__ inline void load_box6(const T* p, T (&lo)[3], T (&hi)[3]) {
    lo[0] = p[0]; lo[1] = p[1]; lo[2] = p[2];
    hi[0] = p[3]; hi[1] = p[4]; hi[2] = p[5];
}

// Closed intervals on one axis: [lo, hi] is the query's, already known to be proper (lo <= hi); [bmin, bmax] overlaps it iff it is
// proper itself and neither lies wholly before the other. A NaN makes the comparison it is part of false; -0 equals +0.
template <typename T>
__device__ inline bool axis_overlaps(T bmin, T bmax, T lo, T hi) { return bmin <= hi && lo <= bmax && bmin <= bmax; }

// The one test of the walk, for a child's box of a pair record {minx, maxx, miny, maxy, minz, maxz} ...
template <typename T>
__device__ inline bool node_overlaps(const T (&b)[6], const T (&lo)[3], const T (&hi)[3]) {
    return axis_overlaps(b[0], b[1], lo[0], hi[0]) && axis_overlaps(b[2], b[3], lo[1], hi[1]) && axis_overlaps(b[4], b[5], lo[2], hi[2]);
}
// ... and for a primitive's box {min.xyz}, {max.xyz}.
template <typename T>
__device__ inline bool box_overlaps(const T (&bl)[3], const T (&bh)[3], const T (&lo)[3], const T (&hi)[3]) {
    return axis_overlaps(bl[0], bh[0], lo[0], hi[0]) && axis_overlaps(bl[1], bh[1], lo[1], hi[1]) && axis_overlaps(bl[2], bh[2], lo[2], hi[2]);
}

// One query, one lane: depth-first walk, the left child's subtree before the right's, a child entered iff its box overlaps the query;
// inside a leaf the BVH-order index ascends. Every primitive whose box overlaps is counted; with Fill the first (segment length) of
// them are listed in walk order and the rest of the segment is padded with BVH_AMD_INVALID. Nothing is pruned against what was found.
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

    unsigned long long seg_begin = 0, seg_len = 0;
    if (Fill) {
        seg_begin = a.offsets[qi];
        const unsigned long long seg_end = a.offsets[qi + 1];
        seg_len = seg_end > seg_begin ? seg_end - seg_begin : 0;               // (offsets that do not ascend: an empty segment)
    }
    uint32_t found = 0;

    uint32_t spill_node[kPointSmall - kOverlapLds];
    uint32_t sp = 0;
    auto push = [&](uint32_t node) {
        if (sp < kOverlapLds) lds_node[sp * kBlock + tid] = node;
        else if (!Deep || sp < kPointSmall) spill_node[stack_small_at<kOverlapLds>(sp)] = node;
        else a.deep_nodes[stack_deep_at(a, lane, sp)] = node;
        ++sp;
    };
    auto pop = [&](uint32_t& node) -> bool {
        if (sp == 0) return false;
        --sp;
        if (sp < kOverlapLds) node = lds_node[sp * kBlock + tid];
        else if (!Deep || sp < kPointSmall) node = spill_node[stack_small_at<kOverlapLds>(sp)];
        else node = a.deep_nodes[stack_deep_at(a, lane, sp)];
        return true;
    };

    uint32_t node = a.root_index;
    bool live = valid;
    while (live) {
        while ((node & kCountMask) == 0) {                    // inner node: both children in one record
            T lb[6], rb[6];
            uint32_t li = 0, ri = 0;
            load_pair(a.pairs + (node >> (kCountBits + 1)), lb, rb, li, ri);
            if (Stats) ++cnt[0];
            const bool hl = node_overlaps(lb, lo, hi), hr = node_overlaps(rb, lo, hi);
            if (hl && hr) { push(ri); node = li; }
            else if (hl) node = li;
            else if (hr) node = ri;
            else if (!pop(node)) { live = false; break; }
        }
        if (!live) break;
        const uint32_t first = node >> kCountBits, count = node & kCountMask;
        if (Stats) ++cnt[2];
        // (one primitive at a time, as in radius_lane: an interleaved loop costs registers and the gathers are dependent anyway)
#pragma clang loop vectorize(disable) interleave(disable)
        for (uint32_t i = first; i < first + count; ++i) {
            if (Self && i <= qi) continue;
            if (Stats) ++cnt[1];
            const uint32_t id = a.box_ids[i];
            T bl[3], bh[3];
            load_box6(a.prims + 6ull * id, bl, bh);
            if (box_overlaps(bl, bh, lo, hi)) {
                if (Fill && found < seg_len) store_stream(a.list_prims + (seg_begin + found), a.prim_ids ? id : i);
                ++found;
            }
        }
        live = pop(node);
    }
    if (a.counts) a.counts[qi] = found;
    if (Fill) {
        for (unsigned long long k = found; k < seg_len; ++k) store_stream(a.list_prims + (seg_begin + k), BVH_AMD_INVALID);
    }
}

} // namespace

} // namespace bvh_amd
