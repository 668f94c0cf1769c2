// Per-lane body of the batched triangle-intersection query (tri_intersect.hip): every BVH-order primitive whose TRIANGLE intersects a
// query triangle, as a count and, optionally, a list in the query's segment of a caller-sized buffer: the narrow phase of a collision
// test, inside the walk of the broad phase (overlap_body.inc). The triangles are the caller's array of 9 scalars {p0, p1, p2} indexed
// by ORIGINAL primitive id (what bvh3X_refit_tris takes): the triangle of BVH-order primitive i is tris[tri_ids[i]]. In self mode the
// query IS BVH-order primitive `slot` and only i > slot is listed: every unordered intersecting pair once.
//
// The test (tri_pair.inc; closed sets: touching counts, and so does coplanar containment) takes its decision from SIGNS of determinants of
// coordinate differences only, after Guigue and Devillers ("Fast and robust triangle-triangle overlap test using orientation
// predicates", 2003): the side of each vertex of one triangle against the plane of the other (a difference dotted with the plane's
// normal, itself three 2 x 2 determinants of differences), two 3 x 3 determinants that order the triangles' intervals on the line the
// planes share and, for coplanar triangles, 2 x 2 orientations in the projection along the normal's largest component. No division, no
// square root, no epsilon, and never a product of two determinants: whenever every determinant is computed without rounding the answer
// is the exact one. The vertex permutations of the interval step are selects on the sign pattern, not a tree of branches: the lanes
// of a wave hold different patterns.
// Kept as an include so that tests/cpp/tri_intersect_body_host.cpp compiles the very same text for the host (one emulated lane per
// query). Expects what point_walk.inc expects.
#pragma once

#include "list_walk.inc"
#include "tri_pair.inc"                        // the triangle helpers and the pair test; the box test of the walk is point_walk.inc's

namespace bvh_amd {

namespace {

constexpr int kTriIntersectLds = kListLds;     // the kernel and the harness size their LDS array by this name

template <typename T>
struct TriIntersectArgs : ListArgs<T> {        // prims = the triangles, n_tris x {p0.xyz, p1.xyz, p2.xyz} by original id; queries = n x the same (null: self mode)
    const uint32_t* tri_ids;                   // BVH-order index -> original id (always; prim_ids is set only to REPORT original ids)
    uint32_t skip_shared;                      // BVH_AMD_TRI_SKIP_SHARED: a pair with a common vertex is not listed
};

// One query, one lane: list_walk (which has the order of the walk and the shape of the output), a child entered iff its box overlaps
// the query triangle's box, every primitive whose triangle intersects the query's a match, the unused rest of a segment padded with
// BVH_AMD_INVALID. Self: the query is the triangle of BVH-order primitive qi = slot, primitives i <= qi are skipped before anything
// of theirs is fetched. Slot `slot` of the launch (query order[slot], or slot itself); `lane` indexes the HBM spill (Deep), `tid` the
// LDS array. cnt += {pair records fetched, triangles fetched, leaves visited}.
template <typename T, bool Stats, bool Deep, bool Fill, bool Self>
__device__ inline void tri_intersect_lane(const TriIntersectArgs<T>& a, unsigned long long slot, uint32_t* lds_node, int tid, unsigned long long lane,
                                          unsigned long long (&cnt)[3]) {
    const unsigned long long qi = !Self && a.order ? a.order[slot] : slot;
    T q[9], lo[3], hi[3], nq[3];
    load_tri9(Self ? a.prims + 9ull * a.tri_ids[qi] : a.queries + 9ull * qi, q);
    tri_box(q, lo, hi);
    tri_normal(q, nq);
    const bool valid = normal_usable(nq);                     // no area, a NaN or an infinite coordinate: an empty list
    const bool skip_shared = a.skip_shared != 0;

    list_walk<T, Stats, Deep, Fill>(a, qi, valid, lds_node, tid, lane, cnt,
        [&](const T (&box)[6]) { return node_overlaps(box, lo, hi); },
        [&](uint32_t i, unsigned long long at, bool room) {
            if (Self && i <= qi) return false;
            if (Stats) ++cnt[1];
            const uint32_t id = a.tri_ids[i];
            T t[9];
            load_tri9(a.prims + 9ull * id, t);
            if (!tri_pair_intersects(q, lo, hi, nq, t, skip_shared)) return false;
            if (room) store_stream(a.list_prims + at, a.prim_ids ? id : i);
            return true;
        },
        [&](unsigned long long at) { store_stream(a.list_prims + at, BVH_AMD_INVALID); });
}

} // namespace

} // namespace bvh_amd
