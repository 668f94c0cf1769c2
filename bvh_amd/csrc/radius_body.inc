// Per-lane body of the batched radius query (radius.hip): every BVH-order primitive — a PrecomputedTri or a Sphere — within
// max_distance of a query point, as a count and, optionally, a list in the query's segment of a caller-sized buffer. The distance
// functions are point_walk.inc's (tri_dist2 / sphere_dist2 / box_dist2), so "within" means exactly what closest_points measures.
// Kept as an include so that tests/cpp/radius_body_host.cpp compiles the very same text for the host (one emulated lane per query).
// Expects what point_walk.inc expects.
#pragma once

#include "list_walk.inc"

namespace bvh_amd {

namespace {

constexpr int kRadiusLds = kListLds;           // the kernel and the harness size their LDS array by this name

template <typename T>
struct RadiusArgs : ListArgs<T> {            // counts = primitives within the radius
    T* list_dist;                              // Fill kernels only, optional: sqrt(d2) beside each listed primitive
};

// One query, one lane: list_walk (which has the order of the walk and the shape of the output), a child entered iff its box is
// within the radius (box_dist2 <= max_distance^2), every primitive with d2 <= max_distance^2 a match, the unused rest of a segment
// padded with {BVH_AMD_INVALID, max_distance}. Slot `slot` of the launch (query order[slot], or slot itself); `lane` indexes the HBM
// spill (Deep), `tid` the LDS array. cnt += {pair records fetched, primitives tested, leaves visited}.
template <typename T, int Leaf, bool Stats, bool Deep, bool Fill>
__device__ inline void radius_lane(const RadiusArgs<T>& a, unsigned long long slot, uint32_t* lds_node, int tid, unsigned long long lane,
                                   unsigned long long (&cnt)[3]) {
    unsigned long long qi;
    T q[3], max_d;
    const bool valid = load_query(a, slot, qi, q, max_d);    // NaN coordinates / radius, negative radius: empty list
    const T r2 = max_d * max_d;

    list_walk<T, Stats, Deep, Fill>(a, qi, valid, lds_node, tid, lane, cnt,
        [&](const T (&box)[6]) { return box_dist2(box, q) <= r2; },
        [&](uint32_t i, unsigned long long at, bool room) {
            if (Stats) ++cnt[1];
            T u = T(0), v = T(0);
            const T d2 = leaf_dist2<T, Leaf>(a.prims, i, q, u, v);
            if (!(d2 <= r2)) return false;
            if (room) {
                store_stream(a.list_prims + at, a.prim_ids ? a.prim_ids[i] : i);
                if (a.list_dist) store_stream(a.list_dist + at, Num<T>::sqrt_(d2));
            }
            return true;
        },
        [&](unsigned long long at) {                                            // the unused rest of the segment: closest_points' miss record
            store_stream(a.list_prims + at, BVH_AMD_INVALID);
            if (a.list_dist) store_stream(a.list_dist + at, max_d);
        });
}

} // namespace

} // namespace bvh_amd
