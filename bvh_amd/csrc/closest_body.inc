// Per-lane body of the batched closest-point query (closest.hip): one query's load, its two tests and its record around
// nearest_walk.inc, the pruned depth-first walk through the pair records that ray_nearest_body.inc, sphere_cast_body.inc and
// tri_distance_body.inc also run (knn_body.inc holds a copy of it); the LDS tier of its stack, kClosestLds, was measured on this query
// and stands beside the walk. The query load and the distance functions are point_walk.inc's. Kept as an include so that tests/cpp/closest_body_host.cpp
// compiles the very same text for the host (one emulated lane per query). Expects what point_walk.inc expects, and store_hit.
#pragma once

#include "nearest_walk.inc"

namespace bvh_amd {

namespace {

template <typename T>
struct ClosestArgs : PointArgs<T> {
    typename HitOf<T>::Type* hits;             // one record per query, caller order
    T* deep_d2;                                // Deep kernels only: beside deep_nodes
};

// One query, one lane: nearest_walk keyed by box distance^2 with `best` as its limit: nearer child first, the farther one pushed with
// its key; a child or popped entry farther than the best primitive so far is dropped. best starts at max_distance^2; among the primitives the walk TESTS, the lowest
// BVH-order index of those at the smallest computed squared distance wins, whatever the visiting order. A subtree is skipped when
// its box's computed distance^2 exceeds `best`, so a primitive whose computed distance rounds below its own leaf box's (a sphere's
// (fl(sqrt(s)) - r)^2 against the box's exact s; a triangle with area) can hide one at an equal or one-ulp-nearer distance in another
// leaf. The record is the brute force's (argmin by (d2, index)) exactly when the distances are computed exactly, otherwise its distance
// is within the tolerance of INTEGRATION.md 3b of it (tests/test_query_fuzz_host.py pins both; docs/HISTORY.md has the open item).
// Slot `slot` of the launch (query order[slot], or slot itself); `lane`
// indexes the HBM spill (Deep), `tid` the LDS arrays. cnt += {pair records fetched, primitives tested, leaves visited}.
template <typename T, int Leaf, bool Stats, bool Deep>
__device__ inline void closest_lane(const ClosestArgs<T>& a, unsigned long long slot, uint32_t* lds_node, T* lds_d2, int tid,
                                    unsigned long long lane, unsigned long long (&cnt)[3]) {
    unsigned long long qi;
    T q[3], max_d;
    const bool valid = load_query(a, slot, qi, q, max_d);    // NaN coordinates / radius, negative radius: miss
    uint32_t best_prim = BVH_AMD_INVALID;
    T best = max_d * max_d, best_u = T(0), best_v = T(0);

    nearest_walk<T, kClosestLds, Stats, Deep>(a, valid, lds_node, lds_d2, uint32_t(kBlock), tid, lane, a.deep_d2, best, cnt,
        [&](const T (&lb)[6], const T (&rb)[6], T& dl, T& dr, bool& hl, bool& hr) {
            dl = box_dist2(lb, q); dr = box_dist2(rb, q);
            hl = dl <= best; hr = dr <= best;
        },
        [&](uint32_t i) {
            T u = T(0), v = T(0);
            const T d2 = leaf_dist2<T, Leaf>(a.prims, i, q, u, v);
            if (d2 < best || (d2 == best && i < best_prim)) { best = d2; best_prim = i; best_u = u; best_v = v; }
        });
    if (best_prim != BVH_AMD_INVALID) {
        store_hit(a.hits + qi, a.prim_ids ? a.prim_ids[best_prim] : best_prim, Num<T>::sqrt_(best), best_u, best_v);
    } else {
        store_hit(a.hits + qi, BVH_AMD_INVALID, max_d, T(0), T(0));
    }
}

} // namespace

} // namespace bvh_amd
