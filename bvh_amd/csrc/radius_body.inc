// Per-lane body of the batched radius query (radius.hip): every BVH-order primitive — a PrecomputedTri or a Sphere — within
// max_distance of a query point, as a count and, optionally, a list in the query's segment of a caller-sized buffer. The distance
// functions are point_walk.inc's (tri_dist2 / sphere_dist2 / box_dist2), so "within" means exactly what closest_points measures.
// Kept as an include so that tests/cpp/radius_body_host.cpp compiles the very same text for the host (one emulated lane per query).
// Expects what point_walk.inc expects.
#pragma once

#include "point_walk.inc"

namespace bvh_amd {

namespace {

// Stack entries of a lane held in LDS (node words only, one [depth][lane] array), the rest in scratch and HBM (point_walk.inc has the
// tiers). Without a distance beside the node word, 16 entries cost the 16 KB per block that closest_lane
// spends on 8 of float queries: eight blocks per CU stay resident (128 KB of the 160 KB of LDS), which is the most the register
// budget of these kernels allows anyway (DESIGN.md, "Radius queries").
constexpr int kRadiusLds = 16;

template <typename T>
struct RadiusArgs : PointArgs<T> {
    uint32_t* counts;                          // optional: primitives within the radius per query (never truncated), caller order
    const unsigned long long* offsets;         // Fill kernels only: query q owns [offsets[q], offsets[q + 1]) of the list arrays
    uint32_t* list_prims;                      // Fill kernels only
    T* list_dist;                              // Fill kernels only, optional: sqrt(d2) beside each listed primitive
};

// One query, one lane: depth-first walk, the left child's subtree before the right's, a child entered iff its box is within the
// radius (box_dist2 <= max_distance^2); inside a leaf the BVH-order index ascends. Every primitive with d2 <= max_distance^2 is
// counted; with Fill the first (segment length) of them are listed in walk order and the rest of the segment is padded with
// {BVH_AMD_INVALID, max_distance}. Nothing is pruned against what was found, so the list depends on the tree, the primitives and the
// query only. Slot `slot` of the launch (query order[slot], or slot itself); `lane` indexes the HBM spill (Deep), `tid` the LDS
// array. cnt += {pair records fetched, primitives tested, leaves visited}.
template <typename T, int Leaf, bool Stats, bool Deep, bool Fill>
__device__ inline void radius_lane(const RadiusArgs<T>& a, unsigned long long slot, uint32_t* lds_node, int tid, unsigned long long lane,
                                   unsigned long long (&cnt)[3]) {
    unsigned long long qi;
    T q[3], max_d;
    const bool valid = load_query(a, slot, qi, q, max_d);    // NaN coordinates / radius, negative radius: empty list
    const T r2 = max_d * max_d;

    unsigned long long seg_begin = 0, seg_len = 0;
    if (Fill) {
        seg_begin = a.offsets[qi];
        const unsigned long long seg_end = a.offsets[qi + 1];
        seg_len = seg_end > seg_begin ? seg_end - seg_begin : 0;               // (offsets that do not ascend: an empty segment)
    }
    uint32_t found = 0;

    uint32_t spill_node[kPointSmall - kRadiusLds];
    uint32_t sp = 0;
    auto push = [&](uint32_t node) {
        if (sp < kRadiusLds) lds_node[sp * kBlock + tid] = node;
        else if (!Deep || sp < kPointSmall) spill_node[stack_small_at<kRadiusLds>(sp)] = node;
        else a.deep_nodes[stack_deep_at(a, lane, sp)] = node;
        ++sp;
    };
    auto pop = [&](uint32_t& node) -> bool {
        if (sp == 0) return false;
        --sp;
        if (sp < kRadiusLds) node = lds_node[sp * kBlock + tid];
        else if (!Deep || sp < kPointSmall) node = spill_node[stack_small_at<kRadiusLds>(sp)];
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
            const bool hl = box_dist2(lb, q) <= r2, hr = box_dist2(rb, q) <= r2;
            if (hl && hr) { push(ri); node = li; }
            else if (hl) node = li;
            else if (hr) node = ri;
            else if (!pop(node)) { live = false; break; }
        }
        if (!live) break;
        const uint32_t first = node >> kCountBits, count = node & kCountMask;
        if (Stats) ++cnt[2];
        // (one primitive at a time: left alone, the compiler turns the bare counting loop of the <Stats, Deep, Fill = false> triangle
        //  kernel into a two-wide interleaved one of 103 VGPRs, 4 waves per SIMD, against the 58-68 and 7-8 waves of its siblings)
#pragma clang loop vectorize(disable) interleave(disable)
        for (uint32_t i = first; i < first + count; ++i) {
            if (Stats) ++cnt[1];
            T u = T(0), v = T(0);
            const T d2 = leaf_dist2<T, Leaf>(a.prims, i, q, u, v);
            if (d2 <= r2) {
                if (Fill && found < seg_len) {
                    store_stream(a.list_prims + (seg_begin + found), a.prim_ids ? a.prim_ids[i] : i);
                    if (a.list_dist) store_stream(a.list_dist + (seg_begin + found), Num<T>::sqrt_(d2));
                }
                ++found;
            }
        }
        live = pop(node);
    }
    if (a.counts) a.counts[qi] = found;
    if (Fill) {
        for (unsigned long long k = found; k < seg_len; ++k) {                  // the unused rest of the segment: closest_points' miss record
            store_stream(a.list_prims + (seg_begin + k), BVH_AMD_INVALID);
            if (a.list_dist) store_stream(a.list_dist + (seg_begin + k), max_d);
        }
    }
}

} // namespace

} // namespace bvh_amd
