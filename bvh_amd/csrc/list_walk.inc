// What the per-lane bodies of the list queries share (radius_body.inc, overlap_body.inc, tri_intersect_body.inc, region_body.inc,
// ray_hits_body.inc): the output arguments, and the one walk
// that counts every match of a query and lists the first of them in the query's segment of a caller-sized buffer. The bodies supply
// the query, the two tests and the stores. Kept as an include so that the host harnesses (tests/cpp/radius_body_host.cpp,
// overlap_body_host.cpp, tri_intersect_body_host.cpp, region_body_host.cpp, ray_hits_body_host.cpp) compile the very same text,
// through the bodies. Expects what point_walk.inc expects.
#pragma once

#include "point_walk.inc"

namespace bvh_amd {

namespace {

// Stack entries of a lane held in LDS (node words only, one [depth][lane] array), the rest in scratch and HBM (point_walk.inc has the
// tiers). Without a distance beside the node word, 16 entries cost the 16 KB per block that closest_lane
// spends on 8 of float queries: eight blocks per CU stay resident (128 KB of the 160 KB of LDS), which is the most the register
// budget of these kernels allows anyway (DESIGN.md, "Radius queries").
constexpr int kListLds = 16;

template <typename T>
struct ListArgs : PointArgs<T> {
    uint32_t* counts;                          // optional: matches per query (never truncated), caller order
    const unsigned long long* offsets;         // Fill kernels only: query q owns [offsets[q], offsets[q + 1]) of the list arrays
    uint32_t* list_prims;                      // Fill kernels only (unused by the ray query, whose list is one array of hit records)
};

// One query, one lane: depth-first walk from the root, the left child's subtree before the right's, a child entered iff
// enter(its box {minx, maxx, miny, maxy, minz, maxz}); inside a leaf the BVH-order index ascends. hit(i, at, room) tests BVH-order
// primitive i, adds to cnt[1] what it counts as a test and, when i matches and `room` is set, stores its entry at position `at` of the
// list arrays; it returns whether i matched. Every match is counted; with Fill the first (segment length) of them are listed in walk
// order and pad(at) fills the rest of the segment. Nothing is pruned against what was found, so the list depends on the tree, the
// primitives and the query only. qi = the query's index in the caller's order, valid = false: an empty list; `lane` indexes the HBM
// spill (Deep), `tid` the LDS array of kListLds * kBlock words. cnt += {pair records fetched, (hit's), leaves visited}.
// push / pop are written here, on arrays this function names: see point_walk.inc on why they are not behind a struct.
template <typename T, bool Stats, bool Deep, bool Fill, typename Enter, typename Hit, typename Pad>
__device__ inline void list_walk(const ListArgs<T>& a, unsigned long long qi, bool valid, uint32_t* lds_node, int tid, unsigned long long lane,
                                 unsigned long long (&cnt)[3], Enter enter, Hit hit, Pad pad) {
    unsigned long long seg_begin = 0, seg_len = 0;
    if (Fill) {
        seg_begin = a.offsets[qi];
        const unsigned long long seg_end = a.offsets[qi + 1];
        seg_len = seg_end > seg_begin ? seg_end - seg_begin : 0;               // (offsets that do not ascend: an empty segment)
    }
    uint32_t found = 0;

    uint32_t spill_node[kPointSmall - kListLds];
    uint32_t sp = 0;
    auto push = [&](uint32_t node) {
        if (sp < kListLds) lds_node[sp * kBlock + tid] = node;
        else if (!Deep || sp < kPointSmall) spill_node[stack_small_at<kListLds>(sp)] = node;
        else a.deep_nodes[stack_deep_at(a, lane, sp)] = node;
        ++sp;
    };
    auto pop = [&](uint32_t& node) -> bool {
        if (sp == 0) return false;
        --sp;
        if (sp < kListLds) node = lds_node[sp * kBlock + tid];
        else if (!Deep || sp < kPointSmall) node = spill_node[stack_small_at<kListLds>(sp)];
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
            const bool hl = enter(lb), hr = enter(rb);
            if (hl && hr) { push(ri); node = li; }
            else if (hl) node = li;
            else if (hr) node = ri;
            else if (!pop(node)) { live = false; break; }
        }
        if (!live) break;
        const uint32_t first = node >> kCountBits, count = node & kCountMask;
        if (Stats) ++cnt[2];
        // (one primitive at a time: left alone, the compiler turns the bare counting loop of the <Stats, Deep, Fill = false> triangle
        //  radius kernel into a two-wide interleaved one of 103 VGPRs, 4 waves per SIMD, against the 58-68 and 7-8 waves of its
        //  siblings; the box gathers of the overlap kernels are dependent anyway)
#pragma clang loop vectorize(disable) interleave(disable)
        for (uint32_t i = first; i < first + count; ++i) {
            if (hit(i, seg_begin + found, Fill && found < seg_len)) ++found;
        }
        live = pop(node);
    }
    if (a.counts) a.counts[qi] = found;
    if (Fill) {
        for (unsigned long long k = found; k < seg_len; ++k) pad(seg_begin + k);
    }
}

} // namespace

} // namespace bvh_amd
