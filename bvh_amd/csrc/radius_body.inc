// Per-lane body of the batched radius query (radius.hip): every BVH-order primitive — a PrecomputedTri or a Sphere — within
// max_distance of a query point, as a count and, optionally, a list in the query's segment of a caller-sized buffer. The distance
// functions are those of closest_body.inc (tri_dist2 / sphere_dist2 / box_dist2), so "within" means exactly what closest_points
// measures. Kept as an include so that tests/cpp/radius_body_host.cpp compiles the very same text for the host (one emulated lane
// per query). Expects what closest_body.inc expects. Compiled with -ffp-contract=off on both sides, division and square root
// correctly rounded: host and device produce the same bits.
#pragma once

#include "closest_body.inc"

namespace bvh_amd {

namespace {

// Stack entries of a lane held in LDS (node words only, one [depth][lane] array, conflict-free), the rest of the first 64 in
// per-lane scratch, entries beyond 64 (trees deeper than 64 levels only) in HBM. The walk pushes at most one entry per level, so the
// tree's depth bounds the stack. Without a distance beside the node word, 16 entries cost the 16 KB per block that closest_lane
// spends on 8 of float queries: eight blocks per CU stay resident (128 KB of the 160 KB of LDS), which is the most the register
// budget of these kernels allows anyway (DESIGN.md, "Radius queries").
constexpr int kRadiusLds = 16;
constexpr int kRadiusSmall = 64;

template <typename T>
struct RadiusArgs {
    const PairNode<T>* pairs;
    const T* prims;                            // BVH order: PrecomputedTri (12 scalars) or Sphere<T, 3> (4 scalars)
    const T* queries;                          // {x, y, z, max_distance} per query, caller order
    uint32_t* counts;                          // optional: primitives within the radius per query (never truncated), caller order
    const unsigned long long* offsets;         // Fill kernels only: query q owns [offsets[q], offsets[q + 1]) of the list arrays
    uint32_t* list_prims;                      // Fill kernels only
    T* list_dist;                              // Fill kernels only, optional: sqrt(d2) beside each listed primitive
    unsigned long long n;                      // slots of this launch: [first, first + n)
    unsigned long long first;
    const uint32_t* order;                     // optional: slot -> query index (coherence sort); results are unaffected
    const uint32_t* prim_ids;                  // optional: list prim_ids[i] instead of the BVH-order index i (BVH_AMD_RAY_ORIGINAL_IDS)
    bvh_amd_counters* counters;                // Stats kernels only
    uint32_t* deep_nodes;                      // Deep kernels only: deep_cap entries per lane of the launch beyond the 64 of LDS + scratch
    uint32_t deep_cap;
    uint32_t root_index;
};

// A list entry is written once, by one lane, and not read again by the launch; neighbouring lanes write far apart. Marked
// non-temporal so that the lists do not take lines of the L2 away from the records and primitives the walks share.
__device__ inline void store_list(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}
__device__ inline void store_list(float* p, float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}
__device__ inline void store_list(double* p, double v) {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}

// One query, one lane: depth-first walk, the left child's subtree before the right's, a child entered iff its box is within the
// radius (box_dist2 <= max_distance^2); inside a leaf the BVH-order index ascends. Every primitive with d2 <= max_distance^2 is
// counted; with Fill the first (segment length) of them are listed in walk order and the rest of the segment is padded with
// {BVH_AMD_INVALID, max_distance}. Nothing is pruned against what was found, so the list depends on the tree, the primitives and the
// query only. Slot `slot` of the launch (query order[slot], or slot itself); `lane` indexes the HBM spill (Deep), `tid` the LDS
// array. cnt += {pair records fetched, primitives tested, leaves visited}.
template <typename T, int Leaf, bool Stats, bool Deep, bool Fill>
__device__ inline void radius_lane(const RadiusArgs<T>& a, unsigned long long slot, uint32_t* lds_node, int tid, unsigned long long lane,
                                   unsigned long long (&cnt)[3]) {
    const unsigned long long qi = a.order ? a.order[slot] : slot;
    T qq[4];
    load_prim4(a.queries + 4ull * qi, qq);
    const T q[3] = { qq[0], qq[1], qq[2] };
    const T max_d = qq[3];
    const T r2 = max_d * max_d;
    const bool valid = q[0] == q[0] && q[1] == q[1] && q[2] == q[2] && max_d >= T(0);   // NaN coordinates / radius, negative radius: empty list

    unsigned long long seg_begin = 0, seg_len = 0;
    if (Fill) {
        seg_begin = a.offsets[qi];
        const unsigned long long seg_end = a.offsets[qi + 1];
        seg_len = seg_end > seg_begin ? seg_end - seg_begin : 0;               // (offsets that do not ascend: an empty segment)
    }
    uint32_t found = 0;

    uint32_t spill_node[kRadiusSmall - kRadiusLds];
    uint32_t sp = 0;
    auto deep_at = [&](uint32_t i) { return lane * a.deep_cap + (i < a.deep_cap ? i : a.deep_cap - 1); };
    auto push = [&](uint32_t node) {
        if (sp < kRadiusLds) lds_node[sp * kBlock + tid] = node;
        else if (!Deep || sp < kRadiusSmall) {
            const uint32_t i = sp - kRadiusLds < uint32_t(kRadiusSmall - kRadiusLds - 1) ? sp - kRadiusLds : uint32_t(kRadiusSmall - kRadiusLds - 1);
            spill_node[i] = node;
        } else a.deep_nodes[deep_at(sp - kRadiusSmall)] = node;
        ++sp;
    };
    auto pop = [&](uint32_t& node) -> bool {
        if (sp == 0) return false;
        --sp;
        if (sp < kRadiusLds) node = lds_node[sp * kBlock + tid];
        else if (!Deep || sp < kRadiusSmall) {
            const uint32_t i = sp - kRadiusLds < uint32_t(kRadiusSmall - kRadiusLds - 1) ? sp - kRadiusLds : uint32_t(kRadiusSmall - kRadiusLds - 1);
            node = spill_node[i];
        } else node = a.deep_nodes[deep_at(sp - kRadiusSmall)];
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
            T d2, u = T(0), v = T(0);
            if (Leaf == LEAF_TRIANGLE) {
                T p[12];
                load_prim12(a.prims + 12ull * i, p);
                d2 = tri_dist2(p, q, u, v);
            } else {
                T s[4];
                load_prim4(a.prims + 4ull * i, s);
                d2 = sphere_dist2(s, q);
            }
            if (d2 <= r2) {
                if (Fill && found < seg_len) {
                    store_list(a.list_prims + (seg_begin + found), a.prim_ids ? a.prim_ids[i] : i);
                    if (a.list_dist) store_list(a.list_dist + (seg_begin + found), Num<T>::sqrt_(d2));
                }
                ++found;
            }
        }
        live = pop(node);
    }
    if (a.counts) a.counts[qi] = found;
    if (Fill) {
        for (unsigned long long k = found; k < seg_len; ++k) {                  // the unused rest of the segment: closest_points' miss record
            store_list(a.list_prims + (seg_begin + k), BVH_AMD_INVALID);
            if (a.list_dist) store_list(a.list_dist + (seg_begin + k), max_d);
        }
    }
}

} // namespace

} // namespace bvh_amd
