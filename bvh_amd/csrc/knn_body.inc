// Per-lane body of the batched k-nearest query (knn.hip): the k BVH-order primitives — PrecomputedTri or Sphere — nearest to a query
// point within max_distance, as a row of k {index, distance} slots in ascending (squared distance, index) order: the k smallest
// (d2, index) among the primitives the walk TESTS. Those are all of the scene's when the distances are computed exactly; with rounded
// distances a primitive computed nearer than its own leaf box can hide an equal or one-ulp-nearer one in a skipped subtree, and the
// row's distances then differ from the brute force's by rounding only (closest_body.inc; docs/HISTORY.md has the open item).
// The distance functions are point_walk.inc's (tri_dist2 / sphere_dist2 / box_dist2), so a distance is exactly what closest_points
// measures, and the walk is closest_lane's with the best distance replaced by the worst of the k held: k = 1 gives closest_points'
// primitive, distance and counters. Kept as an include so that tests/cpp/knn_body_host.cpp compiles the very same text for the host
// (one emulated lane per query). The candidate set, its two operations and its LDS layout are knn_heap.inc (shared with
// ray_nearest_body.inc). Expects what point_walk.inc expects.
// The walk below is a COPY of nearest_walk.inc's text (the stack, push / pop, the descent, the leaf loop), which closest_lane and
// ray_nearest_lane call: knn_lane built on that function computes the same bytes, but every float-triangle row of tools/knn_bench.py
// came out 1 - 3.5 % slower in each of two alternated runs (DESIGN.md, "Nearest queries: the one walk": same instructions, another
// packing of the two box distances and other registers), so this kind keeps its text. A fix to one belongs in the other.
#pragma once

#include "point_walk.inc"
#include "knn_heap.inc"

namespace bvh_amd {

namespace {

template <typename T>
struct KnnArgs : PointArgs<T> {
    uint32_t* out_prims;                       // n x k, row-major, caller order
    T* out_dist;                               // optional: n x k, sqrt(d2) beside each listed primitive
    uint32_t* counts;                          // optional: valid entries per row (<= k)
    T* deep_d2;                                // Deep kernels only: beside deep_nodes
    uint32_t k;                                // 1 .. BVH_AMD_KNN_MAX_K
};

// One query, one lane: closest_lane's walk — depth-first, nearer child first (ties left), the farther one pushed with its box
// distance^2 — pruned against `worst`: max_distance^2 until k candidates are held, then the d2 of the largest (d2, index) held. A
// child or a popped entry is kept iff its box distance^2 <= worst (not <: a primitive at the same distance with a lower index
// stays reachable wherever its box is not computed farther than `worst`). Inside a leaf the index ascends; a primitive is offered
// to the candidate set (knn_offer): while fewer than k are held it is taken iff d2 <= max_distance^2, afterwards iff (d2, index) is
// below the largest held, which it replaces. At the end knn_sort leaves the candidates ascending, and the row is
// written: nothing is stored while walking, so an invalid query still pads its row. Slot `slot` of the launch (query order[slot], or
// slot itself); `lane` indexes the HBM spill (Deep), `tid` and `stride` the LDS arrays. cnt += {pair records fetched, primitives
// tested, leaves visited}.
template <typename T, int Leaf, bool Stats, bool Deep>
__device__ inline void knn_lane(const KnnArgs<T>& a, unsigned long long slot, const KnnLds<T>& lds, uint32_t stride, int tid, unsigned long long lane,
                                unsigned long long (&cnt)[3]) {
    unsigned long long qi;
    T q[3], max_d;
    const bool valid = load_query(a, slot, qi, q, max_d);    // NaN coordinates / radius, negative radius: empty row
    const T r2 = max_d * max_d;
    const uint32_t k = a.k;
    T* const cand_d2 = lds.cand_key;
    uint32_t* const cand_id = lds.cand_id;
    T worst = r2;                                             // the pruning distance^2
    uint32_t worst_id = BVH_AMD_INVALID;                      // the index beside it, once k are held
    uint32_t held = 0;

    uint32_t spill_node[kPointSmall - kKnnLds];
    T spill_d2[kPointSmall - kKnnLds];
    uint32_t sp = 0;
    auto push = [&](uint32_t node, T d2) {
        if (sp < kKnnLds) { lds.stack_node[sp * stride + tid] = node; lds.stack_key[sp * stride + tid] = d2; }
        else if (!Deep || sp < kPointSmall) { const uint32_t i = stack_small_at<kKnnLds>(sp); spill_node[i] = node; spill_d2[i] = d2; }
        else { const unsigned long long i = stack_deep_at(a, lane, sp); a.deep_nodes[i] = node; a.deep_d2[i] = d2; }
        ++sp;
    };
    // the next stacked entry that can still hold something below the worst candidate (false: the walk is over)
    auto pop = [&](uint32_t& node) -> bool {
        while (sp > 0) {
            --sp;
            uint32_t e;
            T d2;
            if (sp < kKnnLds) { e = lds.stack_node[sp * stride + tid]; d2 = lds.stack_key[sp * stride + tid]; }
            else if (!Deep || sp < kPointSmall) { const uint32_t i = stack_small_at<kKnnLds>(sp); e = spill_node[i]; d2 = spill_d2[i]; }
            else { const unsigned long long i = stack_deep_at(a, lane, sp); e = a.deep_nodes[i]; d2 = a.deep_d2[i]; }
            if (d2 <= worst) { node = e; return true; }
        }
        return false;
    };

    uint32_t node = a.root_index;
    bool live = valid;
    while (live) {
        while ((node & kCountMask) == 0) {                    // inner node: both children in one record
            T lb[6], rb[6];
            uint32_t li = 0, ri = 0;
            load_pair(a.pairs + (node >> (kCountBits + 1)), lb, rb, li, ri);
            if (Stats) ++cnt[0];
            const T dl = box_dist2(lb, q), dr = box_dist2(rb, q);
            const bool hl = dl <= worst, hr = dr <= worst;
            if (hl && hr) {
                if (dr < dl) { push(li, dl); node = ri; }
                else { push(ri, dr); node = li; }
            } else if (hl) node = li;
            else if (hr) node = ri;
            else if (!pop(node)) { live = false; break; }
        }
        if (!live) break;
        const uint32_t first = node >> kCountBits, count = node & kCountMask;
        if (Stats) ++cnt[2];
        for (uint32_t i = first; i < first + count; ++i) {
            if (Stats) ++cnt[1];
            T u = T(0), v = T(0);
            const T d2 = leaf_dist2<T, Leaf>(a.prims, i, q, u, v);
            knn_offer(cand_d2, cand_id, stride, tid, k, held, worst, worst_id, d2, i, d2 <= r2);
        }
        live = pop(node);
    }

    knn_sort(cand_d2, cand_id, stride, tid, k, held);         // ascending (d2, index)
    uint32_t* const row_prims = a.out_prims + qi * k;
    T* const row_dist = a.out_dist ? a.out_dist + qi * k : nullptr;
    for (uint32_t j = 0; j < held; ++j) {
        const uint32_t i = cand_id[j * stride + tid];
        store_stream(row_prims + j, a.prim_ids ? a.prim_ids[i] : i);
        if (row_dist) store_stream(row_dist + j, Num<T>::sqrt_(cand_d2[j * stride + tid]));
    }
    for (uint32_t j = held; j < k; ++j) {                     // the unused rest of the row: closest_points' miss record
        store_stream(row_prims + j, BVH_AMD_INVALID);
        if (row_dist) store_stream(row_dist + j, max_d);
    }
    if (a.counts) a.counts[qi] = held;
}

} // namespace

} // namespace bvh_amd
