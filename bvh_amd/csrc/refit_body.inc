// Body of the primitive-driven refit (refit_prims.hip: bvhXX_refit_boxes / bvh3X_refit_tris): the per-leaf fold over the leaf's
// primitives, the store of a node's box into its half of the traversal record, and the bottom-up climb over arrival tickets.
// Compiles for the device and, with single-lane stand-ins, for the host (tests/cpp/refit_body_host.cpp), so that a CPU test runs
// this very text. The includer provides HostNode<T>, PairNode<T>, kCountBits / kCountMask, the REFIT_* source kinds (common.h) and three hooks:
//   BVH_REFIT_LOAD(ptr)        a box component another climber may have written (device: agent-scope relaxed atomic load)
//   BVH_REFIT_STORE(ptr, v)    a box component another climber may read        (device: agent-scope relaxed atomic store)
//   BVH_REFIT_ARRIVE(counter)  this lane's accesses complete, then the arrival ticket: returns the count before it
#pragma once

namespace bvh_amd {

// robust_min / robust_max (utils.h:41-43) with the ACCUMULATED value first, as BBox::extend passes them (bbox.h:23-27): the order
// and the direction of the comparison decide which of +0 / -0 survives a tie and what a NaN does.
template <typename T> __device__ inline T refit_min(T acc, T other) { return acc < other ? acc : other; }
template <typename T> __device__ inline T refit_max(T acc, T other) { return acc > other ? acc : other; }

template <typename T> struct RefitLimits;
template <> struct RefitLimits<float>  { static constexpr float  kMax = 3.402823466e+38f; };
template <> struct RefitLimits<double> { static constexpr double kMax = 1.7976931348623157e+308; };

template <typename T, int Src>
__device__ inline void refit_prim_box(const T* src, size_t j, T (&lo)[3], T (&hi)[3]) {
    if constexpr (Src == REFIT_BOXES3) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { lo[k] = src[6 * j + k]; hi[k] = src[6 * j + 3 + k]; }
    } else if constexpr (Src == REFIT_BOXES2) {
#pragma unroll
        for (int k = 0; k < 2; ++k) { lo[k] = src[4 * j + k]; hi[k] = src[4 * j + 2 + k]; }
        lo[2] = hi[2] = T(0);
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) {                         // BBox(p0).extend(p1).extend(p2): what bvh_amd_tri_bounds3X writes
            T l = src[9 * j + k], h = l;
            l = refit_min(l, src[9 * j + 3 + k]); h = refit_max(h, src[9 * j + 3 + k]);
            l = refit_min(l, src[9 * j + 6 + k]); h = refit_max(h, src[9 * j + 6 + k]);
            lo[k] = l; hi[k] = h;
        }
    }
}

// box = BBox::make_empty() (bbox.h:40-44), then extend(bboxes[prim_ids[i]]) for i in [first, first + count), in this order.
// Node layout out: {min.x, max.x, min.y, max.y, min.z, max.z}; a 2D tree keeps z = (+0, +0).
// Slots beyond prim_total and ids beyond n_src are skipped (the host refuses such calls; nothing is ever read out of bounds).
template <typename T, int Src>
__device__ inline void refit_fold_leaf(const T* src, size_t n_src, const uint32_t* prim_ids, size_t prim_total, size_t first, uint32_t count,
                                       T (&box)[6]) {
    constexpr int D = Src == REFIT_BOXES2 ? 2 : 3;
    T lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { lo[k] = RefitLimits<T>::kMax; hi[k] = -RefitLimits<T>::kMax; }
    for (uint32_t s = 0; s < count; ++s) {
        const size_t slot = first + s;
        if (slot >= prim_total) break;
        const size_t j = prim_ids[slot];
        if (j >= n_src) continue;
        T plo[3], phi[3];
        refit_prim_box<T, Src>(src, j, plo, phi);
#pragma unroll
        for (int k = 0; k < D; ++k) { lo[k] = refit_min(lo[k], plo[k]); hi[k] = refit_max(hi[k], phi[k]); }
    }
    if constexpr (D == 2) { lo[2] = T(0); hi[2] = T(0); }
#pragma unroll
    for (int k = 0; k < 3; ++k) { box[2 * k] = lo[k]; box[2 * k + 1] = hi[k]; }
}

// Node c > 0 is the left (odd c) or right half of traversal record (c - 1) / 2; the record's index words are never touched.
// Plain stores: the records are read by later kernels only.
template <typename T>
__device__ inline void refit_store_half(PairNode<T>* pairs, size_t c, const T (&box)[6]) {
    if (c == 0) return;                                       // the root is in no record
    PairNode<T>& rec = pairs[(c - 1) / 2];
    T* half = (c & 1) ? rec.lb : rec.rb;
#pragma unroll
    for (int k = 0; k < 6; ++k) half[k] = box[k];
}

// The box of a node goes to both representations; the reference-layout copy is what the climb exchanges between lanes.
template <typename T>
__device__ inline void refit_store_node(HostNode<T>* nodes, PairNode<T>* pairs, size_t c, const T (&box)[6]) {
#pragma unroll
    for (int k = 0; k < 6; ++k) BVH_REFIT_STORE(&nodes[c].bounds[k], box[k]);
    refit_store_half<T>(pairs, c, box);
}

// Bvh::refit's inner step (bvh.h:211-218): every inner box = left.get_bbox().extend(right.get_bbox()), children before parents.
// The lane of leaf `i` (its box already stored) climbs; the second child to arrive at a node computes it. parent[] holds
// 0xFFFFFFFF for a node no inner node references (the root, and the top of an unused subtree: the climb ends there).
template <typename T>
__device__ inline void refit_climb(HostNode<T>* nodes, PairNode<T>* pairs, const uint32_t* parent, uint32_t* arrived, uint32_t n, uint32_t i) {
    uint32_t cur = parent[i];
    while (cur != 0xFFFFFFFFu) {
        if (BVH_REFIT_ARRIVE(&arrived[cur]) == 0) return;     // first child: the sibling's lane finishes this node
        const size_t f = static_cast<size_t>(nodes[cur].index >> kCountBits);
        if (f + 1 >= n) return;                               // (never in a validated tree)
        const T* l = nodes[f].bounds;
        const T* r = nodes[f + 1].bounds;
        T box[6];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const T lo_l = BVH_REFIT_LOAD(&l[2 * q]), lo_r = BVH_REFIT_LOAD(&r[2 * q]);
            const T hi_l = BVH_REFIT_LOAD(&l[2 * q + 1]), hi_r = BVH_REFIT_LOAD(&r[2 * q + 1]);
            box[2 * q] = refit_min(lo_l, lo_r);
            box[2 * q + 1] = refit_max(hi_l, hi_r);
        }
        refit_store_node<T>(nodes, pairs, cur, box);
        cur = parent[cur];
    }
}

// One lane per node of the array: leaves (reachable or not, like the reference's traverse_bottom_up) fold and climb.
template <typename T, int Src>
__device__ inline void refit_lane(HostNode<T>* nodes, PairNode<T>* pairs, const uint32_t* parent, uint32_t* arrived, uint32_t n, const T* src, size_t n_src,
                                  const uint32_t* prim_ids, size_t prim_total, uint32_t i) {
    const auto index = nodes[i].index;
    const uint32_t count = static_cast<uint32_t>(index & kCountMask);
    if (count == 0) return;
    T box[6];
    refit_fold_leaf<T, Src>(src, n_src, prim_ids, prim_total, static_cast<size_t>(index >> kCountBits), count, box);
    refit_store_node<T>(nodes, pairs, i, box);
    refit_climb<T>(nodes, pairs, parent, arrived, n, i);
}

} // namespace bvh_amd
