// The candidate set of the k-smallest queries (knn_body.inc: points, keyed by squared distance; ray_nearest_body.inc: rays, keyed by
// hit t): a lane's k {scalar, index} candidates and the first kKnnLds entries of its stack in the block's dynamic LDS, and the binary
// max-heap on (scalar, index) pairs the walks keep there. The array names say d2 because the point query came first; the ray query
// stores t in the same slots. Kept as an include so that the host harnesses (tests/cpp/knn_body_host.cpp, ray_nearest_body_host.cpp)
// compile the very same text, through the bodies. Expects what point_walk.inc expects.
#pragma once

namespace bvh_amd {

namespace {

// Stack entries of a lane held in LDS beside its candidates ({node word, box distance^2}, as closest_lane), the rest in scratch and
// HBM (point_walk.inc has the tiers).
constexpr int kKnnLds = 8;

// The block's LDS, `stride` lanes wide: candidate d2 [k][stride], stack d2 [kKnnLds][stride], candidate index [k][stride], stack node
// word [kKnnLds][stride] (the scalars first: doubles stay 8-byte aligned). Slot s of lane tid sits at s * stride + tid of its array:
// the bank is the lane's whatever the slot, so lanes at different heap positions do not conflict.
template <typename T>
struct KnnLds {
    T* cand_d2;
    T* stack_d2;
    uint32_t* cand_id;
    uint32_t* stack_node;
};
template <typename T>
__host__ __device__ inline size_t knn_lds_bytes(uint32_t k, uint32_t stride) { return size_t(k + kKnnLds) * stride * (sizeof(T) + sizeof(uint32_t)); }
template <typename T>
__host__ __device__ inline KnnLds<T> knn_lds_carve(void* base, uint32_t k, uint32_t stride) {
    KnnLds<T> l;
    l.cand_d2 = static_cast<T*>(base);
    l.stack_d2 = l.cand_d2 + size_t(k) * stride;
    l.cand_id = reinterpret_cast<uint32_t*>(l.stack_d2 + size_t(kKnnLds) * stride);
    l.stack_node = l.cand_id + size_t(k) * stride;
    return l;
}

// (d2, index) pairs in lexicographic order
template <typename T>
__device__ inline bool knn_less(T da, uint32_t ia, T db, uint32_t ib) { return da < db || (da == db && ia < ib); }

// Max-heap on (d2, index) in the lane's first m candidate slots: the pair (vd, vi) sinks from slot `hole` (whose content is dead) to
// its place, at most log2 m steps.
template <typename T>
__device__ inline void knn_sift_down(T* cand_d2, uint32_t* cand_id, uint32_t stride, int tid, uint32_t hole, uint32_t m, T vd, uint32_t vi) {
    for (;;) {
        uint32_t c = 2 * hole + 1;
        if (c >= m) break;
        T cd = cand_d2[c * stride + tid];
        uint32_t ci = cand_id[c * stride + tid];
        if (c + 1 < m) {
            const T rd = cand_d2[(c + 1) * stride + tid];
            const uint32_t ri = cand_id[(c + 1) * stride + tid];
            if (knn_less(cd, ci, rd, ri)) { cd = rd; ci = ri; ++c; }
        }
        if (!knn_less(vd, vi, cd, ci)) break;
        cand_d2[hole * stride + tid] = cd;
        cand_id[hole * stride + tid] = ci;
        hole = c;
    }
    cand_d2[hole * stride + tid] = vd;
    cand_id[hole * stride + tid] = vi;
}

template <typename T>
__device__ inline void knn_make_heap(T* cand_d2, uint32_t* cand_id, uint32_t stride, int tid, uint32_t m) {
    for (uint32_t h = m / 2; h-- > 0;) knn_sift_down(cand_d2, cand_id, stride, tid, h, m, cand_d2[h * stride + tid], cand_id[h * stride + tid]);
}

} // namespace

} // namespace bvh_amd
