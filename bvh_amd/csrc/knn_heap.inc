// The candidate set of the k-smallest queries (knn_body.inc: points, keyed by squared distance; ray_nearest_body.inc: rays, keyed by
// hit t): a lane's k {key, index} candidates and the first kKnnLds entries of its stack in the block's dynamic LDS, the binary
// max-heap on (key, index) pairs kept there, and the two operations the lanes use: knn_offer while walking (nearest_walk.inc), knn_sort
// before the row is written. Kept as an include so that the host harnesses (tests/cpp/knn_body_host.cpp, ray_nearest_body_host.cpp)
// compile the very same text, through the bodies. Expects what point_walk.inc expects.
#pragma once

namespace bvh_amd {

namespace {

// Stack entries of a lane held in LDS beside its candidates ({node word, key}, as closest_lane), the rest in scratch and HBM
// (point_walk.inc has the tiers).
constexpr int kKnnLds = 8;

// The block's LDS, `stride` lanes wide: candidate key [k][stride], stack key [kKnnLds][stride], candidate index [k][stride], stack node
// word [kKnnLds][stride] (the scalars first: doubles stay 8-byte aligned). Slot s of lane tid sits at s * stride + tid of its array:
// the bank is the lane's whatever the slot, so lanes at different heap positions do not conflict.
template <typename T>
struct KnnLds {
    T* cand_key;
    T* stack_key;
    uint32_t* cand_id;
    uint32_t* stack_node;
};
template <typename T>
__host__ __device__ inline size_t knn_lds_bytes(uint32_t k, uint32_t stride) { return size_t(k + kKnnLds) * stride * (sizeof(T) + sizeof(uint32_t)); }
template <typename T>
__host__ __device__ inline KnnLds<T> knn_lds_carve(void* base, uint32_t k, uint32_t stride) {
    KnnLds<T> l;
    l.cand_key = static_cast<T*>(base);
    l.stack_key = l.cand_key + size_t(k) * stride;
    l.cand_id = reinterpret_cast<uint32_t*>(l.stack_key + size_t(kKnnLds) * stride);
    l.stack_node = l.cand_id + size_t(k) * stride;
    return l;
}

// (key, index) pairs in lexicographic order
template <typename T>
__device__ inline bool knn_less(T da, uint32_t ia, T db, uint32_t ib) { return da < db || (da == db && ia < ib); }

// Max-heap on (key, index) in the lane's first m candidate slots: the pair (vd, vi) sinks from slot `hole` (whose content is dead) to
// its place, at most log2 m steps.
template <typename T>
__device__ inline void knn_sift_down(T* cand_key, uint32_t* cand_id, uint32_t stride, int tid, uint32_t hole, uint32_t m, T vd, uint32_t vi) {
    for (;;) {
        uint32_t c = 2 * hole + 1;
        if (c >= m) break;
        T cd = cand_key[c * stride + tid];
        uint32_t ci = cand_id[c * stride + tid];
        if (c + 1 < m) {
            const T rd = cand_key[(c + 1) * stride + tid];
            const uint32_t ri = cand_id[(c + 1) * stride + tid];
            if (knn_less(cd, ci, rd, ri)) { cd = rd; ci = ri; ++c; }
        }
        if (!knn_less(vd, vi, cd, ci)) break;
        cand_key[hole * stride + tid] = cd;
        cand_id[hole * stride + tid] = ci;
        hole = c;
    }
    cand_key[hole * stride + tid] = vd;
    cand_id[hole * stride + tid] = vi;
}

template <typename T>
__device__ inline void knn_make_heap(T* cand_key, uint32_t* cand_id, uint32_t stride, int tid, uint32_t m) {
    for (uint32_t h = m / 2; h-- > 0;) knn_sift_down(cand_key, cand_id, stride, tid, h, m, cand_key[h * stride + tid], cand_id[h * stride + tid]);
}

// Primitive i with its key, offered to a lane's candidates: appended unordered while fewer than k are held (the k-th makes them a
// max-heap) iff `filling` - the caller's admission rule for that phase alone (knn: within max_distance; rays: true) -, afterwards it
// replaces the largest (key, index) held iff it is below it, by one sift-down. `worst` / `worst_id` are that largest pair once k are
// held (the walk prunes against `worst`; a rejected primitive costs one comparison and no LDS access) and are left alone before:
// `worst` is then still the caller's starting limit.
// (`filling` is an argument and not an `if` around the call: `held == k || rule` at the call site, however it is spelt, compiles to
//  a test of its own in front of this function's, five more instructions per primitive tested in knn_kernel.)
template <typename T>
__device__ inline void knn_offer(T* cand_key, uint32_t* cand_id, uint32_t stride, int tid, uint32_t k, uint32_t& held, T& worst, uint32_t& worst_id,
                                 T key, uint32_t i, bool filling) {
    if (held < k) {
        if (filling) {
            cand_key[held * stride + tid] = key;
            cand_id[held * stride + tid] = i;
            if (++held == k) {
                knn_make_heap(cand_key, cand_id, stride, tid, k);
                worst = cand_key[tid]; worst_id = cand_id[tid];
            }
        }
    } else if (knn_less(key, i, worst, worst_id)) {
        knn_sift_down(cand_key, cand_id, stride, tid, 0u, k, key, i);
        worst = cand_key[tid]; worst_id = cand_id[tid];
    }
}

// The `held` candidates of a lane in ascending (key, index) order: heapsort in place (fewer than k were never made a heap).
template <typename T>
__device__ inline void knn_sort(T* cand_key, uint32_t* cand_id, uint32_t stride, int tid, uint32_t k, uint32_t held) {
    if (held < k) knn_make_heap(cand_key, cand_id, stride, tid, held);
    for (uint32_t m = held; m-- > 1;) {
        const T lk = cand_key[m * stride + tid], tk = cand_key[tid];
        const uint32_t li = cand_id[m * stride + tid], ti = cand_id[tid];
        cand_key[m * stride + tid] = tk; cand_id[m * stride + tid] = ti;
        knn_sift_down(cand_key, cand_id, stride, tid, 0u, m, lk, li);
    }
}

} // namespace

} // namespace bvh_amd
