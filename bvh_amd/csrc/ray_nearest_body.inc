// Per-lane body of the batched nearest-hits ray query (ray_nearest.hip): the first k crossings of a ray {org, dir, tmin, tmax}, front
// to back, as a row of k hit records in ascending (t, BVH-order index) order: the k smallest (t, index) among the primitives the walk
// TESTS and the unshortened ray crosses. It is the ray-side sibling of knn_body.inc: the candidate set and its LDS layout are
// knn_heap.inc's, keyed by the hit's t in place of a squared distance; the walk is nearest_walk.inc's, keyed by the t at which the ray
// enters a box — the order of the closest-hit walk of trace_body.inc, both node tests through slab_pair (trace_device.h) — and pruned
// against the worst of the k candidates held instead of the best hit; the leaf test is all-hits' (ray_prim_test.inc: tri_test.inc, the
// sphere expressions of trace_body.inc) against the ray's OWN [tmin, tmax], and the records are all-hits' (point_walk.inc: store_record). Only {t, index} is
// kept per candidate: the winners' records are rebuilt at the end by running the leaf test again (a pure function of ray and
// primitive: the same bits).
// Kept as an include so that tests/cpp/ray_nearest_body_host.cpp compiles the very same text for the host (one emulated lane per
// ray). Expects what point_walk.inc expects.
#pragma once

#include "nearest_walk.inc"
#include "knn_heap.inc"

namespace bvh_amd {

namespace {

template <typename T>
struct RayNearestArgs : PointArgs<T> {         // queries = rays, 8 scalars each
    typename HitOf<T>::Type* out_hits;         // n x k records, row-major, caller order
    uint32_t* counts;                          // optional: valid records per row (<= k)
    T* deep_t;                                 // Deep kernels only: beside deep_nodes
    uint32_t k;                                // 1 .. BVH_AMD_RAY_NEAREST_MAX_K
};

// The leaf test of the ray walks on BVH-order primitive i against the ray's own [tmin, ray_tmax]: true iff intersect's test accepts it,
// with the record's (t, u, v) — a triangle's {t, u, v}, a sphere's {t0, t1 = min(exit, ray_tmax), 0}. Nothing the walk has found
// enters it, so the walk and the write-out get the same bits from it. The two tests are ray_prim_test.inc, the text the hit lambda of
// ray_hits_lane includes as well.
template <typename T, int Leaf>
__device__ inline bool ray_nearest_test(const T* prims, uint32_t i, const T (&org)[3], const T (&dir)[3], T tmin, T ray_tmax, T& hit_t, T& hit_u, T& hit_v) {
    T tmax = ray_tmax;                                                      // this test's own copy
    bool accepted = false;
#include "ray_prim_test.inc"
    (void)tmax;
    return accepted;
}

// One ray, one lane: nearest_walk keyed by a box's entry t with `worst` as its limit: of two children the ray meets the one it enters
// first (r0 < l0 takes the right one, as trace_body.inc), the other pushed with its entry t. Both boxes are tested by slab_pair
// against [tmin, worst]: worst is the ray's tmax until k candidates are held, then the t of the largest (t, index) held. A popped
// entry is dropped iff its entry t > worst (not >=: a primitive at the same t with a lower index stays reachable, as in knn_lane).
// Every primitive the unshortened ray crosses is offered to the candidate set (knn_offer); at the end knn_sort leaves the candidates
// ascending, and the row is written: the leaf test again on each winner for its record, then
// intersect's miss record {BVH_AMD_INVALID, tmax, 0, 0} on the unused slots. Nothing is stored while walking, so a ray whose tmin or
// tmax is NaN (not walked: the `nan_ray` of slab_pair's callers) still pads its row. Slot `slot` of the launch (ray order[slot], or
// slot itself); `lane` indexes the HBM spill (Deep), `tid` and `stride` the LDS arrays. cnt += {pair records fetched, primitives
// tested (the write-out's repeats not counted), leaves visited}.
template <typename T, int Leaf, bool Robust, bool Stats, bool Deep>
__device__ inline void ray_nearest_lane(const RayNearestArgs<T>& a, unsigned long long slot, const KnnLds<T>& lds, uint32_t stride, int tid,
                                        unsigned long long lane, unsigned long long (&cnt)[3]) {
    const unsigned long long qi = a.order ? a.order[slot] : slot;
    T r[8];
    load_ray(a.queries + 8ull * qi, r);
    const T org[3] = { r[0], r[1], r[2] }, dir[3] = { r[3], r[4], r[5] };
    const T tmin = r[6], ray_tmax = r[7];
    T inv[3], aux[3];
    uint32_t oct[3];
    ray_constants<T, Robust, 3>(org, dir, inv, aux, oct);
    const bool valid = tmin == tmin && ray_tmax == ray_tmax;
    const uint32_t k = a.k;
    T* const cand_t = lds.cand_key;
    uint32_t* const cand_id = lds.cand_id;
    T worst = ray_tmax;                                       // the pruning t
    uint32_t worst_id = BVH_AMD_INVALID;                      // the index beside it, once k are held
    uint32_t held = 0;

    nearest_walk<T, kKnnLds, Stats, Deep>(a, valid, lds.stack_node, lds.stack_key, stride, tid, lane, a.deep_t, worst, cnt,
        [&](const T (&lb)[6], const T (&rb)[6], T& l0, T& r0, bool& hl, bool& hr) {
            T l1, r1;
            slab_pair<T, Robust, 3>(lb, rb, org, inv, aux, oct, tmin, worst, l0, l1, r0, r1);
            hl = l0 <= l1; hr = r0 <= r1;                     // bvh.h:177-180
        },
        [&](uint32_t i) {
            T t = T(0), u = T(0), v = T(0);
            if (ray_nearest_test<T, Leaf>(a.prims, i, org, dir, tmin, ray_tmax, t, u, v)) knn_offer(cand_t, cand_id, stride, tid, k, held, worst, worst_id, t, i, true);
        });

    knn_sort(cand_t, cand_id, stride, tid, k, held);          // ascending (t, index)
    typename HitOf<T>::Type* const row = a.out_hits + qi * k;
    for (uint32_t j = 0; j < held; ++j) {
        const uint32_t i = cand_id[j * stride + tid];
        T t = T(0), u = T(0), v = T(0);
        ray_nearest_test<T, Leaf>(a.prims, i, org, dir, tmin, ray_tmax, t, u, v);
        store_record(row + j, a.prim_ids ? a.prim_ids[i] : i, t, u, v);
    }
    for (uint32_t j = held; j < k; ++j) store_record(row + j, BVH_AMD_INVALID, ray_tmax, T(0), T(0));   // intersect's miss record
    if (a.counts) a.counts[qi] = held;
}

} // namespace

} // namespace bvh_amd
