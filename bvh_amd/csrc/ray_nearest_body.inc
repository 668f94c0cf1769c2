// Per-lane body of the batched nearest-hits ray query (ray_nearest.hip): the first k crossings of a ray {org, dir, tmin, tmax}, front
// to back, as a row of k hit records in ascending (t, BVH-order index) order: the k smallest (t, index) among the primitives the walk
// TESTS and the unshortened ray crosses. It is the ray-side twin of knn_body.inc: the candidate heap and its LDS layout are
// knn_heap.inc's, keyed by the hit's t in place of a squared distance; the walk is the closest-hit walk of trace_body.inc — near child
// first, both node tests through slab_pair (trace_device.h) — pruned against the worst of the k candidates held instead of the best
// hit; the leaf tests are the ray walks' (tri_test.inc, the sphere expressions of trace_body.inc) against the ray's OWN [tmin, tmax],
// as in ray_hits_body.inc, whose records these are. Only {t, index} is kept per candidate: the winners' records are rebuilt at the
// end by running the leaf test again (a pure function of ray and primitive: the same bits).
// Kept as an include so that tests/cpp/ray_nearest_body_host.cpp compiles the very same text for the host (one emulated lane per
// ray). Expects what point_walk.inc expects.
#pragma once

#include "ray_hits_body.inc"                   // store_record (and, through list_walk.inc, point_walk.inc)
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
// enters it, so the walk and the write-out get the same bits from it.
// TWIN COPY: the hit lambda of ray_hits_lane (ray_hits_body.inc) holds the same two tests inline; a fix to one belongs in the other.
// Having that lambda call this function instead was tried and changes the code generated for ray_hits_kernel (other register
// allocation in several variants), so the measured all-hits kernels keep their text.
template <typename T, int Leaf>
__device__ inline bool ray_nearest_test(const T* prims, uint32_t i, const T (&org)[3], const T (&dir)[3], T tmin, T ray_tmax, T& hit_t, T& hit_u, T& hit_v) {
    T tmax = ray_tmax;                                                      // this test's own copy
    bool accepted = false;
    if (Leaf == LEAF_TRIANGLE) {                                            // tri.h:56-74
        T p[12];
        load_prim12(prims + 12ull * i, p);
#define BVH_TRI_ACCEPTED accepted = true
#include "tri_test.inc"
#undef BVH_TRI_ACCEPTED
    } else {                                                                // sphere.h:32-49, as trace_body.inc writes it
        T s[4];
        load_prim4(prims + 4ull * i, s);
        const T o0 = org[0] - s[0], o1 = org[1] - s[1], o2 = org[2] - s[2];
        const T qa = dot3(dir[0], dir[1], dir[2], dir[0], dir[1], dir[2]);
        const T qb = T(2) * dot3(dir[0], dir[1], dir[2], o0, o1, o2);
        const T qc = dot3(o0, o1, o2, o0, o1, o2) - s[3] * s[3];
        const T delta = qb * qb - T(4) * qa * qc;
        if (delta >= 0) {
            const T iv = -T(0.5) / qa;
            const T root = Num<T>::sqrt_(delta);
            const T t0 = pick_max((qb + root) * iv, tmin);
            const T t1 = pick_min((qb - root) * iv, tmax);
            if (t0 <= t1) { hit_t = t0; hit_u = t1; hit_v = T(0); accepted = true; }
        }
    }
    (void)tmax;
    return accepted;
}

// One ray, one lane: depth-first, of two children the ray meets the one it enters first (l0 > r0 takes the right one, as
// trace_body.inc), the other pushed with its entry t. Both boxes are tested by slab_pair against [tmin, worst]: worst is the ray's
// tmax until k candidates are held, then the t of the largest (t, index) held. A popped entry is dropped iff its entry t > worst (not
// >=: a primitive at the same t with a lower index stays reachable, as in knn_lane). Inside a leaf the index ascends; a primitive the
// unshortened ray crosses is accepted while fewer than k are held, afterwards iff (t, index) is below the largest held, which it
// replaces. The candidates are appended unordered until the k-th makes them a max-heap; a replacement is one sift-down; at the end an
// in-place heapsort leaves them ascending, and the row is written: the leaf test again on each winner for its record, then
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
    T* const cand_t = lds.cand_d2;
    uint32_t* const cand_id = lds.cand_id;
    T worst = ray_tmax;                                       // the pruning t
    uint32_t worst_id = BVH_AMD_INVALID;                      // the index beside it, once k are held
    uint32_t held = 0;

    uint32_t spill_node[kPointSmall - kKnnLds];
    T spill_t[kPointSmall - kKnnLds];
    uint32_t sp = 0;
    auto push = [&](uint32_t node, T t) {
        if (sp < kKnnLds) { lds.stack_node[sp * stride + tid] = node; lds.stack_d2[sp * stride + tid] = t; }
        else if (!Deep || sp < kPointSmall) { const uint32_t i = stack_small_at<kKnnLds>(sp); spill_node[i] = node; spill_t[i] = t; }
        else { const unsigned long long i = stack_deep_at(a, lane, sp); a.deep_nodes[i] = node; a.deep_t[i] = t; }
        ++sp;
    };
    // the next stacked entry the ray still reaches in front of the worst candidate (false: the walk is over)
    auto pop = [&](uint32_t& node) -> bool {
        while (sp > 0) {
            --sp;
            uint32_t e;
            T t;
            if (sp < kKnnLds) { e = lds.stack_node[sp * stride + tid]; t = lds.stack_d2[sp * stride + tid]; }
            else if (!Deep || sp < kPointSmall) { const uint32_t i = stack_small_at<kKnnLds>(sp); e = spill_node[i]; t = spill_t[i]; }
            else { const unsigned long long i = stack_deep_at(a, lane, sp); e = a.deep_nodes[i]; t = a.deep_t[i]; }
            if (!(t > worst)) { node = e; return true; }
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
            T l0, l1, r0, r1;
            slab_pair<T, Robust, 3>(lb, rb, org, inv, aux, oct, tmin, worst, l0, l1, r0, r1);
            const bool hl = l0 <= l1, hr = r0 <= r1;          // bvh.h:177-180
            if (hl && hr) {
                if (l0 > r0) { push(li, l0); node = ri; }
                else { push(ri, r0); node = li; }
            } else if (hl) node = li;
            else if (hr) node = ri;
            else if (!pop(node)) { live = false; break; }
        }
        if (!live) break;
        const uint32_t first = node >> kCountBits, count = node & kCountMask;
        if (Stats) ++cnt[2];
        for (uint32_t i = first; i < first + count; ++i) {
            if (Stats) ++cnt[1];
            T t = T(0), u = T(0), v = T(0);
            if (!ray_nearest_test<T, Leaf>(a.prims, i, org, dir, tmin, ray_tmax, t, u, v)) continue;
            if (held < k) {
                cand_t[held * stride + tid] = t;
                cand_id[held * stride + tid] = i;
                if (++held == k) {
                    knn_make_heap(cand_t, cand_id, stride, tid, k);
                    worst = cand_t[tid]; worst_id = cand_id[tid];
                }
            } else if (knn_less(t, i, worst, worst_id)) {
                knn_sift_down(cand_t, cand_id, stride, tid, 0u, k, t, i);
                worst = cand_t[tid]; worst_id = cand_id[tid];
            }
        }
        live = pop(node);
    }

    // ascending (t, index): heapsort in place
    if (held < k) knn_make_heap(cand_t, cand_id, stride, tid, held);
    for (uint32_t m = held; m-- > 1;) {
        const T lt = cand_t[m * stride + tid], tt = cand_t[tid];
        const uint32_t li = cand_id[m * stride + tid], ti = cand_id[tid];
        cand_t[m * stride + tid] = tt; cand_id[m * stride + tid] = ti;
        knn_sift_down(cand_t, cand_id, stride, tid, 0u, m, lt, li);
    }
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
