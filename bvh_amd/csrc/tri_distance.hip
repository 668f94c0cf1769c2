// Batched triangle-distance queries for gfx950: for every query triangle {p0, p1, p2} (or segment, or point: a degenerate triangle)
// and a max_distance (one for the batch or one per query), the nearest triangle of the tree, the distance, and where the two come
// closest, as one hit record {prim, t, u, v} and, optionally, the barycentrics of the closest point on the query triangle. The
// primitives' triangles are the caller's array indexed by original primitive id, the one bvh3X_intersect_tris and bvh3X_refit_tris
// take, read through the tree's prim ids. The per-lane walk and the pair distance are tri_distance_body.inc (shared with the host
// test harness, tests/cpp/tri_distance_body_host.cpp) over nearest_walk.inc and the sign-only pair test of tri_pair.inc,
// which decides distance 0; the launch path is point_query.h's; this file holds the kernel and what is specific to the query.
//
// MI355X mapping (closest.hip's, with a box / box key and a triangle pair behind the primitive's box test):
//   * one lane per query, one-shot grid of ceil(n / 256) blocks: no ticket counter, so no work slot of the tree is claimed and any
//     number of launches of one const tree may run at once;
//   * a lane holds its query for the whole walk: nine coordinates, their box, the normal, and the query's half of the pair
//     distance (its face's 2 x 2 system and the reciprocals of its squared edge lengths), computed once;
//   * depth-first walk over the 64 / 128-byte pair records, the child whose box is nearer to the query's box first, the other stacked
//     with its key so that a popped entry is re-checked against the best distance before anything is fetched;
//   * the stack: kClosestLds entries in LDS ([depth][lane]), the rest of 64 in per-lane scratch, beyond 64 (deep trees) in HBM.
//     kClosestLds is closest-point's measured choice; no other depth was measured for this kernel;
//   * a leaf's primitives one at a time: prim id, then the 36 / 72 bytes of its triangle; its box's key against the best distance
//     (where most leave), the pair test, then 9 edge pairs and 6 edge / face candidates. The candidates are loops that rotate the
//     vertices through registers and selects on the loop counter, one instruction stream for every lane whatever its pair looks like;
//   * query triangles are optionally read in the order of the Hilbert cell of their box's centre in the root box (query_order.h,
//     tri_intersect's key). Records are always written in the caller's order.
//
// Compiled with -ffp-contract=off; division and sqrt are the correctly rounded forms (bit-identical to the host harness).

#include "common.h"
#include "trace_device.h"
#include "ray_key.h"
#include "query_order.h"
#include "tri_distance_body.inc"
#include "point_query.h"

namespace bvh_amd {

namespace {

template <typename T, bool Stats, bool Deep>
__global__ void __launch_bounds__(kBlock) tri_distance_kernel(TriDistanceArgs<T> a) {
    __shared__ uint32_t lds_node[kClosestLds * kBlock];
    __shared__ T lds_d2[kClosestLds * kBlock];
    const int tid = threadIdx.x;
    const unsigned long long lane = static_cast<unsigned long long>(blockIdx.x) * kBlock + tid;
    unsigned long long cnt[3] = {0, 0, 0};
    if (lane < a.n) tri_distance_lane<T, Stats, Deep>(a, a.first + lane, lds_node, lds_d2, tid, lane, cnt);
    if (Stats) add_counters(a.counters, cnt, tid);
}

} // namespace

template <typename T>
int launch_tri_distance(const BvhImpl<T>& b, const T* d_tris9, size_t n_tris, const T* d_queries9, size_t n, T max_distance, const T* d_max_distances,
                        unsigned flags, typename HitOf<T>::Type* d_hits, T* d_query_uv, bvh_amd_counters* d_counters, hipStream_t stream) {
    const char* who = "tri_distance";
    const bool aligned = !(misaligned(d_tris9, sizeof(T)) || misaligned(d_queries9, sizeof(T)) || misaligned(d_max_distances, sizeof(T)) ||
                           misaligned(d_query_uv, sizeof(T)) || misaligned(d_hits, 16) || misaligned(d_counters, 8));
    if (const int rc = point_query_check(b, n, flags, d_tris9 && d_queries9 && d_hits,
                                         aligned ? nullptr : "device pointers must be aligned (triangles, queries, max distances and query barycentrics to their scalar, hit records 16 bytes, counters 8)",
                                         who);
        rc || n == 0)
        return rc;
    if (const int rc = source_array_check(b, n_tris, "triangles", who, stream)) return rc;
    // (kPointSortMin: the threshold measured for closest-point queries; not measured for this kind. tools/bench_tri_distance.py times
    //  SORTED against UNSORTED.)
    return point_query_run<T, kQueryTris>(b, d_tris9, d_queries9, n, flags, d_counters, sizeof(uint32_t) + sizeof(T), kBlock, kPointSortMin, kPointKeyBits, who,
                                          stream, [&](const PointArgs<T>& args, T* deep_d2) {
        const TriDistanceArgs<T> a{args, d_hits, deep_d2, b.d_prim_ids, d_max_distances, max_distance, d_query_uv};
        // (the ladder's leaf kind is unused here: a triangle is a triangle)
        return point_query_dispatch(LEAF_TRIANGLE, d_counters != nullptr, a.deep_cap != 0, [&](auto, auto stats, auto deep) {
            return point_query_launch(tri_distance_kernel<T, stats(), deep()>, a, kBlock, 0, stream);
        });
    });
}

template int launch_tri_distance<float>(const BvhImpl<float>&, const float*, size_t, const float*, size_t, float, const float*, unsigned, bvh_hit3f*, float*,
                                        bvh_amd_counters*, hipStream_t);
template int launch_tri_distance<double>(const BvhImpl<double>&, const double*, size_t, const double*, size_t, double, const double*, unsigned, bvh_hit3d*,
                                         double*, bvh_amd_counters*, hipStream_t);

} // namespace bvh_amd
