// TEST INFRASTRUCTURE (CPU, no GPU): compiles the text of the triangle-distance kernel — bvh_amd/csrc/tri_distance_body.inc (over
// nearest_walk.inc, the pair test of tri_intersect_body.inc and point_walk.inc) with the device helpers of bvh_amd/csrc/trace_device.h
// — for the HOST and runs it with one emulated lane per query (the queries of a batch one after another, or split over host threads).
// What it can show: the pair distance of the very source the device runs is the distance of two triangles (against a float64
// restatement in the tests) and 0 exactly where the pair test intersects; the walk returns what a brute force over the same function
// returns; the device's records, query barycentrics and counters must equal these bit for bit. What it cannot show: anything that
// needs the hardware. tests/test_tri_distance_host.py drives it; tests/test_gpu_tri_distance.py uses it too.
//
// Built by the tests with: g++ -std=c++20 -O1 -mavx2 -mfma -ffp-contract=off -fno-strict-aliasing -shared -fPIC -pthread.
#include "host_lane_prelude.h"
#include "../../bvh_amd/csrc/tri_distance_body.inc"

namespace {

using namespace bvh_amd;

template <typename T>
TriDistanceArgs<T> make_args(const void* pairs, uint32_t root_index, const void* tris9, const uint32_t* tri_ids, const void* queries, size_t n, double max_distance,
                             const void* max_distances, const uint32_t* order, int original_ids, uint32_t deep_cap, void* hits, void* query_uv) {
    TriDistanceArgs<T> a{};
    a.pairs = static_cast<const PairNode<T>*>(pairs); a.prims = static_cast<const T*>(tris9); a.queries = static_cast<const T*>(queries);
    a.hits = static_cast<typename HitOf<T>::Type*>(hits); a.tri_ids = tri_ids;
    a.max_distances = static_cast<const T*>(max_distances); a.max_distance = static_cast<T>(max_distance); a.query_uv = static_cast<T*>(query_uv);
    a.n = n; a.first = 0; a.order = order; a.prim_ids = original_ids ? tri_ids : nullptr; a.counters = nullptr;
    a.deep_cap = deep_cap; a.root_index = root_index;
    return a;
}

template <typename T, bool Deep>
void walk_range(const TriDistanceArgs<T>& a0, unsigned long long begin, unsigned long long end, unsigned long long (&cnt)[3]) {
    TriDistanceArgs<T> a = a0;
    std::vector<uint32_t> lds_node(size_t(kClosestLds) * kBlock);
    std::vector<T> lds_d2(size_t(kClosestLds) * kBlock);
    std::vector<uint32_t> deep_nodes(Deep ? a.deep_cap : 1);
    std::vector<T> deep_d2(Deep ? a.deep_cap : 1);
    a.deep_nodes = deep_nodes.data(); a.deep_d2 = deep_d2.data();            // one lane at a time: lane 0's spill
    for (unsigned long long s = begin; s < end; ++s) tri_distance_lane<T, true, Deep>(a, s, lds_node.data(), lds_d2.data(), int(s % kBlock), 0, cnt);
}

template <typename T>
int walk(const void* pairs, uint32_t root_index, const void* tris9, const uint32_t* tri_ids, const void* queries, size_t n, double max_distance,
         const void* max_distances, const uint32_t* order, int original_ids, uint32_t deep_cap, int threads, void* hits, void* query_uv,
         unsigned long long* counters3) {
    const TriDistanceArgs<T> a = make_args<T>(pairs, root_index, tris9, tri_ids, queries, n, max_distance, max_distances, order, original_ids, deep_cap, hits, query_uv);
    run_lanes(n, threads, counters3, [&](unsigned long long b, unsigned long long e, unsigned long long (&cnt)[3]) {
        if (deep_cap) walk_range<T, true>(a, b, e, cnt); else walk_range<T, false>(a, b, e, cnt);
    });
    return 0;
}

// every query against every BVH-order triangle through the same pair distance and the walk's update rule: argmin by (d2, index),
// without the walk's box rejection. best2 (optional): the smallest squared distance of a triangle OTHER than the record's.
template <typename T>
void brute(const T* tris9, const uint32_t* tri_ids, size_t n_prims, const T* queries, size_t n, double max_distance, const T* max_distances,
           typename HitOf<T>::Type* hits, T* query_uv, T* runner_up, int threads) {
    const int nt = std::max(1, threads);
    std::vector<std::thread> pool;
    for (int th = 0; th < nt; ++th) {
        pool.emplace_back([=] {
            for (size_t k = n * th / nt; k < n * (th + 1) / nt; ++k) {
                TdQuery<T> q;
                td_query(queries + 9 * k, q);
                const T max_d = max_distances ? max_distances[k] : static_cast<T>(max_distance);
                bool valid = max_d >= T(0);
                for (int c = 0; c < 9; ++c) valid = valid && q.raw[c] == q.raw[c];
                T best = max_d * max_d, second = Num<T>::kMax, bu = T(0), bv = T(0), bs = T(0), bw = T(0);
                uint32_t bi = BVH_AMD_INVALID;
                for (size_t i = 0; valid && i < n_prims; ++i) {
                    T b[9], u, v, s, w;
                    load_tri9(tris9 + 9ull * tri_ids[i], b);
                    const T d2 = tri_tri_dist2(q, b, u, v, s, w);
                    if (d2 < best || (d2 == best && i < bi)) {
                        if (bi != BVH_AMD_INVALID && best < second) second = best;
                        best = d2; bi = uint32_t(i); bu = u; bv = v; bs = s; bw = w;
                    } else if (d2 < second) second = d2;
                }
                if (bi != BVH_AMD_INVALID) store_hit(hits + k, bi, Num<T>::sqrt_(best), bu, bv);
                else store_hit(hits + k, BVH_AMD_INVALID, max_d, T(0), T(0));
                if (query_uv) { query_uv[2 * k] = bs; query_uv[2 * k + 1] = bw; }
                if (runner_up) runner_up[k] = second;
            }
        });
    }
    for (auto& th : pool) th.join();
}

// one pair: out6 = {d2, u, v, s, w, 1 / 0: the pair test accepts it}
template <typename T>
void one(const T* query9, const T* tri9, T* out6) {
    TdQuery<T> q;
    td_query(query9, q);
    T b[9], u, v, s, w;
    load_tri9(tri9, b);
    out6[0] = tri_tri_dist2(q, b, u, v, s, w);
    out6[1] = u; out6[2] = v; out6[3] = s; out6[4] = w;
    out6[5] = q.usable && tri_pair_intersects(q.raw, q.lo, q.hi, q.n, b, false) ? T(1) : T(0);
}

} // namespace

extern "C" {

// The pair distance of n (query triangle, tree triangle) pairs, row k of each array (9 scalars per row):
// out6[k] = {squared distance, (u, v) on the tree triangle, (s, w) on the query triangle, 1 / 0: tri_pair_intersects accepts the pair}.
void tri_distance_host_pairs(int is_double, const void* queries9, const void* tris9, size_t n, void* out6) {
    for (size_t k = 0; k < n; ++k) {
        if (is_double) one<double>(static_cast<const double*>(queries9) + 9 * k, static_cast<const double*>(tris9) + 9 * k, static_cast<double*>(out6) + 6 * k);
        else one<float>(static_cast<const float*>(queries9) + 9 * k, static_cast<const float*>(tris9) + 9 * k, static_cast<float*>(out6) + 6 * k);
    }
}

// The kernel's walk for n query triangles of 9 scalars (slot s reads query order[s], or s) with max_distances[q] (or `max_distance`
// when max_distances is NULL). tris9: triangles by original id, tri_ids: BVH-order index -> original id; original_ids != 0 =
// BVH_AMD_RAY_ORIGINAL_IDS; deep_cap > 0: the HBM spill of trees deeper than 64 levels, deep_cap entries. hits: bvh_hit3f / bvh_hit3d
// records; query_uv (optional): 2 scalars per query; counters3 = {pairs fetched, triangles fetched, leaves visited}. Returns 0.
int tri_distance_host_walk(int is_double, const void* pairs, uint32_t root_index, const void* tris9, const uint32_t* tri_ids, const void* queries, size_t n,
                           double max_distance, const void* max_distances, const uint32_t* order, int original_ids, uint32_t deep_cap, int threads, void* hits,
                           void* query_uv, unsigned long long* counters3) {
    if (is_double) return walk<double>(pairs, root_index, tris9, tri_ids, queries, n, max_distance, max_distances, order, original_ids, deep_cap, threads, hits, query_uv, counters3);
    return walk<float>(pairs, root_index, tris9, tri_ids, queries, n, max_distance, max_distances, order, original_ids, deep_cap, threads, hits, query_uv, counters3);
}

// Brute force over all n_prims BVH-order triangles with the kernel's pair distance and update rule: one record per query (BVH-order
// prim), its query barycentrics (optional) and the smallest SQUARED distance among the other triangles (optional; kMax if none).
void tri_distance_host_brute(int is_double, const void* tris9, const uint32_t* tri_ids, size_t n_prims, const void* queries, size_t n, double max_distance,
                             const void* max_distances, void* hits, void* query_uv, void* runner_up, int threads) {
    if (is_double) brute<double>(static_cast<const double*>(tris9), tri_ids, n_prims, static_cast<const double*>(queries), n, max_distance,
                                 static_cast<const double*>(max_distances), static_cast<bvh_hit3d*>(hits), static_cast<double*>(query_uv),
                                 static_cast<double*>(runner_up), threads);
    else brute<float>(static_cast<const float*>(tris9), tri_ids, n_prims, static_cast<const float*>(queries), n, max_distance,
                      static_cast<const float*>(max_distances), static_cast<bvh_hit3f*>(hits), static_cast<float*>(query_uv),
                      static_cast<float*>(runner_up), threads);
}

} // extern "C"
