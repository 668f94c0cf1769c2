// TEST INFRASTRUCTURE (CPU, no GPU): compiles the text of the closest-point kernel — bvh_amd/csrc/closest_body.inc with the device
// helpers of bvh_amd/csrc/trace_device.h — for the HOST and runs it with one emulated lane per query (the queries of a batch one after
// another, or split over host threads). What it can show: the distance functions and the walk of the very source the device runs give
// the nearest primitive, and the device's records must equal these bit for bit. What it cannot show: anything that needs the hardware.
// tests/test_closest_point_host.py drives it; tests/test_gpu_closest_point.py and tools/closest_point_bench.py (CPU baseline) use it too.
//
// Built by the tests with: g++ -std=c++20 -O1 -mavx2 -mfma -ffp-contract=off -fno-strict-aliasing -shared -fPIC -pthread.
#include "host_lane_prelude.h"
#include "../../bvh_amd/csrc/closest_body.inc"

namespace {

using namespace bvh_amd;

template <typename T, int Leaf, bool Deep>
void walk_range(const ClosestArgs<T>& a0, unsigned long long begin, unsigned long long end, unsigned long long (&cnt)[3]) {
    ClosestArgs<T> a = a0;
    std::vector<uint32_t> lds_node(size_t(kClosestLds) * kBlock);
    std::vector<T> lds_d2(size_t(kClosestLds) * kBlock);
    std::vector<uint32_t> deep_nodes(Deep ? a.deep_cap : 1);
    std::vector<T> deep_d2(Deep ? a.deep_cap : 1);
    a.deep_nodes = deep_nodes.data(); a.deep_d2 = deep_d2.data();            // one lane at a time: lane 0's spill
    for (unsigned long long s = begin; s < end; ++s) closest_lane<T, Leaf, true, Deep>(a, s, lds_node.data(), lds_d2.data(), 0, 0, cnt);
}

template <typename T, int Leaf>
int walk(const void* pairs, uint32_t root_index, const void* prims, const void* queries, size_t n, const uint32_t* order, const uint32_t* prim_ids,
         uint32_t deep_cap, int threads, void* hits, unsigned long long* counters3) {
    ClosestArgs<T> a{};
    a.pairs = static_cast<const PairNode<T>*>(pairs); a.prims = static_cast<const T*>(prims); a.queries = static_cast<const T*>(queries);
    a.hits = static_cast<typename HitOf<T>::Type*>(hits); a.n = n; a.first = 0; a.order = order; a.prim_ids = prim_ids; a.counters = nullptr;
    a.deep_cap = deep_cap; a.root_index = root_index;
    run_lanes(n, threads, counters3, [&](unsigned long long b, unsigned long long e, unsigned long long (&cnt)[3]) {
        if (deep_cap) walk_range<T, Leaf, true>(a, b, e, cnt); else walk_range<T, Leaf, false>(a, b, e, cnt);
    });
    return 0;
}

// One launch of a sliced batch as the device runs it (prelude: GuardedSpill, run_slice): both spill arrays sized for the launch's lanes.
template <typename T, int Leaf>
long long walk_slice(const void* pairs, uint32_t root_index, const void* prims, const void* queries, size_t first, size_t n, size_t launch_lanes,
                     const uint32_t* order, const uint32_t* prim_ids, uint32_t deep_cap, void* hits, unsigned long long* counters3) {
    if (deep_cap == 0 || n > launch_lanes) return kSliceBadArgs;
    ClosestArgs<T> a{};
    a.pairs = static_cast<const PairNode<T>*>(pairs); a.prims = static_cast<const T*>(prims); a.queries = static_cast<const T*>(queries);
    a.hits = static_cast<typename HitOf<T>::Type*>(hits); a.n = n; a.first = first; a.order = order; a.prim_ids = prim_ids; a.counters = nullptr;
    a.deep_cap = deep_cap; a.root_index = root_index;
    GuardedSpill<uint32_t> deep_nodes(first, launch_lanes, deep_cap);
    GuardedSpill<T> deep_d2(first, launch_lanes, deep_cap);
    a.deep_nodes = deep_nodes.data(); a.deep_d2 = deep_d2.data();
    std::vector<uint32_t> lds_node(size_t(kClosestLds) * kBlock);
    std::vector<T> lds_d2(size_t(kClosestLds) * kBlock);
    run_slice(n, kBlock, counters3, [&](unsigned long long lane, int tid, unsigned long long (&cnt)[3]) {
        closest_lane<T, Leaf, true, true>(a, first + lane, lds_node.data(), lds_d2.data(), tid, lane, cnt);
    });
    if (!deep_nodes.guards_intact() || !deep_d2.guards_intact()) return kSliceGuardBroken;
    return deep_nodes.overwritten() + deep_d2.overwritten();
}

template <typename T, int Leaf>
T prim_dist2(const T* prims, size_t i, const T (&q)[3], T& u, T& v) {
    u = T(0); v = T(0);
    if (Leaf == LEAF_TRIANGLE) { T p[12]; std::memcpy(p, prims + 12 * i, sizeof(p)); return tri_dist2(p, q, u, v); }
    T s[4]; std::memcpy(s, prims + 4 * i, sizeof(s)); return sphere_dist2(s, q);
}

// every query against every primitive through the same distance function: the smallest d2, ties to the lowest index
template <typename T, int Leaf>
void brute(const T* prims, size_t n_prims, const T* queries, size_t n, T* out_d2, uint32_t* out_prim, int threads) {
    const int nt = std::max(1, threads);
    std::vector<std::thread> pool;
    for (int t = 0; t < nt; ++t) {
        pool.emplace_back([=] {
            for (size_t k = n * t / nt; k < n * (t + 1) / nt; ++k) {
                const T q[3] = { queries[4 * k], queries[4 * k + 1], queries[4 * k + 2] };
                T best = T(0); uint32_t bi = BVH_AMD_INVALID;
                for (size_t i = 0; i < n_prims; ++i) {
                    T u, v;
                    const T d2 = prim_dist2<T, Leaf>(prims, i, q, u, v);
                    if (bi == BVH_AMD_INVALID || d2 < best) { best = d2; bi = static_cast<uint32_t>(i); }
                }
                out_d2[k] = best; out_prim[k] = bi;
            }
        });
    }
    for (auto& th : pool) th.join();
}

} // namespace

extern "C" {

// d2[k] = squared distance of query k to primitive prim[k] (the kernel's function); u, v likewise (NULL: not wanted)
void closest_host_eval(int is_double, int leaf, const void* prims, const void* queries, size_t n, const uint32_t* prim, void* d2, void* u, void* v) {
    for (size_t k = 0; k < n; ++k) {
        if (is_double) {
            const double* qq = static_cast<const double*>(queries) + 4 * k;
            const double q[3] = { qq[0], qq[1], qq[2] };
            double uu, vv;
            const double r = leaf == LEAF_SPHERE ? prim_dist2<double, LEAF_SPHERE>(static_cast<const double*>(prims), prim[k], q, uu, vv)
                                                 : prim_dist2<double, LEAF_TRIANGLE>(static_cast<const double*>(prims), prim[k], q, uu, vv);
            static_cast<double*>(d2)[k] = r;
            if (u) static_cast<double*>(u)[k] = uu;
            if (v) static_cast<double*>(v)[k] = vv;
        } else {
            const float* qq = static_cast<const float*>(queries) + 4 * k;
            const float q[3] = { qq[0], qq[1], qq[2] };
            float uu, vv;
            const float r = leaf == LEAF_SPHERE ? prim_dist2<float, LEAF_SPHERE>(static_cast<const float*>(prims), prim[k], q, uu, vv)
                                                : prim_dist2<float, LEAF_TRIANGLE>(static_cast<const float*>(prims), prim[k], q, uu, vv);
            static_cast<float*>(d2)[k] = r;
            if (u) static_cast<float*>(u)[k] = uu;
            if (v) static_cast<float*>(v)[k] = vv;
        }
    }
}

// brute force over all n_prims primitives with the kernel's distance function (no radius): d2 and index of the nearest, ties to the lowest
void closest_host_brute(int is_double, int leaf, const void* prims, size_t n_prims, const void* queries, size_t n, void* out_d2, uint32_t* out_prim, int threads) {
    if (is_double) {
        if (leaf == LEAF_SPHERE) brute<double, LEAF_SPHERE>(static_cast<const double*>(prims), n_prims, static_cast<const double*>(queries), n, static_cast<double*>(out_d2), out_prim, threads);
        else brute<double, LEAF_TRIANGLE>(static_cast<const double*>(prims), n_prims, static_cast<const double*>(queries), n, static_cast<double*>(out_d2), out_prim, threads);
    } else {
        if (leaf == LEAF_SPHERE) brute<float, LEAF_SPHERE>(static_cast<const float*>(prims), n_prims, static_cast<const float*>(queries), n, static_cast<float*>(out_d2), out_prim, threads);
        else brute<float, LEAF_TRIANGLE>(static_cast<const float*>(prims), n_prims, static_cast<const float*>(queries), n, static_cast<float*>(out_d2), out_prim, threads);
    }
}

// Squared distance from q (3 scalars) to one PrecomputedTri (12) / Sphere (4); out = {d2, u, v}.
void closest_host_tri(int is_double, const void* prim12, const void* q3, void* out3) {
    if (is_double) {
        double p[12], q[3], u = 0, v = 0;
        std::memcpy(p, prim12, sizeof(p)); std::memcpy(q, q3, sizeof(q));
        const double d2 = tri_dist2(p, q, u, v);
        double o[3] = {d2, u, v}; std::memcpy(out3, o, sizeof(o));
    } else {
        float p[12], q[3], u = 0, v = 0;
        std::memcpy(p, prim12, sizeof(p)); std::memcpy(q, q3, sizeof(q));
        const float d2 = tri_dist2(p, q, u, v);
        float o[3] = {d2, u, v}; std::memcpy(out3, o, sizeof(o));
    }
}
void closest_host_sphere(int is_double, const void* s4, const void* q3, void* out1) {
    if (is_double) {
        double s[4], q[3]; std::memcpy(s, s4, sizeof(s)); std::memcpy(q, q3, sizeof(q));
        const double d2 = sphere_dist2(s, q); std::memcpy(out1, &d2, sizeof(d2));
    } else {
        float s[4], q[3]; std::memcpy(s, s4, sizeof(s)); std::memcpy(q, q3, sizeof(q));
        const float d2 = sphere_dist2(s, q); std::memcpy(out1, &d2, sizeof(d2));
    }
}

// The kernel's walk for n queries {x, y, z, max_distance} (slot s reads query order[s], or s); leaf 0 = triangles, 1 = spheres;
// prim_ids (optional) = BVH_AMD_RAY_ORIGINAL_IDS; deep_cap > 0: the HBM spill of trees deeper than 64 levels, deep_cap entries.
// hits: bvh_hit3f / bvh_hit3d records; counters3 = {pairs fetched, primitives tested, leaves visited}. Returns 0.
int closest_host_walk(int is_double, int leaf, const void* pairs, uint32_t root_index, const void* prims, const void* queries, size_t n,
                      const uint32_t* order, const uint32_t* prim_ids, uint32_t deep_cap, int threads, void* hits, unsigned long long* counters3) {
    if (is_double) {
        if (leaf == LEAF_SPHERE) return walk<double, LEAF_SPHERE>(pairs, root_index, prims, queries, n, order, prim_ids, deep_cap, threads, hits, counters3);
        return walk<double, LEAF_TRIANGLE>(pairs, root_index, prims, queries, n, order, prim_ids, deep_cap, threads, hits, counters3);
    }
    if (leaf == LEAF_SPHERE) return walk<float, LEAF_SPHERE>(pairs, root_index, prims, queries, n, order, prim_ids, deep_cap, threads, hits, counters3);
    return walk<float, LEAF_TRIANGLE>(pairs, root_index, prims, queries, n, order, prim_ids, deep_cap, threads, hits, counters3);
}

// One launch of a batch that point_query_run cut into slices (a tree deeper than 64 levels: deep_cap > 0): slots [first, first + n) as
// the device walks them — a.first = first, slot = first + lane, lane = 0 .. n-1 indexing spill arrays of launch_lanes * deep_cap
// entries that the launch's lanes share, tid = lane % 256 in one LDS stand-in. queries, order and hits are the whole batch's.
// counters3 = the launch's counters. Returns the spill entries the launch overwrote (both arrays), -1 if a guard zone around a
// spill array was written to, -2 for deep_cap == 0 or n > launch_lanes.
long long closest_host_walk_slice(int is_double, int leaf, const void* pairs, uint32_t root_index, const void* prims, const void* queries, size_t first,
                                  size_t n, size_t launch_lanes, const uint32_t* order, const uint32_t* prim_ids, uint32_t deep_cap, void* hits,
                                  unsigned long long* counters3) {
    if (is_double) {
        if (leaf == LEAF_SPHERE) return walk_slice<double, LEAF_SPHERE>(pairs, root_index, prims, queries, first, n, launch_lanes, order, prim_ids, deep_cap, hits, counters3);
        return walk_slice<double, LEAF_TRIANGLE>(pairs, root_index, prims, queries, first, n, launch_lanes, order, prim_ids, deep_cap, hits, counters3);
    }
    if (leaf == LEAF_SPHERE) return walk_slice<float, LEAF_SPHERE>(pairs, root_index, prims, queries, first, n, launch_lanes, order, prim_ids, deep_cap, hits, counters3);
    return walk_slice<float, LEAF_TRIANGLE>(pairs, root_index, prims, queries, first, n, launch_lanes, order, prim_ids, deep_cap, hits, counters3);
}

} // extern "C"
