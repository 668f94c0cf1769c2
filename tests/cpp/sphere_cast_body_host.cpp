// TEST INFRASTRUCTURE (CPU, no GPU): compiles the text of the sphere-cast kernel — bvh_amd/csrc/sphere_cast_body.inc (over
// nearest_walk.inc, point_walk.inc's distance functions and the ray arithmetic of bvh_amd/csrc/trace_device.h) — for the HOST and runs
// it with one emulated lane per query (the queries of a batch one after another, or split over host threads). What it can show: the
// sweep test of the very source the device runs finds the first contact of a moving ball with a triangle or a sphere, and the walk
// returns what a brute force over the same function returns; the device's records and counters must equal these bit for bit. What
// it cannot show: anything that needs the hardware. tests/test_sphere_cast_host.py drives it; tests/test_gpu_sphere_cast.py uses it too.
//
// Built by the tests with: g++ -std=c++20 -O1 -mavx2 -mfma -ffp-contract=off -fno-strict-aliasing -shared -fPIC -pthread.
#include <type_traits>

#include "host_lane_prelude.h"
#include "../../bvh_amd/csrc/sphere_cast_body.inc"

namespace {

using namespace bvh_amd;

template <typename T>
SphereCastArgs<T> make_args(const void* pairs, uint32_t root_index, const void* prims, const void* rays, size_t first, size_t n, double radius,
                            const void* radii, const uint32_t* order, const uint32_t* prim_ids, uint32_t deep_cap, void* hits) {
    SphereCastArgs<T> a{};
    a.pairs = static_cast<const PairNode<T>*>(pairs); a.prims = static_cast<const T*>(prims); a.queries = static_cast<const T*>(rays);
    a.hits = static_cast<typename HitOf<T>::Type*>(hits); a.radii = static_cast<const T*>(radii); a.radius = static_cast<T>(radius);
    a.n = n; a.first = first; a.order = order; a.prim_ids = prim_ids; a.counters = nullptr;
    a.deep_cap = deep_cap; a.root_index = root_index;
    return a;
}

template <typename T, int Leaf, bool Robust, bool Deep>
void walk_range(const SphereCastArgs<T>& a0, unsigned long long begin, unsigned long long end, unsigned long long (&cnt)[3]) {
    SphereCastArgs<T> a = a0;
    std::vector<uint32_t> lds_node(size_t(kClosestLds) * kBlock);
    std::vector<T> lds_t(size_t(kClosestLds) * kBlock);
    std::vector<uint32_t> deep_nodes(Deep ? a.deep_cap : 1);
    std::vector<T> deep_t(Deep ? a.deep_cap : 1);
    a.deep_nodes = deep_nodes.data(); a.deep_t = deep_t.data();              // one lane at a time: lane 0's spill
    for (unsigned long long s = begin; s < end; ++s) sphere_cast_lane<T, Leaf, Robust, true, Deep>(a, s, lds_node.data(), lds_t.data(), int(s % kBlock), 0, cnt);
}

template <typename T, int Leaf, bool Robust>
int walk(const void* pairs, uint32_t root_index, const void* prims, const void* rays, size_t n, double radius, const void* radii, const uint32_t* order,
         const uint32_t* prim_ids, uint32_t deep_cap, int threads, void* hits, unsigned long long* counters3) {
    const SphereCastArgs<T> a = make_args<T>(pairs, root_index, prims, rays, 0, n, radius, radii, order, prim_ids, deep_cap, hits);
    run_lanes(n, threads, counters3, [&](unsigned long long b, unsigned long long e, unsigned long long (&cnt)[3]) {
        if (deep_cap) walk_range<T, Leaf, Robust, true>(a, b, e, cnt); else walk_range<T, Leaf, Robust, false>(a, b, e, cnt);
    });
    return 0;
}

// every query against every primitive through the same sweep test and the walk's update rule: argmin by (t, index)
template <typename T, int Leaf>
void brute(const T* prims, size_t n_prims, const T* rays, size_t n, double radius, const T* radii, typename HitOf<T>::Type* hits, int threads,
           unsigned long long* tests) {
    const int nt = std::max(1, threads);
    std::vector<std::thread> pool;
    for (int th = 0; th < nt; ++th) {
        pool.emplace_back([=] {
            for (size_t k = n * th / nt; k < n * (th + 1) / nt; ++k) {
                const T* r = rays + 8 * k;
                const T org[3] = { r[0], r[1], r[2] }, dir[3] = { r[3], r[4], r[5] };
                const T tmin = r[6], tmax = r[7], rad = radii ? radii[k] : static_cast<T>(radius);
                const T c0[3] = { org[0] + tmin * dir[0], org[1] + tmin * dir[1], org[2] + tmin * dir[2] };
                T best = tmax, bu = T(0), bv = T(0);
                uint32_t bi = BVH_AMD_INVALID;
                if (tmin == tmin && tmax == tmax && rad >= T(0)) {
                    for (size_t i = 0; i < n_prims; ++i) {
                        T t = T(0), u = T(0), v = T(0);
                        if (sphere_cast_test<T, Leaf>(prims, uint32_t(i), org, c0, dir, tmin, best, rad, t, u, v) && (t < best || (t == best && i < bi))) {
                            best = t; bi = uint32_t(i); bu = u; bv = v;
                        }
                    }
                }
                store_hit(hits + k, bi, best, bu, bv);
            }
        });
    }
    for (auto& th : pool) th.join();
    *tests = static_cast<unsigned long long>(n) * n_prims;
}

// f.template operator()<T, Leaf, Robust>() for the three run-time choices
template <typename F>
auto pick(int is_double, int leaf, int robust, F f) {
    auto by_robust = [&](auto t, auto l) {
        using T = decltype(t);
        return robust ? f.template operator()<T, decltype(l)::value, true>() : f.template operator()<T, decltype(l)::value, false>();
    };
    auto by_leaf = [&](auto t) {
        return leaf == LEAF_SPHERE ? by_robust(t, std::integral_constant<int, LEAF_SPHERE>{}) : by_robust(t, std::integral_constant<int, LEAF_TRIANGLE>{});
    };
    return is_double ? by_leaf(double{}) : by_leaf(float{});
}

// one ray {org, dir, tmin, tmax} and radius against one primitive: out4 = {1 / 0, t, u, v}
template <typename T, int Leaf>
void one(const void* prim, const void* ray8, double radius, void* out4) {
    T r[8];
    std::memcpy(r, ray8, sizeof(r));
    const T org[3] = { r[0], r[1], r[2] }, dir[3] = { r[3], r[4], r[5] };
    const T c0[3] = { org[0] + r[6] * dir[0], org[1] + r[6] * dir[1], org[2] + r[6] * dir[2] };
    T t = T(0), u = T(0), v = T(0);
    const bool hit = sphere_cast_test<T, Leaf>(static_cast<const T*>(prim), 0, org, c0, dir, r[6], r[7], static_cast<T>(radius), t, u, v);
    const T o[4] = { hit ? T(1) : T(0), t, u, v };
    std::memcpy(out4, o, sizeof(o));
}

} // namespace

extern "C" {

// The sweep test of n (ray, radius, primitive) triples, row k of each array: out4[k] = {1 / 0, t, u, v}. leaf 0: prims holds 12
// scalars per row (PrecomputedTri), 1: 4 (sphere).
void sphere_cast_host_pairs(int is_double, int leaf, const void* prims, const void* rays, const void* radii, size_t n, void* out4) {
    const size_t sz = is_double ? 8 : 4, pw = leaf == LEAF_SPHERE ? 4 : 12;
    for (size_t k = 0; k < n; ++k) {
        const char* p = static_cast<const char*>(prims) + k * pw * sz;
        const char* r = static_cast<const char*>(rays) + k * 8 * sz;
        char* o = static_cast<char*>(out4) + k * 4 * sz;
        if (is_double) {
            const double rad = static_cast<const double*>(radii)[k];
            if (leaf == LEAF_SPHERE) one<double, LEAF_SPHERE>(p, r, rad, o); else one<double, LEAF_TRIANGLE>(p, r, rad, o);
        } else {
            const double rad = static_cast<const float*>(radii)[k];
            if (leaf == LEAF_SPHERE) one<float, LEAF_SPHERE>(p, r, rad, o); else one<float, LEAF_TRIANGLE>(p, r, rad, o);
        }
    }
}

// The kernel's walk for n rays {org, dir, tmin, tmax} (slot s reads ray order[s], or s) with radii[q] (or `radius` when radii is NULL);
// leaf 0 = triangles, 1 = spheres; robust = the robust node test; prim_ids (optional) = BVH_AMD_RAY_ORIGINAL_IDS; deep_cap > 0: the HBM
// spill of trees deeper than 64 levels, deep_cap entries. hits: bvh_hit3f / bvh_hit3d records; counters3 = {pairs fetched, primitives
// tested, leaves visited}. Returns 0.
int sphere_cast_host_walk(int is_double, int leaf, int robust, const void* pairs, uint32_t root_index, const void* prims, const void* rays, size_t n,
                          double radius, const void* radii, const uint32_t* order, const uint32_t* prim_ids, uint32_t deep_cap, int threads, void* hits,
                          unsigned long long* counters3) {
    return pick(is_double, leaf, robust, [&]<typename T, int Leaf, bool Robust>() {
        return walk<T, Leaf, Robust>(pairs, root_index, prims, rays, n, radius, radii, order, prim_ids, deep_cap, threads, hits, counters3);
    });
}

// Brute force over all n_prims primitives with the kernel's sweep test and update rule: one record per ray (BVH-order prim);
// *tests = the primitives it tested.
void sphere_cast_host_brute(int is_double, int leaf, const void* prims, size_t n_prims, const void* rays, size_t n, double radius, const void* radii,
                            void* hits, int threads, unsigned long long* tests) {
    pick(is_double, leaf, 0, [&]<typename T, int Leaf, bool Robust>() {
        brute<T, Leaf>(static_cast<const T*>(prims), n_prims, static_cast<const T*>(rays), n, radius, static_cast<const T*>(radii),
                       static_cast<typename HitOf<T>::Type*>(hits), threads, tests);
        return 0;
    });
}

} // extern "C"
