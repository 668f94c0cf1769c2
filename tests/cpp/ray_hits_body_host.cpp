// TEST INFRASTRUCTURE (CPU, no GPU): compiles the text of the all-hits ray kernel — bvh_amd/csrc/ray_hits_body.inc (over list_walk.inc, the
// walk it shares with the radius and overlap queries, tri_test.inc and the ray arithmetic of bvh_amd/csrc/trace_device.h) — for the HOST
// and runs it with one emulated lane per ray (the rays of a batch one after another, or split over host threads). What it can show:
// the walk of the very source the device runs lists what the reference's own intersect reports for every primitive alone, in the
// tree's order, and keeps to its segment; the device's counts and records must equal these bit for bit. What it cannot show:
// anything that needs the hardware. tests/test_ray_hits_host.py drives it; tests/test_gpu_ray_hits.py uses it too.
// It also holds two deliberately WRONG walks (mutant 1: a hit shortens tmax, as closest-hit does; mutant 2: the nearer child first):
// the tests must tell each of them from the body.
//
// Built by the tests with: g++ -std=c++20 -O1 -mavx2 -mfma -ffp-contract=off -fno-strict-aliasing -shared -fPIC -pthread.
#include <type_traits>

#include "host_lane_prelude.h"
#include "../../bvh_amd/csrc/ray_hits_body.inc"

namespace {

using namespace bvh_amd;

template <typename T, int Leaf, bool Robust, bool Deep>
void walk_range(const RayHitsArgs<T>& a0, unsigned long long begin, unsigned long long end, unsigned long long (&cnt)[3]) {
    RayHitsArgs<T> a = a0;
    std::vector<uint32_t> lds_node(size_t(kRayHitsLds) * kBlock);
    std::vector<uint32_t> deep_nodes(Deep ? a.deep_cap : 1);
    a.deep_nodes = deep_nodes.data();                                        // one lane at a time: lane 0's spill
    for (unsigned long long s = begin; s < end; ++s) {
        if (a.offsets) ray_hits_lane<T, Leaf, Robust, true, Deep, true>(a, s, lds_node.data(), 0, 0, cnt);
        else ray_hits_lane<T, Leaf, Robust, true, Deep, false>(a, s, lds_node.data(), 0, 0, cnt);
    }
}

// The wrong walks. Same tests, same output protocol; shorten: an accepted hit becomes the ray's tmax for everything after it;
// near_first: of two children the ray meets, the one it enters first is walked first.
template <typename T, int Leaf, bool Robust>
void mutant_lane(const RayHitsArgs<T>& a, unsigned long long qi, bool shorten, bool near_first) {
    const T* r = a.queries + 8 * qi;
    const T org[3] = { r[0], r[1], r[2] }, dir[3] = { r[3], r[4], r[5] };
    const T tmin = r[6];
    T ray_tmax = r[7];
    const T pad_t = r[7];
    T inv[3], aux[3];
    uint32_t oct[3];
    ray_constants<T, Robust, 3>(org, dir, inv, aux, oct);
    unsigned long long seg_begin = 0, seg_len = 0;
    if (a.offsets) { seg_begin = a.offsets[qi]; seg_len = a.offsets[qi + 1] > seg_begin ? a.offsets[qi + 1] - seg_begin : 0; }
    uint32_t found = 0;
    std::vector<uint32_t> stack;
    if (tmin == tmin && ray_tmax == ray_tmax) stack.push_back(a.root_index);
    while (!stack.empty()) {
        const uint32_t node = stack.back();
        stack.pop_back();
        if ((node & kCountMask) == 0) {
            T lb[6], rb[6], l0, l1, r0, r1;
            uint32_t li = 0, ri = 0;
            load_pair(a.pairs + (node >> (kCountBits + 1)), lb, rb, li, ri);
            slab_pair<T, Robust, 3>(lb, rb, org, inv, aux, oct, tmin, ray_tmax, l0, l1, r0, r1);
            const bool hl = l0 <= l1, hr = r0 <= r1;
            if (hl && hr && near_first && l0 > r0) { stack.push_back(li); stack.push_back(ri); }
            else { if (hr) stack.push_back(ri); if (hl) stack.push_back(li); }
            continue;
        }
        for (uint32_t i = node >> kCountBits; i < (node >> kCountBits) + (node & kCountMask); ++i) {
            T tmax = ray_tmax, hit_t = T(0), hit_u = T(0), hit_v = T(0);
            bool accepted = false;
            if (Leaf == LEAF_TRIANGLE) {
                T p[12];
                load_prim12(a.prims + 12ull * i, p);
#define BVH_TRI_ACCEPTED accepted = true
#include "../../bvh_amd/csrc/tri_test.inc"
#undef BVH_TRI_ACCEPTED
            } else {
                T s[4];
                load_prim4(a.prims + 4ull * i, s);
                const T o0 = org[0] - s[0], o1 = org[1] - s[1], o2 = org[2] - s[2];
                const T qa = dot3(dir[0], dir[1], dir[2], dir[0], dir[1], dir[2]), qb = T(2) * dot3(dir[0], dir[1], dir[2], o0, o1, o2);
                const T qc = dot3(o0, o1, o2, o0, o1, o2) - s[3] * s[3];
                const T delta = qb * qb - T(4) * qa * qc;
                if (delta >= 0) {
                    const T iv = -T(0.5) / qa, root = Num<T>::sqrt_(delta);
                    const T t0 = pick_max((qb + root) * iv, tmin), t1 = pick_min((qb - root) * iv, tmax);
                    if (t0 <= t1) { hit_t = t0; hit_u = t1; accepted = true; }
                }
            }
            if (!accepted) continue;
            if (shorten) ray_tmax = hit_t;
            if (a.offsets && found < seg_len) store_hit(a.list_hits + seg_begin + found, a.prim_ids ? a.prim_ids[i] : i, hit_t, hit_u, hit_v);
            ++found;
        }
    }
    if (a.counts) a.counts[qi] = found;
    if (a.offsets) for (unsigned long long k = found; k < seg_len; ++k) store_hit(a.list_hits + seg_begin + k, BVH_AMD_INVALID, pad_t, T(0), T(0));
}

template <typename T>
RayHitsArgs<T> make_args(const void* pairs, uint32_t root_index, const void* prims, const void* rays, size_t first, size_t n, const uint32_t* order,
                         const uint32_t* prim_ids, uint32_t deep_cap, uint32_t* counts, const uint64_t* offsets, void* list_hits) {
    RayHitsArgs<T> a{};
    a.pairs = static_cast<const PairNode<T>*>(pairs); a.prims = static_cast<const T*>(prims); a.queries = static_cast<const T*>(rays);
    a.counts = counts; a.offsets = reinterpret_cast<const unsigned long long*>(offsets); a.list_prims = nullptr;
    a.list_hits = static_cast<typename HitOf<T>::Type*>(list_hits);
    a.n = n; a.first = first; a.order = order; a.prim_ids = prim_ids; a.counters = nullptr;
    a.deep_cap = deep_cap; a.root_index = root_index;
    return a;
}

template <typename T, int Leaf, bool Robust>
int walk(int mutant, const void* pairs, uint32_t root_index, const void* prims, const void* rays, size_t n, const uint32_t* order, const uint32_t* prim_ids,
         uint32_t deep_cap, int threads, uint32_t* counts, const uint64_t* offsets, void* list_hits, unsigned long long* counters3) {
    const RayHitsArgs<T> a = make_args<T>(pairs, root_index, prims, rays, 0, n, order, prim_ids, deep_cap, counts, offsets, list_hits);
    if (mutant) {
        for (size_t s = 0; s < n; ++s) mutant_lane<T, Leaf, Robust>(a, order ? order[s] : s, mutant == 1, mutant == 2);
        counters3[0] = counters3[1] = counters3[2] = 0;
        return 0;
    }
    run_lanes(n, threads, counters3, [&](unsigned long long b, unsigned long long e, unsigned long long (&cnt)[3]) {
        if (deep_cap) walk_range<T, Leaf, Robust, true>(a, b, e, cnt); else walk_range<T, Leaf, Robust, false>(a, b, e, cnt);
    });
    return 0;
}

// One launch of a sliced batch as the device runs it (prelude: GuardedSpill, run_slice): the spill sized for the launch's lanes.
template <typename T, int Leaf, bool Robust>
long long walk_slice(const void* pairs, uint32_t root_index, const void* prims, const void* rays, size_t first, size_t n, size_t launch_lanes,
                     const uint32_t* order, const uint32_t* prim_ids, uint32_t deep_cap, uint32_t* counts, const uint64_t* offsets, void* list_hits,
                     unsigned long long* counters3) {
    if (deep_cap == 0 || n > launch_lanes) return kSliceBadArgs;
    RayHitsArgs<T> a = make_args<T>(pairs, root_index, prims, rays, first, n, order, prim_ids, deep_cap, counts, offsets, list_hits);
    GuardedSpill<uint32_t> deep_nodes(first, launch_lanes, deep_cap);
    a.deep_nodes = deep_nodes.data();
    std::vector<uint32_t> lds_node(size_t(kRayHitsLds) * kBlock);
    run_slice(n, kBlock, counters3, [&](unsigned long long lane, int tid, unsigned long long (&cnt)[3]) {
        if (a.offsets) ray_hits_lane<T, Leaf, Robust, true, true, true>(a, first + lane, lds_node.data(), tid, lane, cnt);
        else ray_hits_lane<T, Leaf, Robust, true, true, false>(a, first + lane, lds_node.data(), tid, lane, cnt);
    });
    if (!deep_nodes.guards_intact()) return kSliceGuardBroken;
    return deep_nodes.overwritten();
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

} // namespace

extern "C" {

// The kernel's walk for n rays {org, dir, tmin, tmax} (slot s reads ray order[s], or s); leaf 0 = triangles, 1 = spheres; robust = the
// robust node test; mutant 0 = the body, 1 / 2 = the wrong walks above (no counters); prim_ids (optional) = BVH_AMD_RAY_ORIGINAL_IDS;
// deep_cap > 0: the HBM spill of trees deeper than 64 levels, deep_cap entries. counts (optional), offsets (optional: NULL = the
// count-pass variant), list_hits (bvh_hit3f / bvh_hit3d records) as in the C ABI; counters3 = {pairs fetched, primitives tested, leaves
// visited}. With threads > 1 the rays' segments must not overlap. Returns 0.
int ray_hits_host_walk(int is_double, int leaf, int robust, int mutant, const void* pairs, uint32_t root_index, const void* prims, const void* rays, size_t n,
                       const uint32_t* order, const uint32_t* prim_ids, uint32_t deep_cap, int threads, uint32_t* counts, const uint64_t* offsets,
                       void* list_hits, unsigned long long* counters3) {
    return pick(is_double, leaf, robust, [&]<typename T, int Leaf, bool Robust>() {
        return walk<T, Leaf, Robust>(mutant, pairs, root_index, prims, rays, n, order, prim_ids, deep_cap, threads, counts, offsets, list_hits, counters3);
    });
}

// One launch of a batch that point_query_run cut into slices (deep_cap > 0): slots [first, first + n) as the device walks them. Returns
// the spill entries the launch overwrote, -1 if a guard zone around the spill was written to, -2 for deep_cap == 0 or n > launch_lanes.
long long ray_hits_host_walk_slice(int is_double, int leaf, int robust, const void* pairs, uint32_t root_index, const void* prims, const void* rays,
                                   size_t first, size_t n, size_t launch_lanes, const uint32_t* order, const uint32_t* prim_ids, uint32_t deep_cap,
                                   uint32_t* counts, const uint64_t* offsets, void* list_hits, unsigned long long* counters3) {
    return pick(is_double, leaf, robust, [&]<typename T, int Leaf, bool Robust>() {
        return walk_slice<T, Leaf, Robust>(pairs, root_index, prims, rays, first, n, launch_lanes, order, prim_ids, deep_cap, counts, offsets, list_hits, counters3);
    });
}

} // extern "C"
