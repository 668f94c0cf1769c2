// TEST INFRASTRUCTURE (CPU, no GPU): compiles the text of the nearest-hits ray kernel — bvh_amd/csrc/ray_nearest_body.inc (over knn_heap.inc,
// the candidate heap it shares with the k-nearest point query, tri_test.inc and the ray arithmetic of bvh_amd/csrc/trace_device.h) — for
// the HOST and runs it with one emulated lane per ray (the rays of a batch one after another, or split over host threads), at any
// lane stride of the LDS arrays. What it can show: the walk of the very source the device runs returns, for every ray, the first k
// records of the reference's own hit list sorted by (t, prim), padded as the contract says, and keeps to its row and to its LDS; the
// device's rows, counts and counters must equal these bit for bit. What it cannot show: anything that needs the hardware.
// tests/test_ray_nearest_host.py drives it; tests/test_gpu_ray_nearest.py uses it too.
// It also holds two deliberately WRONG walks (mutant 1: of two candidates at the same t the one tested later wins, closest-hit's rule;
// mutant 2: a sphere's t1 is clipped to the shortened tmax, closest-hit's record): the tests must tell each of them from the body.
//
// Built by the tests with: g++ -std=c++20 -O1 -mavx2 -mfma -ffp-contract=off -fno-strict-aliasing -shared -fPIC -pthread.
#include <atomic>
#include <type_traits>

#include "host_lane_prelude.h"
#include "../../bvh_amd/csrc/ray_nearest_body.inc"

namespace {

using namespace bvh_amd;

// One lane at a time, sitting at column (slot mod stride) of a block's LDS arrays: the other columns are never touched.
// The block's LDS is allocated at exactly knn_lds_bytes between two zones of sentinel words: false if a lane wrote outside it.
constexpr size_t kLdsGuardWords = 64;
constexpr unsigned long long kLdsSentinel = 0xA5A5A5A5A5A5A5A5ull;

template <typename T, int Leaf, bool Robust, bool Deep>
bool walk_range(const RayNearestArgs<T>& a0, uint32_t stride, unsigned long long begin, unsigned long long end, unsigned long long (&cnt)[3]) {
    RayNearestArgs<T> a = a0;
    const size_t words = knn_lds_bytes<T>(a.k, stride) / 8;                  // (a multiple of 8 bytes: stride is even)
    std::vector<unsigned long long> raw(words + 2 * kLdsGuardWords, kLdsSentinel);
    const KnnLds<T> lds = knn_lds_carve<T>(raw.data() + kLdsGuardWords, a.k, stride);
    std::vector<uint32_t> deep_nodes(Deep ? a.deep_cap : 1);
    std::vector<T> deep_t(Deep ? a.deep_cap : 1);
    a.deep_nodes = deep_nodes.data();                                        // lane 0's spill
    a.deep_t = deep_t.data();
    for (unsigned long long s = begin; s < end; ++s) ray_nearest_lane<T, Leaf, Robust, true, Deep>(a, s, lds, stride, int(s % stride), 0, cnt);
    for (size_t w = 0; w < kLdsGuardWords; ++w)
        if (raw[w] != kLdsSentinel || raw[kLdsGuardWords + words + w] != kLdsSentinel) return false;
    return true;
}

// The wrong walks. The body's descent, pruning and output protocol, the candidates in a sorted vector. later_wins: candidates at the
// same t are ordered by the REVERSE of the order they were tested in, so the later one wins a place (at k = 1: what closest-hit keeps).
// clip_t1: a sphere's t1 = min(exit, worst), the shortened tmax, instead of min(exit, the ray's tmax).
template <typename T, int Leaf, bool Robust>
void mutant_lane(const RayNearestArgs<T>& a, unsigned long long qi, bool later_wins, bool clip_t1) {
    struct Cand { T t, u, v; uint32_t i; unsigned long long seq; };
    const T* r = a.queries + 8 * qi;
    const T org[3] = { r[0], r[1], r[2] }, dir[3] = { r[3], r[4], r[5] };
    const T tmin = r[6], ray_tmax = r[7];
    T inv[3], aux[3];
    uint32_t oct[3];
    ray_constants<T, Robust, 3>(org, dir, inv, aux, oct);
    auto less = [&](const Cand& x, const Cand& y) {
        if (x.t != y.t) return x.t < y.t;
        return later_wins ? x.seq > y.seq : x.i < y.i;
    };
    std::vector<Cand> held;
    T worst = ray_tmax;
    unsigned long long seq = 0;
    struct Entry { uint32_t node; T t; };
    std::vector<Entry> stack;
    if (tmin == tmin && ray_tmax == ray_tmax) stack.push_back({a.root_index, ray_tmax});      // (the root is never dropped)
    while (!stack.empty()) {
        const Entry e = stack.back();
        stack.pop_back();
        if (e.t > worst) continue;
        uint32_t node = e.node;
        while ((node & kCountMask) == 0) {
            T lb[6], rb[6], l0, l1, r0, r1;
            uint32_t li = 0, ri = 0;
            load_pair(a.pairs + (node >> (kCountBits + 1)), lb, rb, li, ri);
            slab_pair<T, Robust, 3>(lb, rb, org, inv, aux, oct, tmin, worst, l0, l1, r0, r1);
            const bool hl = l0 <= l1, hr = r0 <= r1;
            if (hl && hr) {
                if (l0 > r0) { stack.push_back({li, l0}); node = ri; }
                else { stack.push_back({ri, r0}); node = li; }
            } else if (hl) node = li;
            else if (hr) node = ri;
            else { node = 0xFFFFFFFFu; break; }
        }
        if (node == 0xFFFFFFFFu) continue;
        for (uint32_t i = node >> kCountBits; i < (node >> kCountBits) + (node & kCountMask); ++i) {
            Cand c{T(0), T(0), T(0), i, seq++};
            if (!ray_nearest_test<T, Leaf>(a.prims, i, org, dir, tmin, ray_tmax, c.t, c.u, c.v)) continue;
            if (Leaf == LEAF_SPHERE && clip_t1) {
                if (!(c.t <= worst)) continue;                                 // (closest-hit's test: t0 <= min(exit, shortened tmax))
                c.u = pick_min(c.u, worst);
            }
            if (held.size() == a.k && !less(c, held.back())) continue;
            held.insert(std::upper_bound(held.begin(), held.end(), c, less), c);
            if (held.size() > a.k) held.pop_back();
            if (held.size() == a.k) worst = held.back().t;
        }
    }
    typename HitOf<T>::Type* const row = a.out_hits + qi * a.k;
    for (size_t j = 0; j < held.size(); ++j) store_hit(row + j, a.prim_ids ? a.prim_ids[held[j].i] : held[j].i, held[j].t, held[j].u, held[j].v);
    for (size_t j = held.size(); j < a.k; ++j) store_hit(row + j, BVH_AMD_INVALID, ray_tmax, T(0), T(0));
    if (a.counts) a.counts[qi] = uint32_t(held.size());
}

template <typename T>
RayNearestArgs<T> make_args(const void* pairs, uint32_t root_index, const void* prims, const void* rays, size_t first, size_t n, uint32_t k,
                            const uint32_t* order, const uint32_t* prim_ids, uint32_t deep_cap, void* out_hits, uint32_t* counts) {
    RayNearestArgs<T> a{};
    a.pairs = static_cast<const PairNode<T>*>(pairs); a.prims = static_cast<const T*>(prims); a.queries = static_cast<const T*>(rays);
    a.out_hits = static_cast<typename HitOf<T>::Type*>(out_hits); a.counts = counts; a.k = k;
    a.n = n; a.first = first; a.order = order; a.prim_ids = prim_ids; a.counters = nullptr;
    a.deep_cap = deep_cap; a.root_index = root_index;
    return a;
}

inline bool bad_shape(uint32_t k, uint32_t stride) { return k == 0 || k > BVH_AMD_RAY_NEAREST_MAX_K || stride == 0 || stride % 2 != 0; }

template <typename T, int Leaf, bool Robust>
int walk(int mutant, const void* pairs, uint32_t root_index, const void* prims, const void* rays, size_t n, uint32_t k, uint32_t stride,
         const uint32_t* order, const uint32_t* prim_ids, uint32_t deep_cap, int threads, void* out_hits, uint32_t* counts, unsigned long long* counters3) {
    if (bad_shape(k, stride)) return 1;
    const RayNearestArgs<T> a = make_args<T>(pairs, root_index, prims, rays, 0, n, k, order, prim_ids, deep_cap, out_hits, counts);
    if (mutant) {
        for (size_t s = 0; s < n; ++s) mutant_lane<T, Leaf, Robust>(a, order ? order[s] : s, mutant == 1, mutant == 2);
        counters3[0] = counters3[1] = counters3[2] = 0;
        return 0;
    }
    std::atomic<bool> lds_overrun{false};
    run_lanes(n, threads, counters3, [&](unsigned long long b, unsigned long long e, unsigned long long (&cnt)[3]) {
        const bool ok = deep_cap ? walk_range<T, Leaf, Robust, true>(a, stride, b, e, cnt) : walk_range<T, Leaf, Robust, false>(a, stride, b, e, cnt);
        if (!ok) lds_overrun = true;
    });
    return lds_overrun ? 2 : 0;
}

// One launch of a sliced batch as the device runs it (prelude: GuardedSpill, run_slice): both spill arrays sized for the launch's
// lanes, one block's LDS (`stride` lanes wide, between its sentinels) shared by the launch.
template <typename T, int Leaf, bool Robust>
long long walk_slice(const void* pairs, uint32_t root_index, const void* prims, const void* rays, size_t first, size_t n, size_t launch_lanes, uint32_t k,
                     uint32_t stride, const uint32_t* order, const uint32_t* prim_ids, uint32_t deep_cap, void* out_hits, uint32_t* counts,
                     unsigned long long* counters3) {
    if (bad_shape(k, stride) || deep_cap == 0 || n > launch_lanes) return kSliceBadArgs;
    RayNearestArgs<T> a = make_args<T>(pairs, root_index, prims, rays, first, n, k, order, prim_ids, deep_cap, out_hits, counts);
    GuardedSpill<uint32_t> deep_nodes(first, launch_lanes, deep_cap);
    GuardedSpill<T> deep_t(first, launch_lanes, deep_cap);
    a.deep_nodes = deep_nodes.data(); a.deep_t = deep_t.data();
    const size_t words = knn_lds_bytes<T>(k, stride) / 8;
    std::vector<unsigned long long> raw(words + 2 * kLdsGuardWords, kLdsSentinel);
    const KnnLds<T> lds = knn_lds_carve<T>(raw.data() + kLdsGuardWords, k, stride);
    run_slice(n, stride, counters3, [&](unsigned long long lane, int tid, unsigned long long (&cnt)[3]) {
        ray_nearest_lane<T, Leaf, Robust, true, true>(a, first + lane, lds, stride, tid, lane, cnt);
    });
    for (size_t w = 0; w < kLdsGuardWords; ++w)
        if (raw[w] != kLdsSentinel || raw[kLdsGuardWords + words + w] != kLdsSentinel) return kSliceGuardBroken;
    if (!deep_nodes.guards_intact() || !deep_t.guards_intact()) return kSliceGuardBroken;
    return deep_nodes.overwritten() + deep_t.overwritten();
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

// The kernel's walk for n rays {org, dir, tmin, tmax} (slot s reads ray order[s], or s), k records per row, the LDS arrays `stride`
// lanes wide; leaf 0 = triangles, 1 = spheres; robust = the robust node test; mutant 0 = the body, 1 / 2 = the wrong walks above (no
// counters); prim_ids (optional) = BVH_AMD_RAY_ORIGINAL_IDS; deep_cap > 0: the HBM spill of trees deeper than 64 levels, deep_cap
// entries. out_hits (n x k bvh_hit3f / bvh_hit3d records), counts (optional) as in the C ABI; counters3 = {pairs fetched, primitives
// tested, leaves visited}. Returns 0 (1: k or stride out of range; 2: a lane wrote outside the block's LDS).
int ray_nearest_host_walk(int is_double, int leaf, int robust, int mutant, const void* pairs, uint32_t root_index, const void* prims, const void* rays,
                          size_t n, uint32_t k, uint32_t stride, const uint32_t* order, const uint32_t* prim_ids, uint32_t deep_cap, int threads,
                          void* out_hits, uint32_t* counts, unsigned long long* counters3) {
    return pick(is_double, leaf, robust, [&]<typename T, int Leaf, bool Robust>() {
        return walk<T, Leaf, Robust>(mutant, pairs, root_index, prims, rays, n, k, stride, order, prim_ids, deep_cap, threads, out_hits, counts, counters3);
    });
}

// One launch of a batch that point_query_run cut into slices (deep_cap > 0): slots [first, first + n) as the device walks them —
// slot = first + lane, lane = 0 .. n-1 indexing spill arrays of launch_lanes * deep_cap entries, tid = lane % stride in one block's
// LDS. rays, order and the outputs are the whole batch's. Returns the spill entries the launch overwrote (both arrays), -1 if a guard
// zone around a spill array or the LDS was written to, -2 for arguments out of range (k, stride, deep_cap == 0, n > launch_lanes).
long long ray_nearest_host_walk_slice(int is_double, int leaf, int robust, const void* pairs, uint32_t root_index, const void* prims, const void* rays,
                                      size_t first, size_t n, size_t launch_lanes, uint32_t k, uint32_t stride, const uint32_t* order,
                                      const uint32_t* prim_ids, uint32_t deep_cap, void* out_hits, uint32_t* counts, unsigned long long* counters3) {
    return pick(is_double, leaf, robust, [&]<typename T, int Leaf, bool Robust>() {
        return walk_slice<T, Leaf, Robust>(pairs, root_index, prims, rays, first, n, launch_lanes, k, stride, order, prim_ids, deep_cap, out_hits, counts,
                                           counters3);
    });
}

} // extern "C"
