// TEST INFRASTRUCTURE (CPU, no GPU): compiles the text of the winding-number kernels — bvh_amd/csrc/winding_body.inc (atan2, the solid
// angle, the leaf fold and ticket climb of the moments, the walk) over point_walk.inc, with the device helpers of
// bvh_amd/csrc/trace_device.h — for the HOST and runs it with one emulated lane per query / per node. What it can show: the arithmetic
// of the very source the device runs (atan2 against libm, moments against a float64 restatement, the walk against a brute-force sum),
// and that the climb's bytes do not depend on the order or the interleaving of its lanes; the device's moments, winding numbers and
// counters must equal these bit for bit. What it cannot show: the hand-off between workgroups (tests/test_gpu_winding.py).
// tests/test_winding_host.py drives it; tests/test_gpu_winding.py uses it too.
//
// Built by the tests with: g++ -std=c++20 -O1 -mavx2 -mfma -ffp-contract=off -fno-strict-aliasing -shared -fPIC -pthread.
#include "host_lane_prelude.h"

// The climb's hooks: lanes on several host threads hand a node over through the ticket (an acquire-release increment), as the device's
// do through its wait and atomic add.
#define BVH_WIND_LOAD(ptr) (*(ptr))
#define BVH_WIND_STORE(ptr, v) (*(ptr) = (v))
#define BVH_WIND_ARRIVE(counter) __atomic_fetch_add((counter), 1u, __ATOMIC_ACQ_REL)

#include "../../bvh_amd/csrc/climb_parents.h"
#include "../../bvh_amd/csrc/winding_body.inc"

namespace {

using namespace bvh_amd;

// winding.hip: launch_winding_prepare (the memsets, k_winding_parents, k_winding_moments with lane i = lanes[k] or k)
template <typename T>
int prepare(const void* pairs_, uint32_t root_index, uint32_t n, const void* tris, size_t prim_total, const uint32_t* lanes, int threads, void* moments_,
            void* sums_) {
    auto pairs = static_cast<const PairNode<T>*>(pairs_);
    T* moments = static_cast<T*>(moments_);
    std::vector<T> own_sums(sums_ ? 0 : size_t(4) * n);
    T* sums = sums_ ? static_cast<T*>(sums_) : own_sums.data();
    std::memset(moments, 0, (size_t(n) + 1) * kWindRow * sizeof(T));
    std::vector<uint32_t> parent(n, 0xFFFFFFFFu), arrived(n, 0u);
    for (uint32_t i = 0; i < n; ++i) climb_note_parent(wind_node_word(pairs, root_index, i), i, n, parent.data());   // k_winding_parents
    const int nt = std::max(1, threads);
    std::vector<std::thread> pool;
    for (int t = 0; t < nt; ++t) {
        pool.emplace_back([&, t] {
            for (size_t k = t; k < n; k += nt)                                   // interleaved: neighbours climb at the same time
                wind_prepare_lane<T>(pairs, root_index, static_cast<const T*>(tris), prim_total, parent.data(), arrived.data(), n, moments, sums,
                                     lanes ? lanes[k] : uint32_t(k));
        });
    }
    for (auto& th : pool) th.join();
    return 0;
}

template <typename T, bool Deep>
void walk_range(const WindingArgs<T>& a0, unsigned long long begin, unsigned long long end, unsigned long long (&cnt)[3]) {
    WindingArgs<T> a = a0;
    std::vector<uint32_t> lds_node(size_t(kWindLds) * kBlock);
    std::vector<uint32_t> deep_nodes(Deep ? a.deep_cap : 1);
    a.deep_nodes = deep_nodes.data();                                        // one lane at a time: lane 0's spill
    for (unsigned long long s = begin; s < end; ++s) winding_lane<T, true, Deep>(a, s, lds_node.data(), 0, 0, cnt);
}

template <typename T>
int walk(const void* pairs, uint32_t root_index, const void* tris, const void* moments, const void* queries, size_t n, const uint32_t* order, double beta,
         uint32_t deep_cap, int threads, void* w, void* hits, unsigned long long* counters3) {
    WindingArgs<T> a{};
    a.pairs = static_cast<const PairNode<T>*>(pairs); a.prims = static_cast<const T*>(tris); a.queries = static_cast<const T*>(queries);
    a.n = n; a.first = 0; a.order = order; a.prim_ids = nullptr; a.counters = nullptr;
    a.deep_cap = deep_cap; a.root_index = root_index;
    a.moments = static_cast<const T*>(moments); a.beta2 = wind_beta2<T>(beta); a.w = static_cast<T*>(w);
    a.hits = static_cast<typename HitOf<T>::Type*>(hits);
    run_lanes(n, threads, counters3, [&](unsigned long long b, unsigned long long e, unsigned long long (&cnt)[3]) {
        if (deep_cap) walk_range<T, true>(a, b, e, cnt); else walk_range<T, false>(a, b, e, cnt);
    });
    return 0;
}

template <typename T>
void atan2_n(const void* y_, const void* x_, size_t n, void* out_) {
    auto y = static_cast<const T*>(y_); auto x = static_cast<const T*>(x_); auto out = static_cast<T*>(out_);
    for (size_t i = 0; i < n; ++i) out[i] = wind_atan2<T>(y[i], x[i]);
}

template <typename T>
void solid_angle_n(const void* pre_, const void* q_, size_t n, void* out_) {
    auto pre = static_cast<const T*>(pre_); auto q = static_cast<const T*>(q_); auto out = static_cast<T*>(out_);
    for (size_t i = 0; i < n; ++i) {
        T p[12], qq[3];
        std::memcpy(p, pre + 12 * i, sizeof(p));
        std::memcpy(qq, q + 3 * i, sizeof(qq));
        out[i] = wind_solid_angle<T>(p, qq);
    }
}

} // namespace

extern "C" {

// out[i] = the body's atan2(y[i], x[i])
void winding_host_atan2(int is_double, const void* y, const void* x, size_t n, void* out) {
    if (is_double) atan2_n<double>(y, x, n, out); else atan2_n<float>(y, x, n, out);
}

// out[i] = the body's signed solid angle of PrecomputedTri pre12[i] seen from q3[i]
void winding_host_solid_angle(int is_double, const void* pre12, const void* q3, size_t n, void* out) {
    if (is_double) solid_angle_n<double>(pre12, q3, n, out); else solid_angle_n<float>(pre12, q3, n, out);
}

// The moments of a tree of n nodes given as its (n - 1) / 2 pair records and root index word: moments = (n + 1) x 8 scalars, sums
// (optional) = n x 4 {sx, sy, sz, -}. lanes (optional) = the order in which the n lanes are started; threads > 1: lane k of that order
// runs on thread k % threads.
int winding_host_prepare(int is_double, const void* pairs, uint32_t root_index, uint32_t n, const void* tris12, size_t prim_total, const uint32_t* lanes,
                         int threads, void* moments, void* sums) {
    return is_double ? prepare<double>(pairs, root_index, n, tris12, prim_total, lanes, threads, moments, sums)
                     : prepare<float>(pairs, root_index, n, tris12, prim_total, lanes, threads, moments, sums);
}

// The kernel's walk for n queries {x, y, z, -} (slot s reads query order[s], or s); deep_cap > 0: the HBM spill of trees deeper than
// 64 levels, deep_cap entries. w = n scalars; hits (optional) = closest_points' records, t negated where w >= 1/2; counters3 = {pair
// records opened, triangles summed exactly, far terms added}. Returns 0.
int winding_host_walk(int is_double, const void* pairs, uint32_t root_index, const void* tris12, const void* moments, const void* queries, size_t n,
                      const uint32_t* order, double beta, uint32_t deep_cap, int threads, void* w, void* hits, unsigned long long* counters3) {
    return is_double ? walk<double>(pairs, root_index, tris12, moments, queries, n, order, beta, deep_cap, threads, w, hits, counters3)
                     : walk<float>(pairs, root_index, tris12, moments, queries, n, order, beta, deep_cap, threads, w, hits, counters3);
}

} // extern "C"
