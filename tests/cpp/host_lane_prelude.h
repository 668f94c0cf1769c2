// TEST INFRASTRUCTURE (CPU, no GPU): what the host harnesses of the one-lane-per-query kinds (closest_body_host.cpp,
// radius_body_host.cpp, knn_body_host.cpp, overlap_body_host.cpp, tri_intersect_body_host.cpp, tri_distance_body_host.cpp,
// region_body_host.cpp, winding_body_host.cpp, ray_hits_body_host.cpp, ray_nearest_body_host.cpp, sphere_cast_body_host.cpp,
// instanced_body_host.cpp; every *_body_host.cpp but trace_body_host.cpp and refit_body_host.cpp) put in front of the kernels' text:
// single-lane stand-ins for hip_runtime.h and for bvh_amd/csrc/common.h, then the device helpers of bvh_amd/csrc/trace_device.h, the
// thread-split scaffold of their walks, and the emulation of one launch of a sliced batch over a deep tree. The stand-ins must follow
// common.h (PairNode, kCountBits, LEAF_*).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/bvh_amd.h"                               // bvh_hit3f / bvh_hit3d, bvh_amd_counters, BVH_AMD_INVALID

// ---- single-lane stand-ins for what hip_runtime.h provides ------------------------------------------------------------
#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static

struct float2 { float x, y; };
struct float4 { float x, y, z, w; };
struct double2 { double x, y; };
struct uint2 { uint32_t x, y; };
struct uint4 { uint32_t x, y, z, w; };
inline float4 make_float4(float x, float y, float z, float w) { return {x, y, z, w}; }
inline double2 make_double2(double x, double y) { return {x, y}; }
inline uint32_t __float_as_uint(float x) { return __builtin_bit_cast(uint32_t, x); }
inline float __uint_as_float(uint32_t x) { return __builtin_bit_cast(float, x); }
inline long long __double_as_longlong(double x) { return __builtin_bit_cast(long long, x); }
inline double __longlong_as_double(long long x) { return __builtin_bit_cast(double, x); }
using std::min;

// ---- stand-ins for bvh_amd/csrc/common.h (which needs the HIP headers) ------------------------------------------------------
namespace bvh_amd {
constexpr unsigned kCountBits = 4;
constexpr uint32_t kCountMask = 15u;
constexpr int kWave = 64;
template <typename T> struct PairNode;
template <> struct PairNode<float> { float lb[6], rb[6]; uint32_t li, ri; uint32_t pad[2]; };
template <> struct PairNode<double> { double lb[6], rb[6]; uint32_t li, ri; uint32_t pad[6]; };
template <typename T> struct HitOf;
template <> struct HitOf<float> { using Type = bvh_hit3f; };
template <> struct HitOf<double> { using Type = bvh_hit3d; };
enum { LEAF_TRIANGLE = 0, LEAF_SPHERE = 1 };
} // namespace bvh_amd

#include "../../bvh_amd/csrc/trace_device.h"

// ---- the scaffold of a harness's walk: slots [0, n) split over `threads` host threads, range(begin, end, cnt) on each (it walks its
// slots one emulated lane at a time and adds to its own cnt), counters3 = the sum of the threads' cnt -----------------------------------
template <typename Range>
void run_lanes(size_t n, int threads, unsigned long long* counters3, Range range) {
    const int nt = std::max(1, threads);
    std::vector<std::thread> pool;
    std::vector<unsigned long long> sums(3 * size_t(nt), 0);
    for (int t = 0; t < nt; ++t) {
        const unsigned long long b = n * t / nt, e = n * (t + 1) / nt;
        pool.emplace_back([&, t, b, e] {
            unsigned long long cnt[3] = {0, 0, 0};
            range(b, e, cnt);
            for (int k = 0; k < 3; ++k) sums[3 * size_t(t) + k] = cnt[k];
        });
    }
    for (auto& th : pool) th.join();
    for (int k = 0; k < 3; ++k) { counters3[k] = 0; for (int t = 0; t < nt; ++t) counters3[k] += sums[3 * size_t(t) + k]; }
}

// ---- one emulated launch of a sliced batch (point_query.h, point_query_run: a tree deeper than 64 levels, slots [first, first + n) of
// the batch, the HBM spill sized for the launch's lanes and shared by them) ----------------------------------------------------------
// An HBM spill array of `entries` elements between two guard zones, every byte kSpillByte before the walk. The zone behind it is long
// enough for a lane that indexed the spill by its SLOT, or a spill sized for one lane only, to land in the zone and not in foreign
// memory: (first + launch_lanes) * deep_cap entries and kSpillGuard more.
constexpr size_t kSpillGuard = 64;
constexpr unsigned char kSpillByte = 0xC3;                     // (0xC3C3C3C3: as a node word a leaf at primitive 2 * 10^8, as a distance negative: neither is ever pushed)

template <typename V>
class GuardedSpill {
public:
    GuardedSpill(size_t first, size_t launch_lanes, size_t deep_cap)
        : entries_(launch_lanes * deep_cap), bytes_((kSpillGuard + launch_lanes * deep_cap + (first + launch_lanes) * deep_cap + kSpillGuard) * sizeof(V), kSpillByte) {}
    V* data() { return reinterpret_cast<V*>(bytes_.data()) + kSpillGuard; }
    bool guards_intact() const {
        const size_t lo = kSpillGuard * sizeof(V), hi = (kSpillGuard + entries_) * sizeof(V);
        for (size_t i = 0; i < lo; ++i) if (bytes_[i] != kSpillByte) return false;
        for (size_t i = hi; i < bytes_.size(); ++i) if (bytes_[i] != kSpillByte) return false;
        return true;
    }
    // entries of the spill the launch wrote to
    long long overwritten() const {
        long long count = 0;
        for (size_t e = 0; e < entries_; ++e) {
            const unsigned char* p = bytes_.data() + (kSpillGuard + e) * sizeof(V);
            bool touched = false;
            for (size_t i = 0; i < sizeof(V); ++i) touched |= p[i] != kSpillByte;
            count += touched;
        }
        return count;
    }
private:
    size_t entries_;
    std::vector<unsigned char> bytes_;
};

// The lanes 0 .. n-1 of the launch, one after the other as the device numbers them: lane_fn(lane, tid = lane % block, cnt) walks slot
// first + lane with the spill index `lane` and the LDS column `tid` of one LDS stand-in shared by the launch; counters3 = their sum.
template <typename Lane>
void run_slice(size_t n, unsigned block, unsigned long long* counters3, Lane lane_fn) {
    unsigned long long cnt[3] = {0, 0, 0};
    for (unsigned long long lane = 0; lane < n; ++lane) lane_fn(lane, int(lane % block), cnt);
    for (int k = 0; k < 3; ++k) counters3[k] = cnt[k];
}

// What a slice entry returns: the spill entries the launch overwrote (>= 0), or one of these.
constexpr long long kSliceGuardBroken = -1;                   // a guard zone of the spill (or of the LDS stand-in) was written to
constexpr long long kSliceBadArgs = -2;                       // deep_cap == 0, n > launch_lanes, ...
