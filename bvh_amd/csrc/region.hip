// Batched convex-region queries for gfx950: for every query of m <= 8 planes {nx, ny, nz, d}, how many BVH-order primitives meet the
// intersection of the half-spaces ((nx*x + ny*y) + nz*z) + d <= 0 and, optionally, which ones and whether each lies wholly inside: a
// view or tile frustum, a sensor cone, a selection volume, a slab, a half-space. The primitives are the caller's arrays indexed by
// original primitive id (triangles: the 9 scalars bvh3X_refit_tris takes; spheres: {c, r}), read through the tree's prim ids. The
// per-lane body is region_body.inc (shared with the host test harness, tests/cpp/region_body_host.cpp): the planes and the node,
// triangle and sphere tests, handed to the walk radius.hip and overlap.hip use, list_walk.inc (stack, descent, counts, segments), over
// point_walk.inc (stack tiers, streaming stores); the launch path is point_query.h's.
//
// MI355X mapping (overlap.hip's, with plane values in place of interval tests):
//   * one lane per query, one-shot grid of ceil(n / 256) blocks: no ticket counter, so no work slot of the tree is claimed and any
//     number of launches of one const tree may run at once. One lane lists a region's whole output serially: the mapping is for
//     many regions (thousands of tile frusta), not for one huge one;
//   * a lane holds its planes in registers for the whole walk (4 m scalars; spheres: m lengths more). m is one number for the batch,
//     so the loops over the planes are unrolled over 8 and leave at a wave-uniform m: every plane has a constant register index;
//   * depth-first walk over the 64 / 128-byte pair records, left child first, the right one stacked as a bare node word when both
//     boxes pass the node test. Nothing is pruned against what was found;
//   * the stack: kRegionLds entries in LDS, the rest of 64 in per-lane scratch, beyond 64 (deep trees) in HBM (point_walk.inc);
//   * a leaf's primitives one at a time: prim id, then the 36 / 72 bytes of its triangle (16 / 32 of its sphere), 3 m (m) plane values;
//   * Exact is a template parameter: the CULL kernels carry neither the stored plane values nor the pair loop of region_exact;
//   * radius search's variable-length output: counts, segments [offsets[q], offsets[q + 1]), padding, plus one byte per entry for
//     "wholly inside" (the Fill = false kernels hold no list store and no offset load);
//   * the batch is never reordered: an unbounded region has no cell. Callers get coherence by submitting tiles in screen order.

#include "common.h"
#include "trace_device.h"
#include "ray_key.h"
#include "query_order.h"
#include "region_body.inc"
#include "point_query.h"

namespace bvh_amd {

namespace {

template <typename T, bool Stats, bool Deep, bool Fill, int Leaf, bool Exact>
__global__ void __launch_bounds__(kBlock) region_kernel(RegionArgs<T> a) {
    __shared__ uint32_t lds_node[kRegionLds * kBlock];
    const int tid = threadIdx.x;
    const unsigned long long lane = static_cast<unsigned long long>(blockIdx.x) * kBlock + tid;
    unsigned long long cnt[3] = {0, 0, 0};
    if (lane < a.n) region_lane<T, Stats, Deep, Fill, Leaf, Exact>(a, a.first + lane, lds_node, tid, lane, cnt);
    if (Stats) add_counters(a.counters, cnt, tid);
}

} // namespace

template <typename T>
int launch_region(const BvhImpl<T>& b, int leaf_kind, const T* d_prims, size_t n_prims, const T* d_planes, size_t m, size_t n, unsigned flags,
                  uint32_t* d_counts, const uint64_t* d_offsets, uint32_t* d_list_prims, uint8_t* d_list_inside, bvh_amd_counters* d_counters,
                  hipStream_t stream) {
    const bool tris = leaf_kind == LEAF_TRIANGLE;
    const char* who = tris ? "region_tris" : "region_spheres";
    if (flags & ~unsigned(BVH_AMD_RAY_ORIGINAL_IDS | BVH_AMD_REGION_EXACT))
        return fail(BVH_AMD_ERR_ARG, std::string(who) + ": unsupported flags (ORIGINAL_IDS and REGION_EXACT only: the batch is never reordered)");
    const bool exact = (flags & BVH_AMD_REGION_EXACT) != 0;
    if (exact && !tris) return fail(BVH_AMD_ERR_ARG, std::string(who) + ": REGION_EXACT is a triangle test (spheres have the plane-by-plane test only)");
    if (m < 1 || m > size_t(kRegionMaxPlanes)) return fail(BVH_AMD_ERR_ARG, std::string(who) + ": m = " + std::to_string(m) + " planes per query (1 .. 8)");
    const unsigned walk_flags = flags & ~unsigned(BVH_AMD_REGION_EXACT);         // what the shared launch path knows
    const bool aligned = !(misaligned(d_prims, sizeof(T)) || misaligned(d_planes, sizeof(T)) || misaligned(d_offsets, 8) || misaligned(d_counters, 8) ||
                           misaligned(d_counts, 4) || misaligned(d_list_prims, 4));
    const char* fault = list_output_fault(d_counts, d_offsets, d_list_prims, d_list_inside);
    if (!fault && !aligned) fault = "device pointers must be aligned (primitives and planes to their scalar, offsets and counters 8 bytes, counts and list prims 4)";
    if (const int rc = point_query_check(b, n, walk_flags, d_prims && d_planes, fault, who); rc || n == 0) return rc;
    if (const int rc = source_array_check(b, n_prims, "primitives", who, stream)) return rc;
    return point_query_run<T>(b, d_prims, d_planes, n, walk_flags | BVH_AMD_RAY_UNSORTED, d_counters, sizeof(uint32_t), kBlock, kPointSortMin, kPointKeyBits, who,
                              stream, [&](const PointArgs<T>& args, T*) {
        const RegionArgs<T> a{{args, d_counts, reinterpret_cast<const unsigned long long*>(d_offsets), d_list_prims}, b.d_prim_ids, d_list_inside,
                              static_cast<uint32_t>(m)};
        return list_query_dispatch(leaf_kind, d_counters != nullptr, a.deep_cap != 0, a.offsets != nullptr, [&](auto leaf, auto stats, auto deep, auto fill) {
            if constexpr (leaf() == LEAF_TRIANGLE) {
                if (exact) return point_query_launch(region_kernel<T, stats(), deep(), fill(), LEAF_TRIANGLE, true>, a, kBlock, 0, stream);
            }
            return point_query_launch(region_kernel<T, stats(), deep(), fill(), leaf(), false>, a, kBlock, 0, stream);
        });
    });
}

template int launch_region<float>(const BvhImpl<float>&, int, const float*, size_t, const float*, size_t, size_t, unsigned, uint32_t*, const uint64_t*, uint32_t*,
                                  uint8_t*, bvh_amd_counters*, hipStream_t);
template int launch_region<double>(const BvhImpl<double>&, int, const double*, size_t, const double*, size_t, size_t, unsigned, uint32_t*, const uint64_t*,
                                   uint32_t*, uint8_t*, bvh_amd_counters*, hipStream_t);

} // namespace bvh_amd
