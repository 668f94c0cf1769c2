// Batched winding-number queries for gfx950 (bvh3X_winding_prepare / bvh3X_winding_numbers): is a point inside the mesh? The
// generalized winding number of a triangle mesh at each query point, evaluated hierarchically: a node far from the point (by beta
// radii) contributes the dipole of its summed area vector, a near leaf the exact solid angles of its triangles. The per-lane text is
// winding_body.inc (shared with the host test harness, tests/cpp/winding_body_host.cpp); the launch path of the walk is
// point_query.h's; this file holds the kernels and the host side of both calls.
//
// MI355X mapping:
//   * the moments (one row of 8 scalars per node, caller-owned): the parents pass of the refit (climb_parents.h), then ONE launch with a
//     lane per node: leaves fold their triangles and climb over arrival tickets, exactly as k_refit_prims does (build_common.h:
//     ticket_release / ticket_acquire; what climbers exchange goes through agent-scope relaxed atomics). An inner node is always
//     left + right, so the bytes do not depend on who arrived first. The tree is only read: topology and boxes come from the pair
//     records. Scratch: parent[], arrived[] and 4 scalars of s per node from the per-stream cache;
//   * the walk: one lane per query, one-shot grid of ceil(n / 256) blocks (no ticket counter: any number of launches of one const tree
//     may run at once), depth-first, left before right, nothing pruned; the moment rows of the two children of a pair record share
//     one aligned 16-scalar line and are read with 16-byte loads; the stack holds pair indices: kWindLds entries in LDS, the rest of
//     64 in per-lane scratch, beyond 64 (deep trees) in HBM (point_walk.inc);
//   * optionally the batch is read in the order of the Hilbert cell of each point in the root box (query_order.h). Outputs are always
//     in the caller's order.
//
// Compiled with -ffp-contract=off; division and sqrt are the correctly rounded forms, atan2 is arithmetic of the body (bit-identical to
// the host harness).

#include "build_common.h"
#include "climb_parents.h"
#include "trace_device.h"
#include "ray_key.h"
#include "query_order.h"

#define BVH_WIND_LOAD(ptr) __hip_atomic_load((ptr), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define BVH_WIND_STORE(ptr, v) __hip_atomic_store((ptr), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define BVH_WIND_ARRIVE(counter) winding_arrive(counter)

namespace bvh_amd {

namespace {
// this lane's rows and sums (sc1 stores) are acknowledged before the ticket is issued (refit_prims.hip: refit_arrive)
__device__ inline uint32_t winding_arrive(uint32_t* counter) {
    bld::ticket_release();
    const uint32_t before = atomicAdd(counter, 1u);
    bld::ticket_acquire();
    return before;
}
} // namespace

} // namespace bvh_amd

#include "winding_body.inc"
#include "point_query.h"

namespace bvh_amd {

namespace {

template <typename T>
__global__ void __launch_bounds__(256) k_winding_parents(const PairNode<T>* pairs, uint32_t root_index, uint32_t n, uint32_t* parent) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    climb_note_parent(wind_node_word(pairs, root_index, i), i, n, parent);
}

template <typename T>
__global__ void __launch_bounds__(256) k_winding_moments(const PairNode<T>* pairs, uint32_t root_index, const T* tris, size_t prim_total,
                                                         const uint32_t* parent, uint32_t* arrived, uint32_t n, T* moments, T* sums) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    wind_prepare_lane<T>(pairs, root_index, tris, prim_total, parent, arrived, n, moments, sums, i);
}

template <typename T, bool Stats, bool Deep>
__global__ void __launch_bounds__(kBlock) winding_kernel(WindingArgs<T> a) {
    __shared__ uint32_t lds_node[kWindLds * kBlock];
    const int tid = threadIdx.x;
    const unsigned long long lane = static_cast<unsigned long long>(blockIdx.x) * kBlock + tid;
    unsigned long long cnt[3] = {0, 0, 0};
    if (lane < a.n) winding_lane<T, Stats, Deep>(a, a.first + lane, lds_node, tid, lane, cnt);
    if (Stats) add_counters(a.counters, cnt, tid);
}

// What both calls check of the tree and the moments, in the order of the point queries' checks.
template <typename T>
int winding_check(const BvhImpl<T>& b, const void* d_tris12, const void* d_moments, size_t moments_rows, const std::string& who) {
    if (b.dim != 3) return fail(BVH_AMD_ERR_ARG, who + ": 3D trees only");
    if (!d_tris12 || !d_moments) return fail(BVH_AMD_ERR_ARG, who + ": null device pointer");
    if (misaligned(d_tris12, 16) || misaligned(d_moments, 16)) return fail(BVH_AMD_ERR_ARG, who + ": device pointers must be 16-byte aligned");
    if (b.node_count == 0 || !b.d_work || (b.pair_count && !b.d_pairs)) return fail(BVH_AMD_ERR_ARG, who + ": BVH has no device copy");
    if (moments_rows < b.node_count + 1)
        return fail(BVH_AMD_ERR_ARG, who + ": " + std::to_string(moments_rows) + " moment rows given, the tree needs node_count + 1 = " +
                                         std::to_string(b.node_count + 1));
    return BVH_AMD_OK;
}

} // namespace

template <typename T>
int launch_winding_prepare(const BvhImpl<T>& b, const T* d_tris12, T* d_moments, size_t moments_rows, hipStream_t stream) {
    if (const int rc = winding_check(b, d_tris12, d_moments, moments_rows, "winding_prepare")) return rc;
    StreamScope scratch_on(stream);
    const uint32_t n = static_cast<uint32_t>(b.node_count);
    bld::DevBuf<uint32_t> links;                              // parent[n], arrived[n]
    bld::DevBuf<T> sums;                                      // s of every node: {sx, sy, sz, -}
    BVH_HIP_TRY(links.alloc(size_t{2} * n), BVH_AMD_ERR_HIP);
    BVH_HIP_TRY(sums.alloc(size_t{4} * n), BVH_AMD_ERR_HIP);
    uint32_t *parent = links.p, *arrived = links.p + n;
    BVH_HIP_TRY(hipMemsetAsync(parent, 0xFF, size_t{n} * 4, stream), BVH_AMD_ERR_HIP);
    BVH_HIP_TRY(hipMemsetAsync(arrived, 0, size_t{n} * 4, stream), BVH_AMD_ERR_HIP);
    // (row 0 is zero, and so stay the rows of inner nodes nothing references: only in a tree that is not validated)
    BVH_HIP_TRY(hipMemsetAsync(d_moments, 0, (size_t{n} + 1) * kWindRow * sizeof(T), stream), BVH_AMD_ERR_HIP);
    const dim3 grid((n + 255) / 256), block(256);
    hipLaunchKernelGGL(k_winding_parents<T>, grid, block, 0, stream, b.d_pairs, b.root_index, n, parent);
    hipLaunchKernelGGL(k_winding_moments<T>, grid, block, 0, stream, b.d_pairs, b.root_index, d_tris12, b.prim_count, parent, arrived, n, d_moments,
                       sums.p);
    BVH_HIP_TRY(hipGetLastError(), BVH_AMD_ERR_HIP);
    return BVH_AMD_OK;
}

template <typename T>
int launch_winding(const BvhImpl<T>& b, const T* d_tris12, const T* d_moments, size_t moments_rows, const T* d_queries, size_t n, double beta,
                   unsigned flags, T* d_w, typename HitOf<T>::Type* d_hits, bvh_amd_counters* d_counters, hipStream_t stream) {
    const std::string who = "winding_numbers";
    if (!(beta >= 1.0)) return fail(BVH_AMD_ERR_ARG, who + ": beta must be at least 1 (+inf: the exact sum)");
    if (flags & ~(BVH_AMD_RAY_SORTED | BVH_AMD_RAY_UNSORTED)) return fail(BVH_AMD_ERR_ARG, who + ": unsupported flags (SORTED and UNSORTED only)");
    const char* fault = nullptr;
    if (n != 0) {
        if (!d_moments) fault = "null device pointer";
        else if (misaligned(d_tris12, 16) || misaligned(d_moments, 16) || misaligned(d_queries, 16) || misaligned(d_w, sizeof(T)) ||
                 misaligned(d_hits, 16) || misaligned(d_counters, 8))
            fault = "device pointers must be aligned (tris, moments, queries and hits 16 bytes, counters 8, w to its element)";
        else if (moments_rows < b.node_count + 1) fault = "too few moment rows: the tree needs node_count + 1";
    }
    if (const int rc = point_query_check(b, n, flags, d_tris12 && d_queries && d_w, fault, who); rc || n == 0) return rc;
    return point_query_run<T>(b, d_tris12, d_queries, n, flags, d_counters, sizeof(uint32_t), kBlock, kPointSortMin, kPointKeyBits, "winding_numbers", stream,
                              [&](const PointArgs<T>& args, T*) {
        const WindingArgs<T> a{args, d_moments, wind_beta2<T>(beta), d_w, d_hits};
        auto launch = [&](auto stats, auto deep) { return point_query_launch(winding_kernel<T, stats(), deep()>, a, kBlock, 0, stream); };
        return point_query_dispatch(LEAF_TRIANGLE, d_counters != nullptr, a.deep_cap != 0, [&](auto, auto stats, auto deep) { return launch(stats, deep); });
    });
}

template int launch_winding_prepare<float>(const BvhImpl<float>&, const float*, float*, size_t, hipStream_t);
template int launch_winding_prepare<double>(const BvhImpl<double>&, const double*, double*, size_t, hipStream_t);
template int launch_winding<float>(const BvhImpl<float>&, const float*, const float*, size_t, const float*, size_t, double, unsigned, float*, bvh_hit3f*,
                                   bvh_amd_counters*, hipStream_t);
template int launch_winding<double>(const BvhImpl<double>&, const double*, const double*, size_t, const double*, size_t, double, unsigned, double*, bvh_hit3d*,
                                    bvh_amd_counters*, hipStream_t);

} // namespace bvh_amd
