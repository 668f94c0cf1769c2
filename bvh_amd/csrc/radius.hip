// Batched radius queries for gfx950: for every query point {x, y, z, max_distance}, how many BVH-order primitives (PrecomputedTri or
// Sphere<T, 3>) lie within max_distance of it and, optionally, which ones, at what distance. The per-lane body is radius_body.inc
// (shared with the host test harness, tests/cpp/radius_body_host.cpp): the query and its tests, handed to the walk of the list
// queries, list_walk.inc (stack, descent, counts, segments; shared with overlap.hip), over point_walk.inc (distance functions, stack
// tiers); the launch path is point_query.h's; this file holds the kernel, what is specific to the query, and the offsets scan.
//
// MI355X mapping:
//   * one lane per query, one-shot grid of ceil(n / 256) blocks: no ticket counter, so no work slot of the tree is claimed and any
//     number of launches of one const tree may run at once;
//   * depth-first walk over the 64 / 128-byte pair records (common.h: PairNode), left child first, the right one stacked as a bare node
//     word when both boxes are within the radius. Nothing is pruned against what was found: the list of a query is fixed by the tree;
//   * the stack: kRadiusLds entries in LDS, the rest of 64 in per-lane scratch, beyond 64 (deep trees) in HBM (point_walk.inc);
//   * variable-length output without a second walk inside the kernel: a query writes into [offsets[q], offsets[q + 1]) of the list
//     arrays, never past it, pads what it does not use and reports its untruncated count. Count pass (no offsets: the Fill = false
//     kernels hold no list store and no offset load), bvh_amd_offsets_from_counts, fill pass give exact lists; fixed-size segments
//     give one pass with an overflow indication;
//   * optionally the batch is read in the order of the Hilbert cell of each point in the root box (query_order.h): neighbouring lanes
//     then walk the same records. Outputs are always in the caller's order.
//
// Compiled with -ffp-contract=off; division and sqrt are the correctly rounded forms (bit-identical to the host harness).

#include "common.h"
#include "trace_device.h"
#include "ray_key.h"
#include "query_order.h"
#include "radius_body.inc"
#include "point_query.h"

namespace bvh_amd {

namespace {

template <typename T, int Leaf, bool Stats, bool Deep, bool Fill>
__global__ void __launch_bounds__(kBlock) radius_kernel(RadiusArgs<T> a) {
    __shared__ uint32_t lds_node[kRadiusLds * kBlock];
    const int tid = threadIdx.x;
    const unsigned long long lane = static_cast<unsigned long long>(blockIdx.x) * kBlock + tid;
    unsigned long long cnt[3] = {0, 0, 0};
    if (lane < a.n) radius_lane<T, Leaf, Stats, Deep, Fill>(a, a.first + lane, lds_node, tid, lane, cnt);
    if (Stats) add_counters(a.counters, cnt, tid);
}

// ---- offsets[0..n] = exclusive sums of counts[0..n), 64-bit, in stream order ----------------------------------------------------
// Blocks of 4096 counts: their sums, one block that scans the sums in place, then every block scans its own counts from its base.
constexpr int kOffsetsBlock = 4096;

__device__ inline unsigned long long block_inclusive_scan(unsigned long long* part, unsigned long long v) {
    part[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const unsigned long long o = threadIdx.x >= unsigned(off) ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += o;
        __syncthreads();
    }
    return part[threadIdx.x];
}

__global__ void __launch_bounds__(1024) offsets_block_sums_kernel(const uint32_t* counts, unsigned long long n, unsigned long long* sums) {
    __shared__ unsigned long long part[1024];
    const unsigned long long base = static_cast<unsigned long long>(blockIdx.x) * kOffsetsBlock + threadIdx.x * 4ull;
    unsigned long long s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) s += base + k < n ? counts[base + k] : 0u;
    block_inclusive_scan(part, s);
    if (threadIdx.x == 1023) sums[blockIdx.x] = part[1023];
}

__global__ void __launch_bounds__(1024) offsets_scan_sums_kernel(unsigned long long* sums, unsigned long long m) {
    __shared__ unsigned long long part[1024];
    unsigned long long carry = 0;
    for (unsigned long long base = 0; base < m; base += 1024) {
        const unsigned long long i = base + threadIdx.x;
        const unsigned long long v = i < m ? sums[i] : 0;
        const unsigned long long incl = block_inclusive_scan(part, v);
        if (i < m) sums[i] = carry + incl - v;
        carry += part[1023];
        __syncthreads();                                      // (part is rewritten by the next round)
    }
}

__global__ void __launch_bounds__(1024) offsets_write_kernel(const uint32_t* counts, unsigned long long n, const unsigned long long* bases,
                                                             unsigned long long* offsets) {
    __shared__ unsigned long long part[1024];
    const unsigned long long base = static_cast<unsigned long long>(blockIdx.x) * kOffsetsBlock + threadIdx.x * 4ull;
    uint32_t v[4];
    unsigned long long s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = base + k < n ? counts[base + k] : 0u; s += v[k]; }
    unsigned long long run = (bases ? bases[blockIdx.x] : 0ull) + block_inclusive_scan(part, s) - s;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (base + k < n) offsets[base + k] = run;
        run += v[k];
        if (base + k + 1 == n) offsets[n] = run;
    }
}

} // namespace

int offsets_from_counts(const uint32_t* d_counts, size_t n, uint64_t* d_offsets, hipStream_t stream) {
    if (!d_offsets || (n && !d_counts)) return fail(BVH_AMD_ERR_ARG, "offsets_from_counts: null device pointer");
    if (misaligned(d_counts, 4) || misaligned(d_offsets, 8)) return fail(BVH_AMD_ERR_ARG, "offsets_from_counts: counts must be 4-byte aligned, offsets 8-byte");
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long));
    unsigned long long* offsets = reinterpret_cast<unsigned long long*>(d_offsets);
    if (n == 0) { BVH_HIP_TRY(hipMemsetAsync(d_offsets, 0, sizeof(uint64_t), stream), BVH_AMD_ERR_HIP); return BVH_AMD_OK; }
    const unsigned long long blocks = (n + kOffsetsBlock - 1) / kOffsetsBlock;
    if (blocks > 0x7FFFFFFFull) return fail(BVH_AMD_ERR_ARG, "offsets_from_counts: more than 2^43 counts");
    StreamScope scope(stream);
    void* mem = nullptr;
    ScratchTag tag;
    if (blocks > 1) {
        const hipError_t e = scratch_alloc(&mem, blocks * sizeof(unsigned long long), &tag);
        if (e != hipSuccess) return fail(BVH_AMD_ERR_HIP, std::string("offsets_from_counts: no scratch for the block sums: ") + hipGetErrorString(e));
        unsigned long long* sums = static_cast<unsigned long long*>(mem);
        hipLaunchKernelGGL(offsets_block_sums_kernel, dim3(static_cast<unsigned>(blocks)), dim3(1024), 0, stream, d_counts, n, sums);
        hipLaunchKernelGGL(offsets_scan_sums_kernel, dim3(1), dim3(1024), 0, stream, sums, blocks);
    }
    hipLaunchKernelGGL(offsets_write_kernel, dim3(static_cast<unsigned>(blocks)), dim3(1024), 0, stream, d_counts, n,
                       static_cast<const unsigned long long*>(mem), offsets);
    const hipError_t e = hipGetLastError();
    if (mem) scratch_free(mem, tag);
    BVH_HIP_TRY(e, BVH_AMD_ERR_HIP);
    return BVH_AMD_OK;
}

template <typename T>
int launch_radius(const BvhImpl<T>& b, int leaf_kind, const T* d_prims, const T* d_queries, size_t n, unsigned flags, uint32_t* d_counts,
                  const uint64_t* d_offsets, uint32_t* d_list_prims, T* d_list_dist, bvh_amd_counters* d_counters, hipStream_t stream) {
    const bool aligned = !(misaligned(d_prims, 16) || misaligned(d_queries, 16) || misaligned(d_offsets, 8) || misaligned(d_counters, 8) ||
                           misaligned(d_counts, 4) || misaligned(d_list_prims, 4) || misaligned(d_list_dist, sizeof(T)));
    const char* fault = list_output_fault(d_counts, d_offsets, d_list_prims, d_list_dist);
    if (!fault && !aligned) fault = "device pointers must be aligned (prims and queries 16 bytes, offsets and counters 8, "
                                    "counts, list prims and list distances to their element)";
    if (const int rc = point_query_check(b, n, flags, d_prims && d_queries, fault, "radius_search"); rc || n == 0) return rc;
    return point_query_run<T>(b, d_prims, d_queries, n, flags, d_counters, sizeof(uint32_t), kBlock, kPointSortMin, kPointKeyBits, "radius_search", stream,
                              [&](const PointArgs<T>& args, T*) {
        const RadiusArgs<T> a{{args, d_counts, reinterpret_cast<const unsigned long long*>(d_offsets), d_list_prims}, d_list_dist};
        return list_query_dispatch(leaf_kind, d_counters != nullptr, a.deep_cap != 0, a.offsets != nullptr, [&](auto leaf, auto stats, auto deep, auto fill) {
            return point_query_launch(radius_kernel<T, leaf(), stats(), deep(), fill()>, a, kBlock, 0, stream);
        });
    });
}

template int launch_radius<float>(const BvhImpl<float>&, int, const float*, const float*, size_t, unsigned, uint32_t*, const uint64_t*, uint32_t*, float*,
                                  bvh_amd_counters*, hipStream_t);
template int launch_radius<double>(const BvhImpl<double>&, int, const double*, const double*, size_t, unsigned, uint32_t*, const uint64_t*, uint32_t*, double*,
                                   bvh_amd_counters*, hipStream_t);

} // namespace bvh_amd
