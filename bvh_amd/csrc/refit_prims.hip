// Refit of a resident tree from moved primitives (bvhXX_refit_boxes, bvh3X_refit_tris): what a user of the reference writes as
//   bvh.refit([&](Node& leaf) { box = BBox::make_empty(); for (i in leaf) box.extend(bboxes[prim_ids[i]]); leaf.set_bbox(box); })
// (bvh.h:211-218), with the primitives, the reference-layout nodes and the traversal records all in HBM. One launch does the leaf fold,
// the bottom-up climb over arrival tickets (build_common.h: ticket_release / ticket_acquire) and the update of BOTH representations in
// place: the lane that completes a node stores its box into d_nodes[c] and into its half of d_pairs[(c - 1) / 2]. No host copy, no
// synchronisation, no allocation beyond two words per node from the per-stream scratch cache. The text of the fold, the record-half
// store and the climb is refit_body.inc, which a CPU test compiles for the host.
#include "build_common.h"
#include "climb_parents.h"

namespace bvh_amd {

using namespace bld;

#define BVH_REFIT_LOAD(ptr) __hip_atomic_load((ptr), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define BVH_REFIT_STORE(ptr, v) __hip_atomic_store((ptr), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define BVH_REFIT_ARRIVE(counter) refit_arrive(counter)

namespace {
// this lane's boxes (sc1 stores) and record halves are acknowledged before the ticket is issued; tests/test_refit_prims_host.py
// reads the ISA for the wait
__device__ inline uint32_t refit_arrive(uint32_t* counter) {
    ticket_release();
    const uint32_t before = atomicAdd(counter, 1u);
    ticket_acquire();
    return before;
}
} // namespace

} // namespace bvh_amd

#include "refit_body.inc"

namespace bvh_amd {

namespace {

// compute_parents (reinsertion_optimizer.h:72-86) over a parent[] pre-filled with 0xFFFFFFFF: the root and the top of a subtree
// nothing references keep that mark (climb_parents.h: shared with the moments climb of winding.hip)
template <typename T>
__global__ void __launch_bounds__(256) k_refit_parents(const HostNode<T>* nodes, uint32_t n, uint32_t* parent) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    climb_note_parent(nodes[i].index, i, n, parent);
}

template <typename T, int Src>
__global__ void __launch_bounds__(256) k_refit_prims(HostNode<T>* nodes, PairNode<T>* pairs, const uint32_t* parent, uint32_t* arrived, uint32_t n,
                                                     const T* src, size_t n_src, const uint32_t* prim_ids, size_t prim_total) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    refit_lane<T, Src>(nodes, pairs, parent, arrived, n, src, n_src, prim_ids, prim_total, i);
}

__global__ void __launch_bounds__(256) k_max_u32(const uint32_t* v, size_t n, uint32_t* out) {
    uint32_t mine = 0;
    for (size_t i = blockIdx.x * size_t{256} + threadIdx.x; i < n; i += size_t{gridDim.x} * 256) mine = max(mine, v[i]);
    for (int off = 32; off > 0; off >>= 1) mine = max(mine, static_cast<uint32_t>(__shfl_down(mine, off)));
    if ((threadIdx.x & 63) == 0) atomicMax(out, mine);
}

} // namespace

// The largest value in d_prim_ids (one read-back; largest_prim_id below, its only caller, caches it per tree).
int max_prim_id_device(const uint32_t* d_prim_ids, size_t prim_count, hipStream_t stream, uint32_t* out) {
    *out = 0;
    if (prim_count == 0) return BVH_AMD_OK;
    StreamScope scratch_on(stream);
    DevBuf<uint32_t> word;
    BVH_HIP_TRY(word.alloc(1), BVH_AMD_ERR_HIP);
    BVH_HIP_TRY(hipMemsetAsync(word.p, 0, 4, stream), BVH_AMD_ERR_HIP);
    const unsigned grid = static_cast<unsigned>(std::min<size_t>((prim_count + 255) / 256, 1024));
    hipLaunchKernelGGL(k_max_u32, dim3(grid), dim3(256), 0, stream, d_prim_ids, prim_count, word.p);
    BVH_HIP_TRY(hipGetLastError(), BVH_AMD_ERR_HIP);
    BVH_HIP_TRY(hipMemcpyAsync(out, word.p, 4, hipMemcpyDeviceToHost, stream), BVH_AMD_ERR_HIP);
    BVH_HIP_TRY(hipStreamSynchronize(stream), BVH_AMD_ERR_HIP);
    return BVH_AMD_OK;
}

template <typename T>
int largest_prim_id(const BvhImpl<T>& b, hipStream_t stream, long long* out) {
    long long largest = b.max_prim_id.load();
    if (largest < 0) {
        uint32_t found = 0;
        if (const int rc = max_prim_id_device(b.d_prim_ids, b.prim_count, stream, &found)) return rc;
        b.max_prim_id = largest = found;
    }
    *out = largest;
    return BVH_AMD_OK;
}

template <typename T>
int source_array_check(const BvhImpl<T>& b, size_t n_src, const char* noun, const std::string& who, hipStream_t stream) {
    if (!b.d_prim_ids) return fail(BVH_AMD_ERR_ARG, who + ": BVH has no device prim ids");
    long long largest = 0;
    if (const int rc = largest_prim_id(b, stream, &largest)) return rc;
    if (b.prim_count && n_src <= static_cast<size_t>(largest))
        return fail(BVH_AMD_ERR_ARG, who + ": " + std::to_string(n_src) + " " + noun + " given, but prim_ids refers to primitive " +
                    std::to_string(largest) + " (the array is indexed by original primitive id)");
    return BVH_AMD_OK;
}

template int largest_prim_id<float>(const BvhImpl<float>&, hipStream_t, long long*);
template int largest_prim_id<double>(const BvhImpl<double>&, hipStream_t, long long*);
template int source_array_check<float>(const BvhImpl<float>&, size_t, const char*, const std::string&, hipStream_t);
template int source_array_check<double>(const BvhImpl<double>&, size_t, const char*, const std::string&, hipStream_t);

// Leaf boxes from `d_src` (src_kind: REFIT_BOXES3 / REFIT_BOXES2 / REFIT_TRIS), inner boxes bottom-up, both representations in place.
// Asynchronous on `stream`. (dimension-independent above the leaves: z stays (+0, +0) in 2D)
template <typename T>
int refit_prims_device(HostNode<T>* d_nodes, PairNode<T>* d_pairs, size_t node_count, int src_kind, const T* d_src, size_t n_src,
                       const uint32_t* d_prim_ids, size_t prim_count, hipStream_t stream) {
    StreamScope scratch_on(stream);
    const uint32_t n = static_cast<uint32_t>(node_count);
    if (n == 0) return BVH_AMD_OK;
    DevBuf<uint32_t> links;                                   // parent[n], arrived[n]
    BVH_HIP_TRY(links.alloc(size_t{2} * n), BVH_AMD_ERR_HIP);
    uint32_t *parent = links.p, *arrived = links.p + n;
    BVH_HIP_TRY(hipMemsetAsync(parent, 0xFF, size_t{n} * 4, stream), BVH_AMD_ERR_HIP);
    BVH_HIP_TRY(hipMemsetAsync(arrived, 0, size_t{n} * 4, stream), BVH_AMD_ERR_HIP);
    const dim3 grid((n + 255) / 256), block(256);
    hipLaunchKernelGGL(k_refit_parents<T>, grid, block, 0, stream, d_nodes, n, parent);
    switch (src_kind) {
    case REFIT_BOXES3:
        hipLaunchKernelGGL((k_refit_prims<T, REFIT_BOXES3>), grid, block, 0, stream, d_nodes, d_pairs, parent, arrived, n, d_src, n_src, d_prim_ids, prim_count);
        break;
    case REFIT_BOXES2:
        hipLaunchKernelGGL((k_refit_prims<T, REFIT_BOXES2>), grid, block, 0, stream, d_nodes, d_pairs, parent, arrived, n, d_src, n_src, d_prim_ids, prim_count);
        break;
    case REFIT_TRIS:
        hipLaunchKernelGGL((k_refit_prims<T, REFIT_TRIS>), grid, block, 0, stream, d_nodes, d_pairs, parent, arrived, n, d_src, n_src, d_prim_ids, prim_count);
        break;
    default:
        return fail(BVH_AMD_ERR_ARG, "refit: unknown primitive source");
    }
    BVH_HIP_TRY(hipGetLastError(), BVH_AMD_ERR_HIP);
    return BVH_AMD_OK;
}
template int refit_prims_device<float>(HostNode<float>*, PairNode<float>*, size_t, int, const float*, size_t, const uint32_t*, size_t, hipStream_t);
template int refit_prims_device<double>(HostNode<double>*, PairNode<double>*, size_t, int, const double*, size_t, const uint32_t*, size_t, hipStream_t);

} // namespace bvh_amd
