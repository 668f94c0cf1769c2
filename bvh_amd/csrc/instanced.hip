// Batched instanced ray queries for gfx950: a scene of placed copies of meshes — a table of geometries {tree, BVH-order triangles},
// instances {object-to-world matrix, geometry index}, and a top tree built over the instances' world boxes — traced in one launch by
// a two-level walk, and the preparation of the instances (world-to-object matrices, world boxes, centres) that feeds the builders and
// bvhXX_refit_boxes. The per-lane bodies are instanced_body.inc (shared with the host test harness,
// tests/cpp/instanced_body_host.cpp) over point_walk.inc's stack tiers; the launch shape is the point queries' (point_query.h).
//
// MI355X mapping:
//   * one lane per ray, one-shot grid of ceil(n / 256) blocks: no ticket counter, so no work slot of any tree is claimed and any
//     number of launches over the same const trees may run at once. The batch is never reordered;
//   * one stack for both levels: kInstLds entries in LDS, the rest of 64 in per-lane scratch; only when depth(top) + 1 + the deepest
//     geometry exceeds 64 do the Deep kernels run, with an HBM spill sized from the trees' depths and launches cut to fit it;
//   * the world-space ray constants are recomputed from the stored ray when an instance is left, not kept in registers;
//   * the geometry table travels by value in the kernel arguments up to kInstSmallGeoms geometries, and through stream-ordered scratch
//     filled by copy kernels beyond: the call adds no synchronisation, and geometry trees refitted on the stream before it are seen.
//
// Compiled with -ffp-contract=off; division is the correctly rounded form (bit-identical to the host harness).

#include "common.h"
#include "trace_device.h"
#include "ray_key.h"
#include "query_order.h"
#include "instanced_body.inc"
#include "point_query.h"

namespace bvh_amd {

namespace {

template <typename T, bool Any, bool Robust, bool Stats, bool Deep, bool Small>
__global__ void __launch_bounds__(kBlock) instanced_kernel(InstancedArgs<T, Small> a) {
    __shared__ uint32_t lds_node[kInstLds * kBlock];
    const int tid = threadIdx.x;
    const unsigned long long lane = static_cast<unsigned long long>(blockIdx.x) * kBlock + tid;
    unsigned long long cnt[3] = {0, 0, 0};
    if (lane < a.n) instanced_lane<T, Any, Robust, Stats, Deep, Small>(a, a.first + lane, lds_node, tid, lane, cnt);
    if (Stats) add_counters(a.counters, cnt, tid);
}

template <typename T, bool Small>
__global__ void __launch_bounds__(kBlock) instance_prepare_kernel(InstancePrepareArgs<T, Small> a) {
    const unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * kBlock + threadIdx.x;
    if (i < a.n) instance_prepare_lane<T, Small>(a, i);
}

// A table of more than kInstSmallGeoms geometries reaches the device through the kernel arguments all the same, a chunk per launch.
template <typename T>
__global__ void __launch_bounds__(kWave) geom_table_kernel(InstGeomTable<T, true> chunk, InstGeom<T>* out, uint32_t count) {
    if (threadIdx.x < count) out[threadIdx.x] = chunk.g[threadIdx.x];
}

// The geometry table of a call on the host, checked; `boxes`: the preparation reads node 0 of every geometry, so the reference-layout
// nodes must be resident (they are after a device build or a refit_*; a tree that came from the host is pushed once).
template <typename T>
int host_table(const GeomRef<T>* geoms, size_t n_geoms, bool boxes, const std::string& who, std::vector<InstGeom<T>>& table) {
    if (!geoms || n_geoms == 0) return fail(BVH_AMD_ERR_ARG, who + ": no geometries (geoms is null or n_geoms is 0)");
    if (n_geoms >= (size_t{1} << 32)) return fail(BVH_AMD_ERR_ARG, who + ": too many geometries");
    int cur = -1;
    BVH_HIP_TRY(hipGetDevice(&cur), BVH_AMD_ERR_HIP);
    table.resize(n_geoms);
    for (size_t k = 0; k < n_geoms; ++k) {
        const std::string which = who + ": geometry " + std::to_string(k);
        const BvhImpl<T>* b = geoms[k].bvh;
        if (!b) return fail(BVH_AMD_ERR_ARG, which + ": null bvh");
        if (b->dim != 3) return fail(BVH_AMD_ERR_ARG, which + " belongs to another family (3D trees of the call's scalar type only)");
        if (b->node_count == 0 || b->prim_count == 0) return fail(BVH_AMD_ERR_ARG, which + " is empty");
        if (b->device != cur) return fail(BVH_AMD_ERR_ARG, which + ": BVH lives on another device than the current one");
        if (!b->d_prim_ids || (b->pair_count && !b->d_pairs)) return fail(BVH_AMD_ERR_ARG, which + ": BVH has no device copy");
        if (!boxes) {
            if (!geoms[k].d_tris12) return fail(BVH_AMD_ERR_ARG, which + ": null triangle array");
            if (misaligned(geoms[k].d_tris12, 16)) return fail(BVH_AMD_ERR_ARG, which + ": triangles must be 16-byte aligned");
        } else if (!b->d_nodes || b->d_nodes_count != b->node_count) {
            if (const int rc = nodes_resident<T>(*const_cast<BvhImpl<T>*>(b))) return rc;
        }
        table[k] = InstGeom<T>{b->d_pairs, geoms[k].d_tris12, b->d_prim_ids, reinterpret_cast<const T*>(b->d_nodes), b->root_index, 0};
    }
    return BVH_AMD_OK;
}

// Holds the device copy of a large table for the duration of a call.
struct TableScratch {
    void* mem = nullptr;
    ScratchTag tag;
    ~TableScratch() { if (mem) scratch_free(mem, tag); }
};

// Fills `small` (n_geoms <= kInstSmallGeoms) or the scratch copy and *large.
template <typename T>
int device_table(const std::vector<InstGeom<T>>& table, InstGeomTable<T, true>& small, const InstGeom<T>** large, TableScratch& scratch,
                 const std::string& who, hipStream_t stream) {
    const size_t n = table.size();
    if (n <= size_t(kInstSmallGeoms)) {
        for (size_t k = 0; k < n; ++k) small.g[k] = table[k];
        return BVH_AMD_OK;
    }
    const hipError_t e = scratch_alloc(&scratch.mem, n * sizeof(InstGeom<T>), &scratch.tag);
    if (e != hipSuccess) { scratch.mem = nullptr; return fail(BVH_AMD_ERR_HIP, who + ": geometry table: " + hipGetErrorString(e)); }
    InstGeom<T>* out = static_cast<InstGeom<T>*>(scratch.mem);
    for (size_t at = 0; at < n; at += kInstSmallGeoms) {
        InstGeomTable<T, true> chunk{};
        const uint32_t count = static_cast<uint32_t>(std::min<size_t>(kInstSmallGeoms, n - at));
        for (uint32_t k = 0; k < count; ++k) chunk.g[k] = table[at + k];
        hipLaunchKernelGGL(geom_table_kernel<T>, dim3(1), dim3(kWave), 0, stream, chunk, out + at, count);
        BVH_HIP_TRY(hipGetLastError(), BVH_AMD_ERR_HIP);
    }
    *large = out;
    return BVH_AMD_OK;
}

template <typename F>
int instanced_dispatch(bool any, bool robust, bool stats, bool deep, F f) {
    auto sd = [&](auto an, auto ro) {
        if (deep) return stats ? f(an, ro, std::true_type{}, std::true_type{}) : f(an, ro, std::false_type{}, std::true_type{});
        return stats ? f(an, ro, std::true_type{}, std::false_type{}) : f(an, ro, std::false_type{}, std::false_type{});
    };
    if (any) return robust ? sd(std::true_type{}, std::true_type{}) : sd(std::true_type{}, std::false_type{});
    return robust ? sd(std::false_type{}, std::true_type{}) : sd(std::false_type{}, std::false_type{});
}

} // namespace

template <typename T>
int launch_instance_prepare(const GeomRef<T>* geoms, size_t n_geoms, const T* d_obj2world, const uint32_t* d_geometry, size_t n_instances,
                            T* d_world2obj, T* d_bboxes, T* d_centers, hipStream_t stream) {
    const std::string who = "instance_prepare";
    std::vector<InstGeom<T>> table;
    if (const int rc = host_table<T>(geoms, n_geoms, true, who, table)) return rc;
    if (n_instances == 0) return BVH_AMD_OK;
    if (!d_obj2world || !d_world2obj || !d_bboxes || !d_centers) return fail(BVH_AMD_ERR_ARG, who + ": null device pointer");
    if (misaligned(d_obj2world, 16) || misaligned(d_world2obj, sizeof(T)) || misaligned(d_bboxes, sizeof(T)) || misaligned(d_centers, sizeof(T)) ||
        misaligned(d_geometry, 4))
        return fail(BVH_AMD_ERR_ARG, who + ": device pointers must be aligned (matrices in: 16 bytes; outputs: their scalar; geometry indices: 4)");
    StreamScope scope(stream);
    TableScratch scratch;
    InstancePrepareArgs<T, true> a{};                         // the table by value ...
    InstancePrepareArgs<T, false> b{};                        // ... or behind a pointer
    if (const int rc = device_table<T>(table, a.geoms, &b.geoms.g, scratch, who, stream)) return rc;
    auto fill = [&](auto& x) {
        x.obj2world = d_obj2world; x.geometry = d_geometry; x.world2obj = d_world2obj; x.bboxes = d_bboxes; x.centers = d_centers;
        x.n = n_instances; x.n_geoms = static_cast<uint32_t>(n_geoms);
    };
    fill(a); fill(b);
    const unsigned blocks = static_cast<unsigned>((n_instances + kBlock - 1) / kBlock);
    if (b.geoms.g) hipLaunchKernelGGL((instance_prepare_kernel<T, false>), dim3(blocks), dim3(kBlock), 0, stream, b);
    else hipLaunchKernelGGL((instance_prepare_kernel<T, true>), dim3(blocks), dim3(kBlock), 0, stream, a);
    BVH_HIP_TRY(hipGetLastError(), BVH_AMD_ERR_HIP);
    return BVH_AMD_OK;
}

template <typename T>
int launch_instanced(const BvhImpl<T>& top, const GeomRef<T>* geoms, size_t n_geoms, const T* d_world2obj, const uint32_t* d_geometry,
                     size_t n_instances, const T* d_rays, size_t n_rays, unsigned flags, typename HitOf<T>::Type* d_hits, uint32_t* d_hit_instances,
                     bvh_amd_counters* d_counters, hipStream_t stream) {
    const std::string who = "intersect_rays_instanced";
    constexpr unsigned kAccepted = BVH_AMD_RAY_ANY_HIT | BVH_AMD_RAY_ROBUST | BVH_AMD_RAY_ORIGINAL_IDS | BVH_AMD_RAY_UNSORTED;
    if (flags & ~kAccepted)
        return fail(BVH_AMD_ERR_ARG, who + ": unsupported flags (ANY_HIT, ROBUST, ORIGINAL_IDS and UNSORTED only: the batch is never reordered)");
    if (n_rays == 0) return BVH_AMD_OK;
    if (top.dim != 3) return fail(BVH_AMD_ERR_ARG, who + ": 3D trees only");
    std::vector<InstGeom<T>> table;
    if (const int rc = host_table<T>(geoms, n_geoms, false, who, table)) return rc;
    if (!d_world2obj || !d_rays || !d_hits || !d_hit_instances) return fail(BVH_AMD_ERR_ARG, who + ": null device pointer");
    if (misaligned(d_world2obj, 16) || misaligned(d_rays, 16) || misaligned(d_hits, 16) || misaligned(d_hit_instances, 4) || misaligned(d_geometry, 4) ||
        misaligned(d_counters, 8))
        return fail(BVH_AMD_ERR_ARG, who + ": device pointers must be 16-byte aligned (hit instances and geometry indices 4, counters 8)");
    if (top.node_count == 0 || !top.d_prim_ids || (top.pair_count && !top.d_pairs)) return fail(BVH_AMD_ERR_ARG, who + ": the top BVH has no device copy");
    long long largest = 0;                                    // (cached per layout, shared with source_array_check's callers)
    if (const int rc = largest_prim_id(top, stream, &largest)) return rc;
    if (top.prim_count && n_instances <= static_cast<size_t>(largest))
        return fail(BVH_AMD_ERR_ARG, who + ": " + std::to_string(n_instances) + " instances given, but the top tree's prim_ids refer to instance " +
                    std::to_string(largest));

    set_last_query_launches(0);                               // (bvh_amd_last_query_launches: the checks are passed; counted below, one per launch)
    // the stack's bound: depth(top) + the marker + the deepest geometry (cached per layout)
    if (const int rc = tree_depth<T>(top, stream)) return rc;
    int bound = top.max_depth.load() + 1, deepest = 0;
    for (size_t k = 0; k < n_geoms; ++k) {
        if (const int rc = tree_depth<T>(*geoms[k].bvh, stream)) return rc;
        deepest = std::max(deepest, geoms[k].bvh->max_depth.load());
    }
    bound += deepest;

    StreamScope scope(stream);
    TableScratch scratch, deep;
    if (d_counters) BVH_HIP_TRY(hipMemsetAsync(d_counters, 0, sizeof(bvh_amd_counters), stream), BVH_AMD_ERR_HIP);
    InstancedArgs<T, true> a{};                               // the table by value ...
    InstancedArgs<T, false> b{};                              // ... or behind a pointer
    if (const int rc = device_table<T>(table, a.geoms, &b.geoms.g, scratch, who, stream)) return rc;
    const bool by_value = b.geoms.g == nullptr;

    size_t per_launch = std::min(n_rays, kPointMaxLaunch);
    uint32_t deep_cap = 0;
    if (bound > kPointSmall) {                                // as point_query_run cuts them: launches of whole blocks within kPointDeepBytes of spill
        const size_t cap = static_cast<size_t>(bound - kPointSmall + 1), lanes = kBlock;
        per_launch = std::max<size_t>(lanes, kPointDeepBytes / (cap * sizeof(uint32_t)) / lanes * lanes);
        per_launch = std::min(per_launch, (std::min(n_rays, kPointMaxLaunch) + lanes - 1) / lanes * lanes);
        const hipError_t e = scratch_alloc(&deep.mem, per_launch * cap * sizeof(uint32_t), &deep.tag);
        if (e != hipSuccess) { deep.mem = nullptr; return fail(BVH_AMD_ERR_HIP, who + ": stack spill buffer: " + hipGetErrorString(e)); }
        deep_cap = static_cast<uint32_t>(cap);
    }
    int launches = 0;
    for (size_t first = 0; first < n_rays; first += per_launch) {
        auto fill = [&](auto& x) {
            x.top_pairs = top.d_pairs; x.top_prim_ids = top.d_prim_ids; x.world2obj = d_world2obj; x.geometry = d_geometry; x.rays = d_rays;
            x.hits = d_hits; x.hit_instances = d_hit_instances; x.counters = d_counters; x.top_root = top.root_index;
            x.n_geoms = static_cast<uint32_t>(n_geoms); x.original_ids = (flags & BVH_AMD_RAY_ORIGINAL_IDS) ? 1u : 0u;
            x.deep_nodes = static_cast<uint32_t*>(deep.mem); x.deep_cap = deep_cap;
            x.first = first; x.n = std::min(per_launch, n_rays - first);
        };
        fill(a); fill(b);
        const int rc = instanced_dispatch((flags & BVH_AMD_RAY_ANY_HIT) != 0, (flags & BVH_AMD_RAY_ROBUST) != 0, d_counters != nullptr, deep_cap != 0,
                                          [&](auto any, auto robust, auto stats, auto dp) {
            return by_value ? point_query_launch(instanced_kernel<T, any(), robust(), stats(), dp(), true>, a, kBlock, 0, stream)
                            : point_query_launch(instanced_kernel<T, any(), robust(), stats(), dp(), false>, b, kBlock, 0, stream);
        });
        if (rc) return rc;
        set_last_query_launches(++launches);
    }
    return BVH_AMD_OK;
}

template int launch_instance_prepare<float>(const GeomRef<float>*, size_t, const float*, const uint32_t*, size_t, float*, float*, float*, hipStream_t);
template int launch_instance_prepare<double>(const GeomRef<double>*, size_t, const double*, const uint32_t*, size_t, double*, double*, double*, hipStream_t);
template int launch_instanced<float>(const BvhImpl<float>&, const GeomRef<float>*, size_t, const float*, const uint32_t*, size_t, const float*, size_t,
                                     unsigned, bvh_hit3f*, uint32_t*, bvh_amd_counters*, hipStream_t);
template int launch_instanced<double>(const BvhImpl<double>&, const GeomRef<double>*, size_t, const double*, const uint32_t*, size_t, const double*, size_t,
                                      unsigned, bvh_hit3d*, uint32_t*, bvh_amd_counters*, hipStream_t);

} // namespace bvh_amd
