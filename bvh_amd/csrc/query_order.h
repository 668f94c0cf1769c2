// Reading order of a batch of point queries {x, y, z, max_distance} (closest.hip, radius.hip, knn.hip, through point_query.h): the
// queries sorted by the Hilbert cell of each point in the root box (ray_key.h, radix sort), so that neighbouring lanes walk the same
// records. One copy for the three kinds of query (closest_keys_kernel is named after the first). Query BOXES (overlap.hip) are ordered
// by the cell of their centre, query RAYS (ray_hits.hip) by the cell of their origin and the octant of their direction, query TRIANGLES
// (tri_intersect.hip) by the cell of the centre of their box.
// Expects common.h, trace_device.h and ray_key.h to have been included.
#pragma once

#include <algorithm>
#include <string>

namespace bvh_amd {

namespace {

// What a query of a batch is: a point {x, y, z, max_distance}, a box {min.xyz, max.xyz}, a ray {org, dir, tmin, tmax}, or a triangle
// {p0.xyz, p1.xyz, p2.xyz}.
enum QueryKind : int { kQueryPoints = 0, kQueryBoxes = 1, kQueryRays = 2, kQueryTris = 3 };

// Sort keys of the queries: ray_key of the ray {p, dir = +0, 0, max_distance} without chord classes (the octant bits are 0), one
// radix tile per block with its first-digit histogram, like traverse.hip's ray_keys_kernel.
template <typename T>
__global__ void __launch_bounds__(1024) closest_keys_kernel(const T* queries, uint32_t n, T lx, T ly, T lz, T sx, T sy, T sz, uint32_t cells,
                                                            uint32_t* keys, uint32_t* hist, uint32_t tiles) {
    __shared__ uint32_t h[256];
    if (threadIdx.x < 256) h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * uint32_t(kRadixTileU32);
#pragma unroll
    for (int s0 = 0; s0 < kRadixTileU32 / 1024; ++s0) {
        const uint32_t i = base + uint32_t(s0) * 1024u + threadIdx.x;
        if (i < n) {
            T q[4];
            load_prim4(queries + 4ull * i, q);
            const T r[8] = { q[0], q[1], q[2], T(0), T(0), T(0), T(0), q[3] };
            const int hilbert_bits = 31 - __clz(cells);
            const uint32_t key = ray_key<T>(r, lx, ly, lz, sx, sy, sz, cells, hilbert_bits, 0, T(0));
            keys[i] = key;
            atomicAdd(&h[key & 0xFFu], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < 256) hist[size_t{threadIdx.x} * tiles + blockIdx.x] = h[threadIdx.x];
}

// The same keys for query BOXES {min.xyz, max.xyz} (overlap.hip): the cell of the box's centre. A centre that is NaN (a NaN component,
// -inf + inf) lands in cell 0; the order never changes a result.
template <typename T>
__global__ void __launch_bounds__(1024) box_keys_kernel(const T* boxes, uint32_t n, T lx, T ly, T lz, T sx, T sy, T sz, uint32_t cells,
                                                        uint32_t* keys, uint32_t* hist, uint32_t tiles) {
    __shared__ uint32_t h[256];
    if (threadIdx.x < 256) h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * uint32_t(kRadixTileU32);
#pragma unroll
    for (int s0 = 0; s0 < kRadixTileU32 / 1024; ++s0) {
        const uint32_t i = base + uint32_t(s0) * 1024u + threadIdx.x;
        if (i < n) {
            const T* q = boxes + 6ull * i;
            const T r[8] = { T(0.5) * q[0] + T(0.5) * q[3], T(0.5) * q[1] + T(0.5) * q[4], T(0.5) * q[2] + T(0.5) * q[5], T(0), T(0), T(0), T(0), T(0) };
            const int hilbert_bits = 31 - __clz(cells);
            const uint32_t key = ray_key<T>(r, lx, ly, lz, sx, sy, sz, cells, hilbert_bits, 0, T(0));
            keys[i] = key;
            atomicAdd(&h[key & 0xFFu], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < 256) hist[size_t{threadIdx.x} * tiles + blockIdx.x] = h[threadIdx.x];
}

// The same keys for query TRIANGLES {p0.xyz, p1.xyz, p2.xyz} (tri_intersect.hip): the cell of the centre of the triangle's box, which
// is the box the walk tests the nodes against. A centre that is NaN lands in cell 0; the order never changes a result.
template <typename T>
__global__ void __launch_bounds__(1024) tri_keys_kernel(const T* tris, uint32_t n, T lx, T ly, T lz, T sx, T sy, T sz, uint32_t cells,
                                                        uint32_t* keys, uint32_t* hist, uint32_t tiles) {
    __shared__ uint32_t h[256];
    if (threadIdx.x < 256) h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * uint32_t(kRadixTileU32);
#pragma unroll
    for (int s0 = 0; s0 < kRadixTileU32 / 1024; ++s0) {
        const uint32_t i = base + uint32_t(s0) * 1024u + threadIdx.x;
        if (i < n) {
            const T* q = tris + 9ull * i;
            T c[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const T a = q[k], b = q[3 + k], d = q[6 + k];
                const T mn = b < a ? b : a, mx = b > a ? b : a;
                c[k] = T(0.5) * (d < mn ? d : mn) + T(0.5) * (d > mx ? d : mx);
            }
            const T r[8] = { c[0], c[1], c[2], T(0), T(0), T(0), T(0), T(0) };
            const int hilbert_bits = 31 - __clz(cells);
            const uint32_t key = ray_key<T>(r, lx, ly, lz, sx, sy, sz, cells, hilbert_bits, 0, T(0));
            keys[i] = key;
            atomicAdd(&h[key & 0xFFu], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < 256) hist[size_t{threadIdx.x} * tiles + blockIdx.x] = h[threadIdx.x];
}

// The same keys for query RAYS {org, dir, tmin, tmax} (ray_hits.hip): the cell of the origin above the octant of the direction, without
// chord classes (a one-shot grid has no drain to shape). A NaN origin component lands in cell 0; the order never changes a result.
template <typename T>
__global__ void __launch_bounds__(1024) ray_query_keys_kernel(const T* rays, uint32_t n, T lx, T ly, T lz, T sx, T sy, T sz, uint32_t cells,
                                                              uint32_t* keys, uint32_t* hist, uint32_t tiles) {
    __shared__ uint32_t h[256];
    if (threadIdx.x < 256) h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * uint32_t(kRadixTileU32);
#pragma unroll
    for (int s0 = 0; s0 < kRadixTileU32 / 1024; ++s0) {
        const uint32_t i = base + uint32_t(s0) * 1024u + threadIdx.x;
        if (i < n) {
            T r[8];
            load_ray(rays + 8ull * i, r);
            const int hilbert_bits = 31 - __clz(cells);
            const uint32_t key = ray_key<T>(r, lx, ly, lz, sx, sy, sz, cells, hilbert_bits, 0, T(0));
            keys[i] = key;
            atomicAdd(&h[key & 0xFFu], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < 256) hist[size_t{threadIdx.x} * tiles + blockIdx.x] = h[threadIdx.x];
}

// *order = slot -> query index of the n < 2^31 queries sorted by their cell (2^cell_bits cells per axis), in stream order. The scratch
// behind it is *sort_mem / *sort_tag: the caller hands it to scratch_free once its launches are queued (also when this fails: then
// *sort_mem may or may not be set). `who` names the caller in error messages. Kind: d_queries holds 4 scalars per query, 6 (kQueryBoxes: box_keys_kernel)
// 8 (kQueryRays: ray_query_keys_kernel) or 9 (kQueryTris: tri_keys_kernel).
template <typename T, int Kind = kQueryPoints>
int query_order(const BvhImpl<T>& b, const T* d_queries, size_t n, int cell_bits, const char* who, hipStream_t stream, void** sort_mem,
                ScratchTag* sort_tag, const uint32_t** order_out) {
    const uint32_t n32 = static_cast<uint32_t>(n);
    const int key_bits = 3 * cell_bits + 3;
    const RadixOrderLayout layout = radix_order_layout(n32, key_bits);        // keys, carried keys, indices + tmp, histogram + digit totals
    const hipError_t e = scratch_alloc(sort_mem, layout.words * sizeof(uint32_t), sort_tag);
    if (e != hipSuccess) { *sort_mem = nullptr; return fail(BVH_AMD_ERR_HIP, std::string(who) + ": no scratch for the query sort: " + hipGetErrorString(e)); }
    uint32_t *keys = static_cast<uint32_t*>(*sort_mem), *hist = keys + layout.hist;
    const uint32_t cells = 1u << cell_bits;
    T lo[3], sc[3];
    if (const int rc0 = b.wait_refit()) return rc0;                   // root_bounds follows a refit_* that changed the boxes on the device
    for (int k = 0; k < 3; ++k) {
        const T ext = b.root_bounds[2 * k + 1] - b.root_bounds[2 * k];
        lo[k] = b.root_bounds[2 * k];
        sc[k] = ext > T(0) ? T(cells) / ext : T(0);
    }
    const uint32_t tiles = (n32 + kRadixTileU32 - 1) / kRadixTileU32;
    if constexpr (Kind == kQueryRays)
        hipLaunchKernelGGL(ray_query_keys_kernel<T>, dim3(tiles), dim3(1024), 0, stream, d_queries, n32, lo[0], lo[1], lo[2], sc[0], sc[1], sc[2], cells,
                           keys, hist, tiles);
    else if constexpr (Kind == kQueryTris)
        hipLaunchKernelGGL(tri_keys_kernel<T>, dim3(tiles), dim3(1024), 0, stream, d_queries, n32, lo[0], lo[1], lo[2], sc[0], sc[1], sc[2], cells,
                           keys, hist, tiles);
    else if constexpr (Kind == kQueryBoxes)
        hipLaunchKernelGGL(box_keys_kernel<T>, dim3(tiles), dim3(1024), 0, stream, d_queries, n32, lo[0], lo[1], lo[2], sc[0], sc[1], sc[2], cells,
                           keys, hist, tiles);
    else
        hipLaunchKernelGGL(closest_keys_kernel<T>, dim3(tiles), dim3(1024), 0, stream, d_queries, n32, lo[0], lo[1], lo[2], sc[0], sc[1], sc[2], cells,
                           keys, hist, tiles);
    BVH_HIP_TRY(hipGetLastError(), BVH_AMD_ERR_HIP);
    uint32_t* order = nullptr;
    const int rc = radix_sort_order(keys, n32, key_bits, stream, /*first_hist_done=*/true, &order);
    if (rc) return rc;
    *order_out = order;
    return BVH_AMD_OK;
}

} // namespace

} // namespace bvh_amd
