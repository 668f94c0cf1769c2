// TEST INFRASTRUCTURE (CPU, no GPU): compiles the text of the instanced ray kernels — bvh_amd/csrc/instanced_body.inc with the device
// helpers of bvh_amd/csrc/trace_device.h — for the HOST and runs it with one emulated lane per ray / per instance. What it can show:
// the two-level walk and the instance preparation of the very source the device runs, against the CPU checker's single-level query;
// the device's records must equal these bit for bit. What it cannot show: anything that needs the hardware.
// tests/test_instanced_host.py drives it; tests/test_gpu_instanced.py uses it too.
//
// Built by the tests with: g++ -std=c++20 -O1 -mavx2 -mfma -ffp-contract=off -fno-strict-aliasing -shared -fPIC -pthread.
#include <type_traits>

#include "host_lane_prelude.h"
#include "../../bvh_amd/csrc/instanced_body.inc"

namespace {

using namespace bvh_amd;

template <typename T>
std::vector<InstGeom<T>> geom_table(uint32_t n_geoms, const void* const* pairs, const void* const* tris, const uint32_t* const* prim_ids,
                                    const void* const* root_box, const uint32_t* root_index) {
    std::vector<InstGeom<T>> g(n_geoms);
    for (uint32_t k = 0; k < n_geoms; ++k) {
        g[k].pairs = pairs ? static_cast<const PairNode<T>*>(pairs[k]) : nullptr;
        g[k].tris = tris ? static_cast<const T*>(tris[k]) : nullptr;
        g[k].prim_ids = prim_ids ? prim_ids[k] : nullptr;
        g[k].root_box = root_box ? static_cast<const T*>(root_box[k]) : nullptr;
        g[k].root_index = root_index ? root_index[k] : 0;
        g[k].pad = 0;
    }
    return g;
}

template <typename T, bool Any, bool Robust, bool Deep>
void walk_range(const InstancedArgs<T, false>& a0, unsigned long long begin, unsigned long long end, unsigned long long (&cnt)[3]) {
    InstancedArgs<T, false> a = a0;
    std::vector<uint32_t> lds_node(size_t(kInstLds) * kBlock);
    std::vector<uint32_t> deep_nodes(Deep ? a.deep_cap : 1);
    a.deep_nodes = deep_nodes.data();                         // one lane at a time: lane 0's spill
    for (unsigned long long s = begin; s < end; ++s) instanced_lane<T, Any, Robust, true, Deep, false>(a, s, lds_node.data(), 0, 0, cnt);
}

template <typename T>
int walk(const void* top_pairs, uint32_t top_root, const uint32_t* top_prim_ids, uint32_t n_geoms, const void* const* g_pairs,
         const void* const* g_tris, const uint32_t* const* g_prim_ids, const uint32_t* g_root, const void* world2obj, const uint32_t* geometry,
         const void* rays, size_t n, int any, int robust, int original_ids, uint32_t deep_cap, int threads, void* hits, uint32_t* hit_instances,
         unsigned long long* counters3) {
    const std::vector<InstGeom<T>> table = geom_table<T>(n_geoms, g_pairs, g_tris, g_prim_ids, nullptr, g_root);
    InstancedArgs<T, false> a{};
    a.top_pairs = static_cast<const PairNode<T>*>(top_pairs); a.top_prim_ids = top_prim_ids; a.world2obj = static_cast<const T*>(world2obj);
    a.geometry = geometry; a.rays = static_cast<const T*>(rays); a.hits = static_cast<typename HitOf<T>::Type*>(hits); a.hit_instances = hit_instances;
    a.n = n; a.first = 0; a.deep_cap = deep_cap; a.top_root = top_root; a.n_geoms = n_geoms; a.original_ids = original_ids ? 1u : 0u;
    a.geoms.g = table.data();
    run_lanes(n, threads, counters3, [&](unsigned long long b, unsigned long long e, unsigned long long (&cnt)[3]) {
        auto go = [&](auto an, auto ro) {
            if (deep_cap) walk_range<T, an(), ro(), true>(a, b, e, cnt); else walk_range<T, an(), ro(), false>(a, b, e, cnt);
        };
        if (any) { if (robust) go(std::true_type{}, std::true_type{}); else go(std::true_type{}, std::false_type{}); }
        else { if (robust) go(std::false_type{}, std::true_type{}); else go(std::false_type{}, std::false_type{}); }
    });
    return 0;
}

// One launch of a sliced batch as the device runs it (prelude: GuardedSpill, run_slice): the spill sized for the launch's lanes.
template <typename T>
long long walk_slice(const void* top_pairs, uint32_t top_root, const uint32_t* top_prim_ids, uint32_t n_geoms, const void* const* g_pairs,
                     const void* const* g_tris, const uint32_t* const* g_prim_ids, const uint32_t* g_root, const void* world2obj, const uint32_t* geometry,
                     const void* rays, size_t first, size_t n, size_t launch_lanes, int any, int robust, int original_ids, uint32_t deep_cap, void* hits,
                     uint32_t* hit_instances, unsigned long long* counters3) {
    if (deep_cap == 0 || n > launch_lanes) return kSliceBadArgs;
    const std::vector<InstGeom<T>> table = geom_table<T>(n_geoms, g_pairs, g_tris, g_prim_ids, nullptr, g_root);
    InstancedArgs<T, false> a{};
    a.top_pairs = static_cast<const PairNode<T>*>(top_pairs); a.top_prim_ids = top_prim_ids; a.world2obj = static_cast<const T*>(world2obj);
    a.geometry = geometry; a.rays = static_cast<const T*>(rays); a.hits = static_cast<typename HitOf<T>::Type*>(hits); a.hit_instances = hit_instances;
    a.n = n; a.first = first; a.deep_cap = deep_cap; a.top_root = top_root; a.n_geoms = n_geoms; a.original_ids = original_ids ? 1u : 0u;
    a.geoms.g = table.data();
    GuardedSpill<uint32_t> deep_nodes(first, launch_lanes, deep_cap);
    a.deep_nodes = deep_nodes.data();
    std::vector<uint32_t> lds_node(size_t(kInstLds) * kBlock);
    run_slice(n, kBlock, counters3, [&](unsigned long long lane, int tid, unsigned long long (&cnt)[3]) {
        auto go = [&](auto an, auto ro) { instanced_lane<T, an(), ro(), true, true, false>(a, first + lane, lds_node.data(), tid, lane, cnt); };
        if (any) { if (robust) go(std::true_type{}, std::true_type{}); else go(std::true_type{}, std::false_type{}); }
        else { if (robust) go(std::false_type{}, std::true_type{}); else go(std::false_type{}, std::false_type{}); }
    });
    if (!deep_nodes.guards_intact()) return kSliceGuardBroken;
    return deep_nodes.overwritten();
}

template <typename T>
int prepare(uint32_t n_geoms, const void* const* g_root_box, const void* obj2world, const uint32_t* geometry, size_t n, void* world2obj, void* bboxes,
            void* centers) {
    const std::vector<InstGeom<T>> table = geom_table<T>(n_geoms, nullptr, nullptr, nullptr, g_root_box, nullptr);
    InstancePrepareArgs<T, false> a{};
    a.obj2world = static_cast<const T*>(obj2world); a.geometry = geometry; a.world2obj = static_cast<T*>(world2obj);
    a.bboxes = static_cast<T*>(bboxes); a.centers = static_cast<T*>(centers); a.n = n; a.n_geoms = n_geoms;
    a.geoms.g = table.data();
    for (size_t i = 0; i < n; ++i) instance_prepare_lane<T, false>(a, i);
    return 0;
}

} // namespace

extern "C" {

// The kernel's two-level walk for n rays {org, dir, tmin, tmax}. Top tree: pair records, root index word, prim ids (slot -> instance).
// Geometry k: g_pairs[k], g_tris[k] (BVH-order PrecomputedTri), g_prim_ids[k], g_root[k]. world2obj: 12 per instance; geometry: per
// instance or NULL (all 0). deep_cap > 0: the HBM spill of a stack bound beyond 64, deep_cap entries. hits: bvh_hit3f / bvh_hit3d;
// hit_instances: uint32 per ray; counters3 = {pairs fetched, triangles tested, leaves visited}. Returns 0.
int instanced_host_walk(int is_double, const void* top_pairs, uint32_t top_root, const uint32_t* top_prim_ids, uint32_t n_geoms,
                        const void* const* g_pairs, const void* const* g_tris, const uint32_t* const* g_prim_ids, const uint32_t* g_root,
                        const void* world2obj, const uint32_t* geometry, const void* rays, size_t n, int any, int robust, int original_ids,
                        uint32_t deep_cap, int threads, void* hits, uint32_t* hit_instances, unsigned long long* counters3) {
    if (is_double)
        return walk<double>(top_pairs, top_root, top_prim_ids, n_geoms, g_pairs, g_tris, g_prim_ids, g_root, world2obj, geometry, rays, n, any, robust,
                            original_ids, deep_cap, threads, hits, hit_instances, counters3);
    return walk<float>(top_pairs, top_root, top_prim_ids, n_geoms, g_pairs, g_tris, g_prim_ids, g_root, world2obj, geometry, rays, n, any, robust,
                       original_ids, deep_cap, threads, hits, hit_instances, counters3);
}

// One launch of a batch that the instanced driver cut into slices (deep_cap > 0): rays [first, first + n) as the device walks them —
// a.first = first, ray = first + lane, lane = 0 .. n-1 indexing a spill of launch_lanes * deep_cap entries that the launch's lanes
// share, tid = lane % 256 in one LDS stand-in. rays, hits and hit_instances are the whole batch's. Returns the spill entries the
// launch overwrote, -1 if a guard zone around the spill was written to, -2 for deep_cap == 0 or n > launch_lanes.
long long instanced_host_walk_slice(int is_double, const void* top_pairs, uint32_t top_root, const uint32_t* top_prim_ids, uint32_t n_geoms,
                                    const void* const* g_pairs, const void* const* g_tris, const uint32_t* const* g_prim_ids, const uint32_t* g_root,
                                    const void* world2obj, const uint32_t* geometry, const void* rays, size_t first, size_t n, size_t launch_lanes, int any,
                                    int robust, int original_ids, uint32_t deep_cap, void* hits, uint32_t* hit_instances, unsigned long long* counters3) {
    if (is_double)
        return walk_slice<double>(top_pairs, top_root, top_prim_ids, n_geoms, g_pairs, g_tris, g_prim_ids, g_root, world2obj, geometry, rays, first, n,
                                  launch_lanes, any, robust, original_ids, deep_cap, hits, hit_instances, counters3);
    return walk_slice<float>(top_pairs, top_root, top_prim_ids, n_geoms, g_pairs, g_tris, g_prim_ids, g_root, world2obj, geometry, rays, first, n,
                             launch_lanes, any, robust, original_ids, deep_cap, hits, hit_instances, counters3);
}

// The kernel's instance preparation: g_root_box[k] = {minx, maxx, miny, maxy, minz, maxz} of geometry k's root; obj2world 12 per
// instance -> world2obj (12), bboxes {min.xyz, max.xyz} (6), centers (3) per instance. Returns 0.
int instanced_host_prepare(int is_double, uint32_t n_geoms, const void* const* g_root_box, const void* obj2world, const uint32_t* geometry, size_t n,
                           void* world2obj, void* bboxes, void* centers) {
    if (is_double) return prepare<double>(n_geoms, g_root_box, obj2world, geometry, n, world2obj, bboxes, centers);
    return prepare<float>(n_geoms, g_root_box, obj2world, geometry, n, world2obj, bboxes, centers);
}

} // extern "C"
