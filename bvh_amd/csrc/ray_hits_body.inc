// Per-lane body of the batched all-hits ray query (ray_hits.hip): every BVH-order primitive — a PrecomputedTri or a Sphere — that
// the UNSHORTENED ray {org, dir, tmin, tmax} crosses, as a count and, optionally, a list of hit records in the ray's segment of a
// caller-sized buffer. It is a client of list_walk.inc, like radius_body.inc and overlap_body.inc: the enter test is the
// ray / box slab test of the ray walks (trace_device.h: ray_constants, slab_pair), the hit test their ray / primitive test
// (ray_prim_test.inc: tri_test.inc, the sphere expressions of trace_body.inc; shared with ray_nearest_body.inc), both against the ray's own [tmin, tmax]: nothing a hit finds shortens
// the ray, so the list is what the reference's intersect<false, Robust> reports to a leaf_fn that never shortens it.
// Kept as an include so that tests/cpp/ray_hits_body_host.cpp compiles the very same text for the host (one emulated lane per ray).
// The records leave through point_walk.inc's store_record. Expects what point_walk.inc expects.
#pragma once

#include "list_walk.inc"

namespace bvh_amd {

namespace {

constexpr int kRayHitsLds = kListLds;          // the kernel and the harness size their LDS array by this name

template <typename T>
struct RayHitsArgs : ListArgs<T> {             // queries = rays, 8 scalars each; counts = primitives crossed; list_prims is unused
    typename HitOf<T>::Type* list_hits;        // Fill kernels only: the record intersect writes, one per listed primitive
};

// One ray, one lane: list_walk (which has the order of the walk and the shape of the output). A child is entered iff the ray's
// [tmin, tmax] meets its box (bvh.h:177-180 through slab_pair; a NaN bound fails); a primitive matches iff the leaf test of the ray
// walks accepts it against a copy of tmax that no other test has touched; the unused rest of a segment is padded with intersect's miss
// record {BVH_AMD_INVALID, tmax, 0, 0}. A ray whose tmin or tmax is NaN is not walked (the `nan_ray` of slab_pair's callers); every
// other ray is, whatever its direction or bounds. Slot `slot` of the launch (ray order[slot], or slot itself); `lane` indexes the HBM
// spill (Deep), `tid` the LDS array. cnt += {pair records fetched, primitives tested, leaves visited}.
template <typename T, int Leaf, bool Robust, bool Stats, bool Deep, bool Fill>
__device__ inline void ray_hits_lane(const RayHitsArgs<T>& a, unsigned long long slot, uint32_t* lds_node, int tid, unsigned long long lane,
                                     unsigned long long (&cnt)[3]) {
    const unsigned long long qi = a.order ? a.order[slot] : slot;
    T r[8];
    load_ray(a.queries + 8ull * qi, r);
    const T org[3] = { r[0], r[1], r[2] }, dir[3] = { r[3], r[4], r[5] };
    const T tmin = r[6], ray_tmax = r[7];
    T inv[3], aux[3];
    uint32_t oct[3];
    ray_constants<T, Robust, 3>(org, dir, inv, aux, oct);
    const bool valid = tmin == tmin && ray_tmax == ray_tmax;

    list_walk<T, Stats, Deep, Fill>(a, qi, valid, lds_node, tid, lane, cnt,
        [&](const T (&box)[6]) {
            // (slab_pair itself, the box in both places: the ray walks' arithmetic bit for bit, and the second copy folds away)
            T l0, l1, r0, r1;
            slab_pair<T, Robust, 3>(box, box, org, inv, aux, oct, tmin, ray_tmax, l0, l1, r0, r1);
            return l0 <= l1;
        },
        [&](uint32_t i, unsigned long long at, bool room) {
            if (Stats) ++cnt[1];
            const T* const prims = a.prims;                                     // (the names ray_prim_test.inc expects)
            T tmax = ray_tmax;                                                  // this test's own copy: what it finds shortens nothing else
            T hit_t = T(0), hit_u = T(0), hit_v = T(0);
            bool accepted = false;
#include "ray_prim_test.inc"
            if (!accepted) return false;
            if (room) store_record(a.list_hits + at, a.prim_ids ? a.prim_ids[i] : i, hit_t, hit_u, hit_v);
            return true;
        },
        [&](unsigned long long at) { store_record(a.list_hits + at, BVH_AMD_INVALID, ray_tmax, T(0), T(0)); });
}

} // namespace

} // namespace bvh_amd
