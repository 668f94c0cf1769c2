// Per-lane body of the batched convex-region query (region.hip): every BVH-order primitive (a triangle, or a sphere) that meets the
// intersection of m <= 8 half-spaces, as a count and, optionally, a list in the query's segment of a caller-sized buffer, with a flag
// per entry for "wholly inside". A query is m planes {nx, ny, nz, d}; the value of a plane at x is ((nx*x0 + ny*x1) + nz*x2) + d, one
// rounding per operation, and x is inside the plane iff value <= 0 (a NaN value is not inside). The primitives are the caller's
// arrays indexed by ORIGINAL primitive id: triangles of 9 scalars {p0, p1, p2} (what bvh3X_refit_tris takes), spheres of 4 {c, r}.
//
// Three tests, all on plane values:
//   * node:      a child is entered iff, for every plane, the value at the corner of its box lowest along the normal is <= 0;
//   * CULL:      a triangle is rejected iff some plane has none of its three vertices inside; a sphere iff some plane has
//                !(value(c) <= r * |n|). Plane by plane: conservative near the region's edges and corners;
//   * EXACT:     (triangles) the triangle and the region share a point as closed sets, decided by SIGNS of 3 x 3 determinants of the
//                plane values only (region_exact below): no division, no epsilon, no product of two determinants.
// Kept as an include so that tests/cpp/region_body_host.cpp compiles the very same text for the host (one emulated lane per query).
// Expects what point_walk.inc expects.
#pragma once

#include "list_walk.inc"

namespace bvh_amd {

namespace {

constexpr int kRegionLds = kListLds;           // the kernel and the harness size their LDS array by this name
constexpr int kRegionMaxPlanes = 8;

template <typename T>
struct RegionArgs : ListArgs<T> {              // prims = n_prims x 9 (triangles) or x 4 (spheres) by original id; queries = n x m x {nx, ny, nz, d}
    const uint32_t* ids;                       // BVH-order index -> original id (always; prim_ids is set only to REPORT original ids)
    uint8_t* list_inside;                      // Fill kernels only, optional: parallel to list_prims, 1 = wholly inside the region
    uint32_t m;                                // planes per query, 1 .. kRegionMaxPlanes, the same for the whole batch
};

// (Every loop over the planes below is unrolled over kRegionMaxPlanes and leaves at the wave-uniform m: the planes stay in registers
//  under constant indices. The verdicts of the planes are combined with & and |, not && and ||: a short-circuit per plane is a nest of
//  eight divergent branches, each with a saved exec mask, and the Deep kernels have no scalar registers to spare.)

template <typename T>
__device__ inline T plane_value(const T (&pl)[4], T x0, T x1, T x2) { return ((pl[0] * x0 + pl[1] * x1) + pl[2] * x2) + pl[3]; }

// x - x is 0 for a finite x and NaN for an infinite or NaN one.
template <typename T>
__device__ inline bool finite_(T x) { return x - x == T(0); }

// The m planes of query qi (aligned to their scalar only). False when a component is NaN or infinite: such a query has an empty list.
template <typename T>
__device__ inline bool load_planes(const T* p, uint32_t m, T (&pl)[kRegionMaxPlanes][4]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < kRegionMaxPlanes; ++k) {
        if (uint32_t(k) >= m) break;
        pl[k][0] = p[4 * k]; pl[k][1] = p[4 * k + 1]; pl[k][2] = p[4 * k + 2]; pl[k][3] = p[4 * k + 3];
        ok = ok & finite_(pl[k][0]) & finite_(pl[k][1]) & finite_(pl[k][2]) & finite_(pl[k][3]);
    }
    return ok;
}

// A child's box {minx, maxx, miny, maxy, minz, maxz}: for every plane the corner lowest along the normal (max where the normal's
// component is < 0, min otherwise) is inside. Products and sums round monotonically, so this value is <= the value at every finite
// point of the box: a box is never left while something in it is inside all planes.
template <typename T>
__device__ inline bool node_in_region(const T (&b)[6], const T (&pl)[kRegionMaxPlanes][4], uint32_t m) {
    bool in = true;
#pragma unroll
    for (int k = 0; k < kRegionMaxPlanes; ++k) {
        if (uint32_t(k) >= m) break;
        // n * corner is the smaller of n * min and n * max, for either sign of n (a product rounds monotonically, so the smaller
        // product IS the rounded product with the corner's coordinate). Taken as a minimum of two products and not as a select on
        // the sign of n: the 24 sign tests do not depend on the box, the compiler hoists them out of the walk and keeps them in 48
        // scalar registers, which the kernels do not have. (Where 0 * an infinite box coordinate gives a NaN product the other
        // product stands in: a box without finite bounds, which no builder or refit produces, is entered rather than left.)
        const T t0 = Num<T>::min_num(pl[k][0] * b[0], pl[k][0] * b[1]), t1 = Num<T>::min_num(pl[k][1] * b[2], pl[k][1] * b[3]);
        const T t2 = Num<T>::min_num(pl[k][2] * b[4], pl[k][2] * b[5]);
        in = in & (((t0 + t1) + t2) + pl[k][3] <= T(0));
    }
    return in;
}

// The determinant test of one pair of constraints: cross(Li, Lj) = (cx, cy, w) is, for w != 0, the point (cx / w, cy / w) where the
// two boundary lines meet; constraint Lk holds there iff sign(w) * dot(Lk, cross) <= 0. `ok` collects the other constraints.
template <typename T>
__device__ __forceinline__ bool holds_at(const T (&l)[3], T cx, T cy, T w, bool pos) {
    const T t = (l[0] * cx + l[1] * cy) + l[2] * w;
    return pos ? t <= T(0) : t >= T(0);
}

// EXACT: the triangle and the region share a point. dv[p][i] = the value of plane p at vertex i. In the triangle's (u, v) parameters
// (point = p0 + u (p1 - p0) + v (p2 - p0)) plane p is the constraint L = (dv[p][1] - dv[p][0], dv[p][2] - dv[p][0], dv[p][0]):
// a u + b v + c <= 0; the triangle adds (-1, 0, 0), (0, -1, 0), (1, 1, -1). The 3 + m half-planes bound a polygon inside the unit
// triangle; it is nonempty iff it has a vertex: some pair i < j of constraints whose lines cross (w != 0) at a point where every other
// constraint holds. A triangle without area is the same unit triangle in (u, v): no special case. A constraint with a NaN or infinite
// coefficient (a NaN vertex, an overflow): the triangle is not listed. The triangle's own constraints come first, so that a triangle
// with p0 in the region leaves at the first pair.
template <typename T>
__device__ __forceinline__ bool region_exact(const T (&dv)[kRegionMaxPlanes][3], uint32_t m) {
    constexpr int kN = kRegionMaxPlanes + 3;
    T l[kN][3] = {{T(-1), T(0), T(0)}, {T(0), T(-1), T(0)}, {T(1), T(1), T(-1)}};
    bool finite = true;
#pragma unroll
    for (int p = 0; p < kRegionMaxPlanes; ++p) {
        if (uint32_t(p) >= m) break;
        l[3 + p][0] = dv[p][1] - dv[p][0]; l[3 + p][1] = dv[p][2] - dv[p][0]; l[3 + p][2] = dv[p][0];
        finite = finite & finite_(l[3 + p][0]) & finite_(l[3 + p][1]) & finite_(l[3 + p][2]);
    }
    if (!finite) return false;
    // (no loop below is left early: every exit would be one more edge for the unroller, and a loop it gives up on indexes l[][]
    //  dynamically, which puts the constraints in scratch. A pair is skipped as a whole once a vertex was found.)
    const uint32_t n = m + 3;
    bool found = false;
#pragma unroll
    for (int i = 0; i < kN - 1; ++i) {
#pragma unroll
        for (int j = i + 1; j < kN; ++j) {
            if (!found && uint32_t(j) < n) {
                const T cx = l[i][1] * l[j][2] - l[i][2] * l[j][1], cy = l[i][2] * l[j][0] - l[i][0] * l[j][2];
                const T w = l[i][0] * l[j][1] - l[i][1] * l[j][0];
                const bool pos = w > T(0);
                bool ok = pos || w < T(0);
#pragma unroll
                for (int k = 0; k < kN; ++k) {
                    if (k != i && k != j && uint32_t(k) < n) ok = ok & holds_at(l[k], cx, cy, w, pos);
                }
                found = ok;
            }
        }
    }
    return found;
}

// |n| of every plane: what the sphere test scales a radius by.
template <typename T>
__device__ inline void plane_lengths(const T (&pl)[kRegionMaxPlanes][4], uint32_t m, T (&len)[kRegionMaxPlanes]) {
#pragma unroll
    for (int k = 0; k < kRegionMaxPlanes; ++k) {
        if (uint32_t(k) >= m) break;
        len[k] = Num<T>::sqrt_((pl[k][0] * pl[k][0] + pl[k][1] * pl[k][1]) + pl[k][2] * pl[k][2]);
    }
}

// The triangle {p0, p1, p2} at p (aligned to its scalar only) against the region: CULL, then (Exact) region_exact on the plane values
// CULL computed. inside = all three vertices inside all planes (meaningful when the triangle matches).
template <typename T, bool Exact>
__device__ __forceinline__ bool tri_in_region(const T* p, const T (&pl)[kRegionMaxPlanes][4], uint32_t m, bool& inside) {
    const T v[9] = { p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8] };
    T dv[kRegionMaxPlanes][3];
    bool pass = true, in = true;
#pragma unroll
    for (int k = 0; k < kRegionMaxPlanes; ++k) {
        if (uint32_t(k) >= m) break;
        const T d0 = plane_value(pl[k], v[0], v[1], v[2]), d1 = plane_value(pl[k], v[3], v[4], v[5]), d2 = plane_value(pl[k], v[6], v[7], v[8]);
        const bool i0 = d0 <= T(0), i1 = d1 <= T(0), i2 = d2 <= T(0);
        pass = pass & (i0 | i1 | i2);
        in = in & (i0 & i1 & i2);
        if (Exact) { dv[k][0] = d0; dv[k][1] = d1; dv[k][2] = d2; }
    }
    inside = in;
    if (!pass) return false;
    if (Exact) return region_exact(dv, m);
    return true;
}

// The sphere {c, r} at p (aligned to its scalar only): outside plane k iff !(value(c) <= r * len[k]); inside = value(c) <= -(r * len[k])
// for every plane.
template <typename T>
__device__ __forceinline__ bool sphere_in_region(const T* p, const T (&pl)[kRegionMaxPlanes][4], const T (&len)[kRegionMaxPlanes], uint32_t m, bool& inside) {
    const T s[4] = { p[0], p[1], p[2], p[3] };
    bool pass = true, in = true;
#pragma unroll
    for (int k = 0; k < kRegionMaxPlanes; ++k) {
        if (uint32_t(k) >= m) break;
        const T c = plane_value(pl[k], s[0], s[1], s[2]), rl = s[3] * len[k];
        pass = pass & (c <= rl);
        in = in & (c <= -rl);
    }
    inside = in;
    return pass;
}

// One query, one lane: list_walk (which has the order of the walk and the shape of the output), a child entered iff node_in_region,
// every primitive that passes its test a match, the unused rest of a segment padded with BVH_AMD_INVALID (inside flags: 0).
// The batch is never reordered: slot `slot` of the launch is query `slot`. `lane` indexes the HBM spill (Deep), `tid` the LDS array.
// cnt += {pair records fetched, primitives tested, leaves visited}.
template <typename T, bool Stats, bool Deep, bool Fill, int Leaf, bool Exact>
__device__ inline void region_lane(const RegionArgs<T>& a, unsigned long long slot, uint32_t* lds_node, int tid, unsigned long long lane,
                                   unsigned long long (&cnt)[3]) {
    static_assert(Leaf == LEAF_TRIANGLE || !Exact, "EXACT is a triangle test");
    const unsigned long long qi = slot;
    const uint32_t m = a.m;
    T pl[kRegionMaxPlanes][4];
    const bool valid = load_planes(a.queries + 4ull * m * qi, m, pl);
    T len[kRegionMaxPlanes];
    if (Leaf == LEAF_SPHERE) plane_lengths(pl, m, len);

    list_walk<T, Stats, Deep, Fill>(a, qi, valid, lds_node, tid, lane, cnt,
        [&](const T (&box)[6]) { return node_in_region(box, pl, m); },
        [&](uint32_t i, unsigned long long at, bool room) {
            if (Stats) ++cnt[1];
            const uint32_t id = a.ids[i];
            bool inside = false;
            if (Leaf == LEAF_TRIANGLE) {
                if (!tri_in_region<T, Exact>(a.prims + 9ull * id, pl, m, inside)) return false;
            } else {
                if (!sphere_in_region(a.prims + 4ull * id, pl, len, m, inside)) return false;
            }
            if (room) {
                store_stream(a.list_prims + at, a.prim_ids ? id : i);
                if (a.list_inside) store_stream(a.list_inside + at, uint8_t(inside ? 1 : 0));
            }
            return true;
        },
        [&](unsigned long long at) {
            store_stream(a.list_prims + at, BVH_AMD_INVALID);
            if (a.list_inside) store_stream(a.list_inside + at, uint8_t(0));
        });
}

} // namespace

} // namespace bvh_amd
