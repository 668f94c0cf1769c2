// What the per-lane bodies of the point, box, triangle, region and ray-list queries share (knn_body.inc, winding_body.inc,
// instanced_body.inc; through nearest_walk.inc closest_body.inc, ray_nearest_body.inc, sphere_cast_body.inc and tri_distance_body.inc;
// through list_walk.inc radius_body.inc, overlap_body.inc, tri_intersect_body.inc, region_body.inc and ray_hits_body.inc; tri_pair.inc):
// the arguments common to their kernels, the query load, the squared distance of a point to one primitive — a PrecomputedTri
// {p0, e1 = p0 - p1, e2 = p2 - p0, n} or a Sphere {c, r} — and to a box, the closed box-overlap tests, the streaming stores of the
// outputs (list entries, hit records) and the index arithmetic of the walk's three-tier stack. Kept as an
// include so that the host harnesses (tests/cpp/*_body_host.cpp) compile the very same text, through the bodies, with one emulated lane
// per query. Expects trace_device.h (Num, dot3, load_pair, load_prim12, load_prim4, store_hit, store_hit_nt, kBlock) and common.h, or the harnesses' stand-ins
// for it (tests/cpp/host_lane_prelude.h: PairNode, HitOf, kCountBits, kCountMask, LEAF_*). Compiled with -ffp-contract=off on both
// sides: one rounding per operation, division and square root correctly rounded, so host and device produce the same bits.
#pragma once

namespace bvh_amd {

namespace {

// The first kPointSmall stack entries of a lane live on the chip (LDS, then scratch), the rest in HBM: the tiers are described below.
constexpr int kPointSmall = 64;

template <typename T>
struct PointArgs {
    const PairNode<T>* pairs;
    const T* prims;                            // BVH order: PrecomputedTri (12 scalars) or Sphere<T, 3> (4 scalars)
    const T* queries;                          // {x, y, z, max_distance} per query, caller order
    unsigned long long n;                      // slots of this launch: [first, first + n)
    unsigned long long first;
    const uint32_t* order;                     // optional: slot -> query index (coherence sort); results are unaffected
    const uint32_t* prim_ids;                  // optional: report prim_ids[i] instead of the BVH-order index i (BVH_AMD_RAY_ORIGINAL_IDS)
    bvh_amd_counters* counters;                // Stats kernels only
    uint32_t* deep_nodes;                      // Deep kernels only: deep_cap entries per lane of the launch beyond the 64 of LDS + scratch
    uint32_t deep_cap;
    uint32_t root_index;
};

// Slot `slot` of the launch: query order[slot], or slot itself. False for NaN coordinates, a NaN or a negative max_distance: such a
// query finds nothing.
template <typename T>
__device__ inline bool load_query(const PointArgs<T>& a, unsigned long long slot, unsigned long long& qi, T (&q)[3], T& max_d) {
    qi = a.order ? a.order[slot] : slot;
    T qq[4];
    load_prim4(a.queries + 4ull * qi, qq);
    q[0] = qq[0]; q[1] = qq[1]; q[2] = qq[2];
    max_d = qq[3];
    return q[0] == q[0] && q[1] == q[1] && q[2] == q[2] && max_d >= T(0);
}

// The closest point of a segment {s, s + e} to q, where sq = q - s: squared distance, and the point's parameter along e in [0, 1].
template <typename T>
__device__ inline T segment_dist2(const T (&sq)[3], const T (&e)[3], T& t) {
    const T ee = dot3(e[0], e[1], e[2], e[0], e[1], e[2]);
    T w = ee > T(0) ? dot3(sq[0], sq[1], sq[2], e[0], e[1], e[2]) / ee : T(0);
    w = w > T(0) ? w : T(0);
    w = w < T(1) ? w : T(1);
    t = w;
    const T d0 = sq[0] - w * e[0], d1 = sq[1] - w * e[1], d2 = sq[2] - w * e[2];
    return dot3(d0, d1, d2, d0, d1, d2);
}

// Squared distance from q to the solid triangle of a PrecomputedTri and the barycentrics (u, v) of its closest point, point =
// p0 + u (p1 - p0) + v (p2 - p0) = p0 - u e1 + v e2 (the convention of the ray records, trace_body.inc), from ab = -e1, ac = e2 and
// ap = q - p0 (no vertex is rebuilt). The closest point of a triangle is either the foot of q on its plane, when that falls inside, or
// the closest point of one of its three edges; so the result is the nearest of these candidates: the foot (when the 2 x 2 system for
// its barycentrics has a positive determinant and the solution lies in the triangle) and the three edges, ties to the first of foot,
// AB, AC, BC. Every candidate is a point of the triangle, so a degenerate or nearly degenerate triangle (collinear or coincident
// vertices, whose determinant is 0 or rounding noise) can only lose its foot, never report a point that is not on it: it is measured
// against its edges, and a rounding accident in the foot's barycentrics can never make the result farther than the nearest edge.
// Never NaN or inf for finite input.
template <typename T>
__device__ inline T tri_dist2(const T (&p)[12], const T (&q)[3], T& u, T& v) {
    const T ab[3] = { -p[3], -p[4], -p[5] }, ac[3] = { p[6], p[7], p[8] };
    const T ap[3] = { q[0] - p[0], q[1] - p[1], q[2] - p[2] };
    const T abab = dot3(ab[0], ab[1], ab[2], ab[0], ab[1], ab[2]), acac = dot3(ac[0], ac[1], ac[2], ac[0], ac[1], ac[2]);
    const T abac = dot3(ab[0], ab[1], ab[2], ac[0], ac[1], ac[2]);
    const T apab = dot3(ap[0], ap[1], ap[2], ab[0], ab[1], ab[2]), apac = dot3(ap[0], ap[1], ap[2], ac[0], ac[1], ac[2]);
    T best = Num<T>::kMax, t = T(0);
    bool found = false;
    const T det = abab * acac - abac * abac;
    if (det > T(0)) {                                         // the foot of q on the plane: ap = fu ab + fv ac + (normal part)
        const T fu = (acac * apab - abac * apac) / det, fv = (abab * apac - abac * apab) / det;
        if (fu >= T(0) && fv >= T(0) && fu + fv <= T(1)) {
            const T d0 = (ap[0] - fu * ab[0]) - fv * ac[0], d1 = (ap[1] - fu * ab[1]) - fv * ac[1], d2 = (ap[2] - fu * ab[2]) - fv * ac[2];
            best = dot3(d0, d1, d2, d0, d1, d2); u = fu; v = fv; found = true;
        }
    }
    const T d_ab = segment_dist2(ap, ab, t);
    if (!found || d_ab < best) { best = d_ab; u = t; v = T(0); }
    const T d_ac = segment_dist2(ap, ac, t);
    if (d_ac < best) { best = d_ac; u = T(0); v = t; }
    const T bp[3] = { ap[0] - ab[0], ap[1] - ab[1], ap[2] - ab[2] };
    const T bc[3] = { ac[0] - ab[0], ac[1] - ab[1], ac[2] - ab[2] };
    const T d_bc = segment_dist2(bp, bc, t);
    if (d_bc < best) { best = d_bc; u = T(1) - t; v = t; }
    return best;
}

// Squared distance from q to the solid sphere {c, r}: max(|q - c| - r, 0)^2 (a point inside is at distance 0).
template <typename T>
__device__ inline T sphere_dist2(const T (&s)[4], const T (&q)[3]) {
    const T o0 = q[0] - s[0], o1 = q[1] - s[1], o2 = q[2] - s[2];
    const T d = Num<T>::sqrt_(dot3(o0, o1, o2, o0, o1, o2)) - s[3];
    const T e = d > T(0) ? d : T(0);
    return e * e;
}

// Squared distance from q to a box {minx, maxx, miny, maxy, minz, maxz} (0 inside): a lower bound of the distance to anything in it.
template <typename T>
__device__ inline T box_dist2(const T (&b)[6], const T (&q)[3]) {
    T e[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const T lo = b[2 * k] - q[k], hi = q[k] - b[2 * k + 1];
        const T m = lo > hi ? lo : hi;
        e[k] = m > T(0) ? m : T(0);
    }
    return dot3(e[0], e[1], e[2], e[0], e[1], e[2]);
}

// A box {min.xyz, max.xyz} of the caller's arrays (aligned to its scalar only).
template <typename T>
__device__ inline void load_box6(const T* p, T (&lo)[3], T (&hi)[3]) {
    lo[0] = p[0]; lo[1] = p[1]; lo[2] = p[2];
    hi[0] = p[3]; hi[1] = p[4]; hi[2] = p[5];
}

// Closed intervals on one axis: [lo, hi] is the query's, already known to be proper (lo <= hi); [bmin, bmax] overlaps it iff it is
// proper itself and neither lies wholly before the other. A NaN makes the comparison it is part of false; -0 equals +0.
template <typename T>
__device__ inline bool axis_overlaps(T bmin, T bmax, T lo, T hi) { return bmin <= hi && lo <= bmax && bmin <= bmax; }

// The one test of the walk, for a child's box of a pair record {minx, maxx, miny, maxy, minz, maxz} ...
template <typename T>
__device__ inline bool node_overlaps(const T (&b)[6], const T (&lo)[3], const T (&hi)[3]) {
    return axis_overlaps(b[0], b[1], lo[0], hi[0]) && axis_overlaps(b[2], b[3], lo[1], hi[1]) && axis_overlaps(b[4], b[5], lo[2], hi[2]);
}
// ... and for a primitive's box {min.xyz}, {max.xyz}.
template <typename T>
__device__ inline bool box_overlaps(const T (&bl)[3], const T (&bh)[3], const T (&lo)[3], const T (&hi)[3]) {
    return axis_overlaps(bl[0], bh[0], lo[0], hi[0]) && axis_overlaps(bl[1], bh[1], lo[1], hi[1]) && axis_overlaps(bl[2], bh[2], lo[2], hi[2]);
}

// Squared distance from q to BVH-order primitive i; (u, v) = the barycentrics of the closest point of a triangle (untouched for a sphere).
template <typename T, int Leaf>
__device__ inline T leaf_dist2(const T* prims, uint32_t i, const T (&q)[3], T& u, T& v) {
    if (Leaf == LEAF_TRIANGLE) {
        T p[12];
        load_prim12(prims + 12ull * i, p);
        return tri_dist2(p, q, u, v);
    }
    T s[4];
    load_prim4(prims + 4ull * i, s);
    return sphere_dist2(s, q);
}

// A list or row entry is written once, by one lane, and not read again by the launch; neighbouring lanes write far apart. Marked
// non-temporal so that the outputs do not take lines of the L2 away from the records and primitives the walks share.
template <typename V>
__device__ inline void store_stream(V* p, V v) {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}

// A list record is written once and not read again by the launch: one streaming store of 16 bytes (float) or two (double).
__device__ inline void store_record(bvh_hit3f* out, uint32_t prim, float t, float u, float v) { store_hit_nt(out, prim, t, u, v); }
__device__ inline void store_record(bvh_hit3d* out, uint32_t prim, double t, double u, double v) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef double d2 __attribute__((ext_vector_type(2)));
    d2 a, b;
    a.x = __longlong_as_double(static_cast<long long>(prim)); a.y = t; b.x = u; b.y = v;
    __builtin_nontemporal_store(a, reinterpret_cast<d2*>(out));
    __builtin_nontemporal_store(b, reinterpret_cast<d2*>(out) + 1);
#else
    store_hit(out, prim, t, u, v);
#endif
}

// The stack of a lane's walk has three tiers: the first Lds entries in LDS ([depth][lane] arrays: a lane's bank does not depend on
// the depth, conflict-free), the rest of the first kPointSmall in per-lane scratch, entries beyond (Deep kernels: trees deeper than
// 64 levels only) in HBM, deep_cap per lane of the launch. A walk pushes at most one entry per level, so the tree's depth bounds the
// stack; the indices are clamped all the same. These two give the index of entry sp in the scratch arrays of kPointSmall - Lds
// entries (Lds <= sp) and in the HBM arrays (kPointSmall <= sp; `lane` of the launch). The accesses themselves stay in the push / pop
// of the two walks (list_walk.inc, nearest_walk.inc), of knn_body.inc and of instanced_body.inc, on arrays they name: behind pointers held in a struct the compiler merges the LDS and scratch accesses of the
// non-Deep kernels into flat ones, at a cost in registers and occupancy (DESIGN.md, "Point queries: the shared launch path and walk kit").
template <int Lds>
__device__ inline uint32_t stack_small_at(uint32_t sp) {
    return sp - Lds < uint32_t(kPointSmall - Lds - 1) ? sp - Lds : uint32_t(kPointSmall - Lds - 1);
}
template <typename Args>                                      // (PointArgs<T>, or any argument block with a deep_cap: instanced_body.inc)
__device__ inline unsigned long long stack_deep_at(const Args& a, unsigned long long lane, uint32_t sp) {
    const uint32_t i = sp - kPointSmall;
    return lane * a.deep_cap + (i < a.deep_cap ? i : a.deep_cap - 1);
}

} // namespace

} // namespace bvh_amd
