// Per-lane body of the batched triangle-distance query (tri_distance.hip): for a query triangle {p0, p1, p2} (a segment or a point
// when its vertices are collinear or coincide), the nearest triangle of the tree, how far it is and where the two come closest, as
// one hit record {prim, t, u, v} and, optionally, the barycentrics of the closest point on the QUERY triangle. The triangles are the
// caller's array of 9 scalars indexed by ORIGINAL primitive id (tri_intersect_body.inc: the triangle of BVH-order primitive i is
// tris[tri_ids[i]]). It is the fourth client of nearest_walk.inc, next to closest_body.inc, ray_nearest_body.inc and
// sphere_cast_body.inc: the key of a box is its squared distance to the query triangle's box, the limit is the best squared distance
// so far, and the leaf test is the pair distance below; the LDS tier of the stack is closest-point's (nearest_walk.inc:
// kClosestLds). Kept as an include so that tests/cpp/tri_distance_body_host.cpp compiles the very same text for the host (one
// emulated lane per query). Expects what point_walk.inc expects.
#pragma once

#include "tri_pair.inc"                        // load_tri9, tri_box, tri_normal, normal_usable, tri_pair_intersects
#include "nearest_walk.inc"

namespace bvh_amd {

namespace {

template <typename T>
struct TriDistanceArgs : PointArgs<T> {        // prims = the triangles, n_tris x 9 by original id; queries = n x 9
    typename HitOf<T>::Type* hits;             // one record per query, caller order
    T* deep_d2;                                // Deep kernels only: beside deep_nodes
    const uint32_t* tri_ids;                   // BVH-order index -> original id (always; prim_ids is set only to REPORT original ids)
    const T* max_distances;                    // optional: one max_distance per query, caller order
    T max_distance;                            // the batch's max_distance when max_distances is null
    T* query_uv;                               // optional: 2 scalars per query, caller order
};

// (Vectors are structs of three named scalars and the loops below ROTATE them instead of indexing arrays of vertices: a lane's
//  array indexed by a loop counter becomes scratch wherever the compiler keeps the loop; tri_pair.inc has the same note.)
template <typename T>
struct Td3 { T x, y, z; };

template <typename T> __device__ inline Td3<T> td_sub(const Td3<T>& a, const Td3<T>& b) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }
template <typename T> __device__ inline T td_dot(const Td3<T>& a, const Td3<T>& b) { return dot3(a.x, a.y, a.z, b.x, b.y, b.z); }
template <typename T> __device__ inline Td3<T> td_along(const Td3<T>& p, T s, const Td3<T>& d) { return { p.x + s * d.x, p.y + s * d.y, p.z + s * d.z }; }
template <typename T>
__device__ inline Td3<T> td_cross(const Td3<T>& a, const Td3<T>& b) { return { a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }

// x clamped to [0, 1]; a NaN (0 * inf of a parameter along an edge of denormal length) becomes 0: every parameter that leaves here
// names a point of its edge.
template <typename T>
__device__ inline T td_clamp01(T x) {
    const T w = x > T(0) ? x : T(0);
    return w < T(1) ? w : T(1);
}
// 1 / x for x > 0, else 0 (an edge of no length, a triangle of no area: the parameter stays 0).
template <typename T>
__device__ inline T td_inv(T x) { return x > T(0) ? T(1) / x : T(0); }

// The face of a triangle {o, o + ab, o + ac}: what the 2 x 2 system of tri_dist2 needs, solved once per triangle.
template <typename T>
struct TdFace {
    Td3<T> o, ab, ac, n;                       // n = ab x ac
    T abab, acac, abac, inv_det;               // inv_det = 0 for a triangle whose Gram determinant is not positive
};

template <typename T>
__device__ inline TdFace<T> td_face(const Td3<T>& p0, const Td3<T>& p1, const Td3<T>& p2) {
    TdFace<T> f;
    f.o = p0; f.ab = td_sub(p1, p0); f.ac = td_sub(p2, p0);
    f.n = td_cross(f.ab, f.ac);
    f.abab = td_dot(f.ab, f.ab); f.acac = td_dot(f.ac, f.ac); f.abac = td_dot(f.ab, f.ac);
    f.inv_det = td_inv(f.abab * f.acac - f.abac * f.abac);
    return f;
}

// The foot of x on the plane of f in barycentrics (fu, fv), and the squared distance from x to the point rebuilt from them (so the
// pair {x, that point} is always a pair of real points, whatever rounding did to fu and fv). True iff the foot lies in the triangle;
// a NaN or infinite (fu, fv) of a triangle whose determinant is noise fails the comparisons.
template <typename T>
__device__ inline bool td_face_foot(const TdFace<T>& f, const Td3<T>& x, T& fu, T& fv, T& d2) {
    const Td3<T> ap = td_sub(x, f.o);
    const T apab = td_dot(ap, f.ab), apac = td_dot(ap, f.ac);
    fu = (f.acac * apab - f.abac * apac) * f.inv_det;
    fv = (f.abab * apac - f.abac * apab) * f.inv_det;
    const Td3<T> d = { (ap.x - fu * f.ab.x) - fv * f.ac.x, (ap.y - fu * f.ab.y) - fv * f.ac.y, (ap.z - fu * f.ab.z) - fv * f.ac.z };
    d2 = td_dot(d, d);
    return fu >= T(0) && fv >= T(0) && fu + fv <= T(1);
}

// Barycentrics (u, v) of the point at parameter x of edge k of a triangle (edge k runs from vertex k to vertex k + 1, cyclic), in
// tri_dist2's convention: point = p0 + u (p1 - p0) + v (p2 - p0).
template <typename T>
__device__ inline void td_edge_uv(int k, T x, T& u, T& v) {
    u = k == 0 ? x : k == 1 ? T(1) - x : T(0);
    v = k == 0 ? T(0) : k == 1 ? x : T(1) - x;
}

// Closest points of the segments {p1, p1 + d1} and {p2, p2 + d2} (a = d1.d1, e = d2.d2, ia = td_inv(a), ie = td_inv(e)): parameters
// s, t in [0, 1] and the squared distance between the two points REBUILT from them. s starts from the unclamped 2 x 2 solution when
// its determinant a e - b^2 is positive (0 otherwise: parallel, or an edge of no length); that determinant cancels for nearly
// parallel edges, so s is not trusted: t is the projection of the s-point onto the other segment, s that of the t-point, twice.
// Each projection is exact in one variable (only the rounding of the coordinates enters), never increases the distance, and the
// first pair already is the optimum whenever s was exact (Ericson, Real-Time Collision Detection, 5.1.9); a parallel pair gets its
// optimum from any s. Never NaN for finite input.
template <typename T>
__device__ inline T td_segment_pair(const Td3<T>& p1, const Td3<T>& d1, T a, T ia, const Td3<T>& p2, const Td3<T>& d2, T e, T ie, T& s, T& t) {
    const Td3<T> r = td_sub(p1, p2);
    const T b = td_dot(d1, d2), c = td_dot(d1, r), f = td_dot(d2, r);
    const T den = a * e - b * b;
    s = den > T(0) ? td_clamp01((b * f - c * e) / den) : T(0);
    t = td_clamp01((b * s + f) * ie);
    s = td_clamp01((b * t - c) * ia);
    t = td_clamp01((b * s + f) * ie);
    s = td_clamp01((b * t - c) * ia);
    const Td3<T> d = { (r.x + s * d1.x) - t * d2.x, (r.y + s * d1.y) - t * d2.y, (r.z + s * d1.z) - t * d2.z };
    return td_dot(d, d);
}

// The three edges of the triangle {a, b, c} against the face f of the other triangle: per edge k ONE point of it, the foot of which
// on f is offered when it falls inside f: the point where the edge crosses f's plane when its ends lie strictly on both sides (an
// edge through the interior of f: every vertex and every edge pair is then apart, the triangles are not), else its first vertex.
// Together the three edges offer all three vertices, except a vertex whose edge crosses the plane: the foot of such a vertex cannot
// be the closest pair, because moving along that edge towards the plane comes closer. offer(d2, fu, fv, k, x).
template <typename T, typename Offer>
__device__ inline void td_edges_to_face(Td3<T> a, Td3<T> b, Td3<T> c, const TdFace<T>& f, Offer offer) {
    T ha = td_dot(td_sub(a, f.o), f.n), hb = td_dot(td_sub(b, f.o), f.n), hc = td_dot(td_sub(c, f.o), f.n);
    for (int k = 0; k < 3; ++k) {
        const bool through = (ha > T(0) && hb < T(0)) || (ha < T(0) && hb > T(0));
        const T x = through ? td_clamp01(ha / (ha - hb)) : T(0);            // |ha - hb| >= |ha| also after rounding; clamped all the same
        T fu, fv, d2;
        if (td_face_foot(f, td_along(a, x, td_sub(b, a)), fu, fv, d2)) offer(d2, fu, fv, k, x);
        const Td3<T> a0 = a;
        a = b; b = c; c = a0;
        const T h0 = ha;
        ha = hb; hb = hc; hc = h0;
    }
}

// What a lane keeps of its query for the whole walk.
template <typename T>
struct TdQuery {
    T raw[9], lo[3], hi[3], n[3];              // the vertices as given, their box, (p1 - p0) x (p2 - p0)
    bool usable;                               // normal_usable(n): the pair test of tri_pair.inc applies
    TdFace<T> face;                            // in the local frame (origin p0): o = 0, ab = p1 - p0, ac = p2 - p0
    T e1, ie0, ie1, ie2;                       // |p2 - p1|^2 and td_inv of the three squared edge lengths (edge 0: abab, edge 2: acac)
};

template <typename T>
__device__ inline void td_query(const T* p, TdQuery<T>& q) {
    load_tri9(p, q.raw);
    tri_box(q.raw, q.lo, q.hi);
    tri_normal(q.raw, q.n);
    q.usable = normal_usable(q.n);
    const Td3<T> zero = { T(0), T(0), T(0) };
    q.face = td_face(zero, Td3<T>{ q.raw[3] - q.raw[0], q.raw[4] - q.raw[1], q.raw[5] - q.raw[2] },
                     Td3<T>{ q.raw[6] - q.raw[0], q.raw[7] - q.raw[1], q.raw[8] - q.raw[2] });
    const Td3<T> bc = td_sub(q.face.ac, q.face.ab);
    q.e1 = td_dot(bc, bc);
    q.ie0 = td_inv(q.face.abab); q.ie1 = td_inv(q.e1); q.ie2 = td_inv(q.face.acac);
}

// Squared distance between the query triangle q and the triangle b (both closed sets, either of them possibly a segment or a point),
// with the barycentrics of the closest pair: (u, v) on b, (s, w) on q, tri_dist2's convention on both.
//   * 0 for every pair tri_pair_intersects accepts (run first, on the raw vertices of both: this query and bvh3X_intersect_tris
//     cannot disagree). The barycentrics are then those of the nearest candidate pair below, which names a common point up to the
//     rounding of the coordinates: a point where an edge of one crosses or touches the face of the other, or where two edges cross.
//   * Otherwise the smallest of 15 candidates, ties to the first: the 9 pairs of edges (td_segment_pair), and per triangle its 3
//     edges against the other's face (td_edges_to_face: the 6 vertex / face pairs, a vertex replaced by the crossing point of its
//     edge where there is one; that candidate is what makes a SEGMENT through a triangle's interior come out at distance ~ 0, a case
//     the pair test, which refuses triangles without area, does not see).
// Everything but the pair test runs in a local frame with the query's p0 as origin: the differences are exact up to the rounding of
// a coordinate DIFFERENCE, so a pair of unit size 4,000 units from the origin loses nothing to its position. Every candidate's
// distance is that of two points rebuilt from its parameters, which are clamped to their edge or tested to lie in their face: a
// rounding accident can make the result a little too large, never name a point outside a triangle. Never NaN for finite input:
// every division is by a quantity tested positive (td_inv, den > 0) or by ha - hb of two heights of strictly opposite sign, and
// whatever 0 * inf a denormal edge length produces is clamped to 0 (td_clamp01) or fails the face's comparisons; candidates are
// taken on d2 < best, which a NaN fails. With infinite coordinates the result is kMax or some non-NaN value.
template <typename T>
__device__ inline T tri_tri_dist2(const TdQuery<T>& q, const T (&b)[9], T& u, T& v, T& s, T& w) {
    const bool hit = q.usable && tri_pair_intersects(q.raw, q.lo, q.hi, q.n, b, false);
    const Td3<T> b0 = { b[0] - q.raw[0], b[1] - q.raw[1], b[2] - q.raw[2] };
    const Td3<T> b1 = { b[3] - q.raw[0], b[4] - q.raw[1], b[5] - q.raw[2] };
    const Td3<T> b2 = { b[6] - q.raw[0], b[7] - q.raw[1], b[8] - q.raw[2] };
    const TdFace<T> fb = td_face(b0, b1, b2);
    const Td3<T> bbc = td_sub(b2, b1);
    const T be1 = td_dot(bbc, bbc);

    T best = Num<T>::kMax;
    u = T(0); v = T(0); s = T(0); w = T(0);

    // the 9 pairs of edges: query edge i (rotating qa, qb, qc), tree edge j (rotating ta, tb, tc)
    {
        Td3<T> qa = q.face.o, qb = q.face.ab, qc = q.face.ac;
        T qe = q.face.abab, qe_next = q.e1, qe_last = q.face.acac, qi = q.ie0, qi_next = q.ie1, qi_last = q.ie2;
        Td3<T> ta = b0, tb = b1, tc = b2;
        T te = fb.abab, te_next = be1, te_last = fb.acac, ti = td_inv(fb.abab), ti_next = td_inv(be1), ti_last = td_inv(fb.acac);
        for (int i = 0; i < 3; ++i) {
            const Td3<T> d1 = td_sub(qb, qa);
            for (int j = 0; j < 3; ++j) {
                T es, et;
                const T d2 = td_segment_pair(qa, d1, qe, qi, ta, td_sub(tb, ta), te, ti, es, et);
                if (d2 < best) { best = d2; td_edge_uv(j, et, u, v); td_edge_uv(i, es, s, w); }
                const Td3<T> t0 = ta;
                ta = tb; tb = tc; tc = t0;
                const T e0 = te, i0 = ti;
                te = te_next; te_next = te_last; te_last = e0;
                ti = ti_next; ti_next = ti_last; ti_last = i0;
            }
            const Td3<T> q0 = qa;
            qa = qb; qb = qc; qc = q0;
            const T e0 = qe, i0 = qi;
            qe = qe_next; qe_next = qe_last; qe_last = e0;
            qi = qi_next; qi_next = qi_last; qi_last = i0;
        }
    }
    // the query's edges (vertices, crossing points) against the tree triangle's face, then the other way round
    td_edges_to_face(q.face.o, q.face.ab, q.face.ac, fb, [&](T d2, T fu, T fv, int k, T x) {
        if (d2 < best) { best = d2; u = fu; v = fv; td_edge_uv(k, x, s, w); }
    });
    td_edges_to_face(b0, b1, b2, q.face, [&](T d2, T fu, T fv, int k, T x) {
        if (d2 < best) { best = d2; s = fu; w = fv; td_edge_uv(k, x, u, v); }
    });
    return hit ? T(0) : best;
}

// Squared distance between two boxes {lo, hi}: per axis the gap max(0, lo_a - hi_b, lo_b - hi_a). A lower bound of the distance
// between anything in the one and anything in the other. No NaN leaves the selects: a NaN difference loses `x > y` or `m > 0`, and
// the gap is then the other difference's or 0, still a lower bound.
template <typename T>
__device__ inline T td_axis_gap(T alo, T ahi, T blo, T bhi) {
    const T x = alo - bhi, y = blo - ahi;
    const T m = x > y ? x : y;
    return m > T(0) ? m : T(0);
}
template <typename T>
__device__ inline T box_box_dist2(const T (&b)[6], const T (&lo)[3], const T (&hi)[3]) {
    const T e0 = td_axis_gap(b[0], b[1], lo[0], hi[0]), e1 = td_axis_gap(b[2], b[3], lo[1], hi[1]), e2 = td_axis_gap(b[4], b[5], lo[2], hi[2]);
    return dot3(e0, e1, e2, e0, e1, e2);
}

// One query, one lane: nearest_walk keyed by the squared distance between a child's box and the query triangle's box (computed once),
// with `best` (at first max_distance^2) as its limit: a child is entered iff key <= best, the nearer one first, the other stacked
// with its key. A leaf triangle is first rejected by the same key, its box taken from its three vertices, then measured by
// tri_tri_dist2. It lowers best on d2 < best || (d2 == best && i < best_prim): among the triangles the walk TESTS, the lowest
// BVH-order index of those at the smallest computed squared distance wins, whatever the visiting order; the walk does not stop at
// best == 0, because that rule needs every overlapping leaf. A subtree is skipped when its key exceeds best, so, as in
// closest_body.inc, a triangle whose computed distance rounds BELOW the key of its own leaf's box can hide one at an equal or
// one-ulp-nearer distance in another leaf: the record is the brute force's (argmin by (d2, index)) exactly when the distances are
// computed exactly, otherwise its distance is within the tolerance of INTEGRATION.md 3m of it.
// The invariant of nearest_walk.inc holds: a child is entered only on `key <= best`, which a NaN key fails; best starts as
// max_distance^2 of a query whose max_distance >= 0 (a NaN or negative one, or a NaN coordinate, is not walked: the miss record
// {BVH_AMD_INVALID, max_distance, 0, 0} and query barycentrics 0), and is lowered only to a d2 that passed d2 < best or d2 == best.
// Slot `slot` of the launch (query order[slot], or slot itself); `lane` indexes the HBM spill (Deep), `tid` the LDS arrays.
// cnt += {pair records fetched, leaf triangles visited (box-rejected ones included), leaves visited}.
template <typename T, bool Stats, bool Deep>
__device__ inline void tri_distance_lane(const TriDistanceArgs<T>& a, unsigned long long slot, uint32_t* lds_node, T* lds_d2, int tid,
                                         unsigned long long lane, unsigned long long (&cnt)[3]) {
    const unsigned long long qi = a.order ? a.order[slot] : slot;
    TdQuery<T> q;
    td_query(a.queries + 9ull * qi, q);
    const T max_d = a.max_distances ? a.max_distances[qi] : a.max_distance;
    bool valid = max_d >= T(0);
#pragma unroll
    for (int k = 0; k < 9; ++k) valid = valid && q.raw[k] == q.raw[k];
    uint32_t best_prim = BVH_AMD_INVALID;
    T best = max_d * max_d, best_u = T(0), best_v = T(0), best_s = T(0), best_w = T(0);

    nearest_walk<T, kClosestLds, Stats, Deep>(a, valid, lds_node, lds_d2, uint32_t(kBlock), tid, lane, a.deep_d2, best, cnt,
        [&](const T (&lb)[6], const T (&rb)[6], T& dl, T& dr, bool& hl, bool& hr) {
            dl = box_box_dist2(lb, q.lo, q.hi); dr = box_box_dist2(rb, q.lo, q.hi);
            hl = dl <= best; hr = dr <= best;
        },
        [&](uint32_t i) {
            T b[9], blo[3], bhi[3];
            load_tri9(a.prims + 9ull * a.tri_ids[i], b);
            tri_box(b, blo, bhi);
            const T bb[6] = { blo[0], bhi[0], blo[1], bhi[1], blo[2], bhi[2] };
            if (!(box_box_dist2(bb, q.lo, q.hi) <= best)) return;
            T u, v, s, w;
            const T d2 = tri_tri_dist2(q, b, u, v, s, w);
            if (d2 < best || (d2 == best && i < best_prim)) { best = d2; best_prim = i; best_u = u; best_v = v; best_s = s; best_w = w; }
        });
    if (best_prim != BVH_AMD_INVALID) store_hit(a.hits + qi, a.prim_ids ? a.prim_ids[best_prim] : best_prim, Num<T>::sqrt_(best), best_u, best_v);
    else store_hit(a.hits + qi, BVH_AMD_INVALID, max_d, T(0), T(0));
    if (a.query_uv) {
        store_stream(a.query_uv + 2ull * qi, best_s);
        store_stream(a.query_uv + 2ull * qi + 1, best_w);
    }
}

} // namespace

} // namespace bvh_amd
