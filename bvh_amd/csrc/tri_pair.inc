// The triangle helpers and the sign-only pair test that tri_intersect_body.inc (every match of a walk) and tri_distance_body.inc
// (which pairs are at distance 0) share: a triangle of 9 scalars {p0, p1, p2} of the caller's arrays, its box and normal, and
// tri_pair_intersects. The test (closed sets: touching counts, and so does coplanar containment) is described at the head of
// tri_intersect_body.inc. Kept as an include so that tests/cpp/tri_intersect_body_host.cpp and tri_distance_body_host.cpp compile the
// very same text for the host, through the bodies. Expects point_walk.inc (box_overlaps) and what it expects.
#pragma once

#include "point_walk.inc"

namespace bvh_amd {

namespace {

// A triangle {p0.xyz, p1.xyz, p2.xyz} of the caller's arrays (aligned to its scalar only).
// (Every index into a lane's arrays below is written out as a constant, without loops: where a select between elements of an array
//  meets an index that is constant only after unrolling, the compiler turns the select into an indexed load and the array into scratch.)
template <typename T>
__device__ inline void load_tri9(const T* p, T (&v)[9]) {
    v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
    v[3] = p[3]; v[4] = p[4]; v[5] = p[5];
    v[6] = p[6]; v[7] = p[7]; v[8] = p[8];
}

template <typename T>
__device__ inline void min_max3(T a, T b, T c, T& lo, T& hi) {
    const T mn = b < a ? b : a, mx = b > a ? b : a;
    lo = c < mn ? c : mn;
    hi = c > mx ? c : mx;
}

template <typename T>
__device__ inline void tri_box(const T (&v)[9], T (&lo)[3], T (&hi)[3]) {
    min_max3(v[0], v[3], v[6], lo[0], hi[0]);
    min_max3(v[1], v[4], v[7], lo[1], hi[1]);
    min_max3(v[2], v[5], v[8], lo[2], hi[2]);
}

// (p1 - p0) x (p2 - p0): three 2 x 2 determinants of coordinate differences.
template <typename T>
__device__ inline void tri_normal(const T (&v)[9], T (&n)[3]) {
    const T e1[3] = { v[3] - v[0], v[4] - v[1], v[5] - v[2] }, e2[3] = { v[6] - v[0], v[7] - v[1], v[8] - v[2] };
    n[0] = e1[1] * e2[2] - e1[2] * e2[1];
    n[1] = e1[2] * e2[0] - e1[0] * e2[2];
    n[2] = e1[0] * e2[1] - e1[1] * e2[0];
}

// A triangle whose computed normal is (0, 0, 0) (no area), or has a NaN or infinite component (any NaN or infinite coordinate ends up
// there), intersects nothing.
template <typename T>
__device__ inline bool normal_usable(const T (&n)[3]) {
    return Num<T>::finite(n[0]) && Num<T>::finite(n[1]) && Num<T>::finite(n[2]) && (n[0] != T(0) || n[1] != T(0) || n[2] != T(0));
}

template <typename T>
__device__ inline int sign_of(T x) { return int(x > T(0)) - int(x < T(0)); }

// The side of point p against the plane through o with normal n: (p - o) . n, a 3 x 3 determinant of differences.
template <typename T>
__device__ inline int plane_side(const T* p, const T* o, const T (&n)[3]) {
    return sign_of(dot3(p[0] - o[0], p[1] - o[1], p[2] - o[2], n[0], n[1], n[2]));
}

// det [a - d, b - d, c - d] = (a - d) . ((b - d) x (c - d)): negative iff d lies above the plane of a, b, c (on the side its normal
// (b - a) x (c - a) points to), zero iff on it.
template <typename T>
__device__ inline T orient3(const T (&a)[3], const T (&b)[3], const T (&c)[3], const T (&d)[3]) {
    const T u[3] = { a[0] - d[0], a[1] - d[1], a[2] - d[2] }, v[3] = { b[0] - d[0], b[1] - d[1], b[2] - d[2] }, w[3] = { c[0] - d[0], c[1] - d[1], c[2] - d[2] };
    return dot3(u[0], u[1], u[2], v[1] * w[2] - v[2] * w[1], v[2] * w[0] - v[0] * w[2], v[0] * w[1] - v[1] * w[0]);
}

// Some vertex of a equals some vertex of b on all three coordinates (==: -0 equals +0, a NaN equals nothing).
template <typename T>
__device__ inline bool same_point(T ax, T ay, T az, T bx, T by, T bz) { return ax == bx && ay == by && az == bz; }
template <typename T>
__device__ inline bool shares_vertex(const T (&a)[9], const T (&b)[9]) {
    return same_point(a[0], a[1], a[2], b[0], b[1], b[2]) || same_point(a[0], a[1], a[2], b[3], b[4], b[5]) || same_point(a[0], a[1], a[2], b[6], b[7], b[8]) ||
           same_point(a[3], a[4], a[5], b[0], b[1], b[2]) || same_point(a[3], a[4], a[5], b[3], b[4], b[5]) || same_point(a[3], a[4], a[5], b[6], b[7], b[8]) ||
           same_point(a[6], a[7], a[8], b[0], b[1], b[2]) || same_point(a[6], a[7], a[8], b[3], b[4], b[5]) || same_point(a[6], a[7], a[8], b[6], b[7], b[8]);
}

// The signs of a triangle's vertices against the other's plane are neither all zero nor all of one strict sign: one vertex then stands
// alone, with the other two on the closed other side. k = that vertex (the first that qualifies), below = it is the one on the
// non-positive side: {+; <= 0, <= 0} and {0; -, -} stand alone above, {-; >= 0, >= 0} and {0; +, +} below.
__device__ inline void alone_vertex(int s0, int s1, int s2, int& k, bool& below) {
    const bool up0 = (s0 > 0 && s1 <= 0 && s2 <= 0) || (s0 == 0 && s1 < 0 && s2 < 0), dn0 = (s0 < 0 && s1 >= 0 && s2 >= 0) || (s0 == 0 && s1 > 0 && s2 > 0);
    const bool up1 = (s1 > 0 && s2 <= 0 && s0 <= 0) || (s1 == 0 && s2 < 0 && s0 < 0), dn1 = (s1 < 0 && s2 >= 0 && s0 >= 0) || (s1 == 0 && s2 > 0 && s0 > 0);
    const bool dn2 = (s2 < 0 && s0 >= 0 && s1 >= 0) || (s2 == 0 && s0 > 0 && s1 > 0);
    const bool at0 = up0 || dn0, at1 = up1 || dn1;
    k = at0 ? 0 : at1 ? 1 : 2;
    below = at0 ? dn0 : at1 ? dn1 : dn2;
}

// Vertex k, k + 1, k + 2 (cyclic: the orientation is kept) of a triangle, the last two exchanged when `flip` (the orientation reversed).
template <typename T>
__device__ inline void rotated1(T x0, T x1, T x2, int k, bool flip, T& p, T& q, T& r) {      // one coordinate of the three vertices
    const T y1 = k == 0 ? x1 : k == 1 ? x2 : x0, y2 = k == 0 ? x2 : k == 1 ? x0 : x1;
    p = k == 0 ? x0 : k == 1 ? x1 : x2;
    q = flip ? y2 : y1;
    r = flip ? y1 : y2;
}
template <typename T>
__device__ inline void rotated(const T (&v)[9], int k, bool flip, T (&p)[3], T (&q)[3], T (&r)[3]) {
    rotated1(v[0], v[3], v[6], k, flip, p[0], q[0], r[0]);
    rotated1(v[1], v[4], v[7], k, flip, p[1], q[1], r[1]);
    rotated1(v[2], v[5], v[8], k, flip, p[2], q[2], r[2]);
}

// The edge a -> b of a triangle, in the projection: whether all three points (px, py) lie strictly on its outer side, which is the right
// of a counter-clockwise triangle and the left of a clockwise one (cw).
template <typename T>
__device__ inline bool outside_edge(T ax, T ay, T bx, T by, bool cw, T px, T py) {
    const T d = (bx - ax) * (py - ay) - (by - ay) * (px - ax);
    return cw ? d > T(0) : d < T(0);
}
template <typename T>
__device__ inline bool edge_separates(T ax, T ay, T bx, T by, bool cw, const T (&px)[3], const T (&py)[3]) {
    return outside_edge(ax, ay, bx, by, cw, px[0], py[0]) && outside_edge(ax, ay, bx, by, cw, px[1], py[1]) && outside_edge(ax, ay, bx, by, cw, px[2], py[2]);
}

// Coplanar triangles, projected along the largest component of a's normal (the first of equals): two closed convex polygons are
// disjoint iff the line through an edge of one has the other strictly on its outer side. Each triangle's winding is the sign of its
// own normal's component along the projection.
template <typename T>
__device__ inline bool coplanar_intersects(const T (&a)[9], const T (&na)[3], const T (&b)[9], const T (&nb)[3]) {
    const T m0 = Num<T>::abs_(na[0]), m1 = Num<T>::abs_(na[1]), m2 = Num<T>::abs_(na[2]);
    const int m = (m0 >= m1 && m0 >= m2) ? 0 : m1 >= m2 ? 1 : 2;
    // axes (m + 1, m + 2) mod 3, in this order: a winds counter-clockwise iff na[m] > 0
    auto first = [m](T x, T y, T z) { return m == 0 ? y : m == 1 ? z : x; };
    auto second = [m](T x, T y, T z) { return m == 0 ? z : m == 1 ? x : y; };
    const T ax[3] = { first(a[0], a[1], a[2]), first(a[3], a[4], a[5]), first(a[6], a[7], a[8]) };
    const T ay[3] = { second(a[0], a[1], a[2]), second(a[3], a[4], a[5]), second(a[6], a[7], a[8]) };
    const T bx[3] = { first(b[0], b[1], b[2]), first(b[3], b[4], b[5]), first(b[6], b[7], b[8]) };
    const T by[3] = { second(b[0], b[1], b[2]), second(b[3], b[4], b[5]), second(b[6], b[7], b[8]) };
    const bool a_cw = (m == 0 ? na[0] : m == 1 ? na[1] : na[2]) < T(0), b_cw = (m == 0 ? nb[0] : m == 1 ? nb[1] : nb[2]) < T(0);
    bool apart = false;
    apart |= edge_separates(ax[0], ay[0], ax[1], ay[1], a_cw, bx, by);
    apart |= edge_separates(ax[1], ay[1], ax[2], ay[2], a_cw, bx, by);
    apart |= edge_separates(ax[2], ay[2], ax[0], ay[0], a_cw, bx, by);
    apart |= edge_separates(bx[0], by[0], bx[1], by[1], b_cw, ax, ay);
    apart |= edge_separates(bx[1], by[1], bx[2], by[2], b_cw, ax, ay);
    apart |= edge_separates(bx[2], by[2], bx[0], by[0], b_cw, ax, ay);
    return !apart;
}

// Triangle a (vertices, box, usable normal na: the lane's query, prepared once) against triangle b, as fetched.
template <typename T>
__device__ inline bool tri_pair_intersects(const T (&a)[9], const T (&alo)[3], const T (&ahi)[3], const T (&na)[3], const T (&b)[9], bool skip_shared) {
    T blo[3], bhi[3];
    tri_box(b, blo, bhi);
    if (!box_overlaps(blo, bhi, alo, ahi)) return false;
    if (skip_shared && shares_vertex(a, b)) return false;
    T nb[3];
    tri_normal(b, nb);
    if (!normal_usable(nb)) return false;
    // the early-out most pairs leave by: one triangle strictly on one side of the other's plane
    const int sa0 = plane_side(&a[0], &b[0], nb), sa1 = plane_side(&a[3], &b[0], nb), sa2 = plane_side(&a[6], &b[0], nb);
    if ((sa0 > 0 && sa1 > 0 && sa2 > 0) || (sa0 < 0 && sa1 < 0 && sa2 < 0)) return false;
    const int sb0 = plane_side(&b[0], &a[0], na), sb1 = plane_side(&b[3], &a[0], na), sb2 = plane_side(&b[6], &a[0], na);
    if ((sb0 > 0 && sb1 > 0 && sb2 > 0) || (sb0 < 0 && sb1 < 0 && sb2 < 0)) return false;
    if ((sa0 | sa1 | sa2) == 0 || (sb0 | sb1 | sb2) == 0) return coplanar_intersects(a, na, b, nb);
    // Both triangles cross the line the planes share. Each is rotated so that its lone vertex comes first, and the OTHER one is
    // reversed when that vertex lies below: then p1 is above b's plane and p2 above a's, the intervals on the line are cut by the
    // edges p1q1, p1r1 and p2q2, p2r2 in one order, and they overlap iff neither begins behind the other's end: q2 is not above the
    // plane of p1, q1, p2, and p2 is not above the plane of p1, r1, r2.
    int ka = 0, kb = 0;
    bool a_below = false, b_below = false;
    alone_vertex(sa0, sa1, sa2, ka, a_below);
    alone_vertex(sb0, sb1, sb2, kb, b_below);
    T p1[3], q1[3], r1[3], p2[3], q2[3], r2[3];
    rotated(a, ka, b_below, p1, q1, r1);
    rotated(b, kb, a_below, p2, q2, r2);
    return orient3(p1, q1, p2, q2) >= T(0) && orient3(p1, r1, r2, p2) >= T(0);
}

} // namespace

} // namespace bvh_amd
