// Per-lane body of the batched sphere-cast query (sphere_cast.hip): a ball of radius r whose centre moves along c(t) = org + t dir,
// t in [tmin, tmax], and the smallest t at which it touches the scene: dist(c(t), primitive) <= r (closed), over solid triangles
// (PrecomputedTri) or solid spheres. It is the third client of nearest_walk.inc, next to closest_body.inc and ray_nearest_body.inc:
// the key of a box is the t at which the ray enters the box GROWN by r on every side (slab_pair, trace_device.h), the limit is the
// best contact so far, and the leaf test is the sweep test below; the LDS tier of the stack is closest-point's (nearest_walk.inc:
// kClosestLds) and the record leaves through point_walk.inc's store_record. Kept as an include so that
// tests/cpp/sphere_cast_body_host.cpp compiles the very same text for the host (one emulated lane per query). Expects what
// point_walk.inc expects.
#pragma once

#include "nearest_walk.inc"

namespace bvh_amd {

namespace {

template <typename T>
struct SphereCastArgs : PointArgs<T> {         // queries = rays, 8 scalars each
    typename HitOf<T>::Type* hits;             // one record per query, caller order
    T* deep_t;                                 // Deep kernels only: beside deep_nodes
    const T* radii;                            // optional: one radius per query, caller order
    T radius;                                  // the batch's radius when radii is null
};

// Where the moving point m + x d enters the ball |.| <= r about the origin (dd = d.d, r2 = r^2): from the point of its path nearest
// to the origin, q = m + x0 d, back by sqrt((r^2 - |q|^2) / d.d). The geometric form of the smaller root of
// d.d x^2 + 2 m.d x + m.m - r^2 = 0, taken because it loses nothing to the size of m: the quadratic's m.m - r^2 and its
// discriminant cancel to an absolute error of eps |m|^2, which put the contact of a float32 ball 4,000 units away off by more than a
// unit, and that of a ball of radius 0.0035 with an edge 2 units long off by 2 % of the radius; here the error of |q| is eps |m|,
// that of the coordinates themselves. False for dd <= 0 (no motion) and for a path that stays outside. A NaN fails every comparison.
template <typename T>
__device__ inline bool sweep_enter(const T (&m)[3], const T (&d)[3], T dd, T r2, T& x) {
    if (!(dd > T(0))) return false;
    const T x0 = -dot3(m[0], m[1], m[2], d[0], d[1], d[2]) / dd;
    const T q[3] = { m[0] + x0 * d[0], m[1] + x0 * d[1], m[2] + x0 * d[2] };
    const T h2 = r2 - dot3(q[0], q[1], q[2], q[0], q[1], q[2]);
    if (!(h2 >= T(0))) return false;
    x = x0 - Num<T>::sqrt_(h2 / dd);
    return true;
}

// First contact of the ball with the solid triangle p on t in [tmin, limit]: true, and t with the barycentrics (u, v) of the contact
// point (point = p0 - u e1 + v e2, tri_dist2's convention), or false. c0 = c(tmin) = org + tmin * dir, computed by the caller; a
// candidate is tau = t - tmin >= 0.
// The triangle grown by the ball is the union of a face prism, three edge cylinders and three vertex balls, so the first contact is
// the smallest of these candidates, ties to the first of them in this order:
//   start    tri_dist2(c0) <= r^2: t = tmin (an initial overlap), with tri_dist2's (u, v);
//   face     only while the centre approaches the plane: s = sign(n.(c0 - p0)), s (n.dir) < 0, and it starts outside the slab
//            |n.(c - p0)| <= r |n| (inside it, a face contact is the start's, or an edge's comes first). The root of
//            n.(c(t) - p0) = s r |n| counts only if the foot of c(t) has barycentrics inside the triangle (the 2 x 2 system of
//            tri_dist2, which ignores the normal part) AND the point rebuilt from them is within r + slop of c(t),
//            slop = 32 eps (sum |c_k| + sum |p0_k| + r). Without the distance condition a triangle collinear up to rounding, whose
//            normal and barycentrics are noise, reports contacts with a plane it does not lie in. The approach condition saves
//            work and decides nothing: the root it excludes is where a centre inside the slab LEAVES it, and a centre that gets
//            there over the triangle has met the start, an edge or a vertex candidate at a smaller t;
//   edges    the ray against the infinite cylinder of radius r around AB, AC, BC: sweep_enter of the parts of c0 - a and dir
//            perpendicular to the edge, iff the contact's parameter along the edge is in [0, 1]. A zero-length edge is skipped,
//            and so is a direction parallel to the edge: |dir_perp|^2 <= 64 eps^2 |dir|^2, what rounding leaves of a parallel one;
//   vertices sweep_enter of the ray against the ball of radius r at A, B, C.
// Edge and vertex candidates are points of the triangle by construction. Ahead of all of them, a rejection along the axis n (any
// vector serves as a separating axis, so a noise normal is safe): the triangle projects onto [hmin, hmax] (its three vertices), the
// centre's path onto [g0, g1]; if the two stay more than r |n| apart, rounding slop included, nothing can touch.
// Never NaN for finite input.
template <typename T>
__device__ inline bool sphere_cast_tri(const T (&p)[12], const T (&org)[3], const T (&c0)[3], const T (&dir)[3], T tmin, T limit, T r,
                                       T& t, T& u, T& v) {
    if (!(tmin <= limit)) return false;
    const T ab[3] = { -p[3], -p[4], -p[5] }, ac[3] = { p[6], p[7], p[8] };
    const T n[3] = { p[9], p[10], p[11] };
    const T ap[3] = { c0[0] - p[0], c0[1] - p[1], c0[2] - p[2] };
    const T span = limit - tmin;
    const T nn = dot3(n[0], n[1], n[2], n[0], n[1], n[2]);
    const T rn = r * Num<T>::sqrt_(nn);
    const T nd = dot3(n[0], n[1], n[2], dir[0], dir[1], dir[2]);
    const T g0 = dot3(n[0], n[1], n[2], ap[0], ap[1], ap[2]);
    {
        const T c1[3] = { c0[0] + span * dir[0], c0[1] + span * dir[1], c0[2] + span * dir[2] };
        const T g1 = dot3(n[0], n[1], n[2], c1[0] - p[0], c1[1] - p[1], c1[2] - p[2]);
        const T hb = dot3(n[0], n[1], n[2], ab[0], ab[1], ab[2]), hc = dot3(n[0], n[1], n[2], ac[0], ac[1], ac[2]);
        const T hmax = pick_max(pick_max(hb, hc), T(0)), hmin = pick_min(pick_min(hb, hc), T(0));
        T w = T(0);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            w += Num<T>::abs_(n[k]) * (((Num<T>::abs_(org[k]) + Num<T>::abs_(c0[k])) + Num<T>::abs_(c1[k])) + ((Num<T>::abs_(p[k]) + Num<T>::abs_(ab[k])) + Num<T>::abs_(ac[k])));
        const T reach = rn + T(8) * Num<T>::kEps * w;
        if ((g0 > hmax + reach && g1 > hmax + reach) || (g0 < hmin - reach && g1 < hmin - reach)) return false;
    }

    const T r2 = r * r;
    T tu = T(0), tv = T(0);
    if (tri_dist2(p, c0, tu, tv) <= r2) { t = tmin; u = tu; v = tv; return true; }

    bool found = false;
    T best = limit;
    auto offer = [&](T tau, T cu, T cv) {
        const T tc = tmin + tau;
        if (found ? tc < best : tc <= best) { best = tc; u = cu; v = cv; found = true; }
    };

    const T abab = dot3(ab[0], ab[1], ab[2], ab[0], ab[1], ab[2]), acac = dot3(ac[0], ac[1], ac[2], ac[0], ac[1], ac[2]);
    const T abac = dot3(ab[0], ab[1], ab[2], ac[0], ac[1], ac[2]);
    const T s = g0 > T(0) ? T(1) : T(-1);
    if (nn > T(0) && g0 != T(0) && s * nd < T(0)) {                    // face
        const T tau = (s * rn - g0) / nd;
        const T det = abab * acac - abac * abac;
        if (tau >= T(0) && tmin + tau <= best && det > T(0)) {
            const T c[3] = { c0[0] + tau * dir[0], c0[1] + tau * dir[1], c0[2] + tau * dir[2] };
            const T cp[3] = { c[0] - p[0], c[1] - p[1], c[2] - p[2] };
            const T cpab = dot3(cp[0], cp[1], cp[2], ab[0], ab[1], ab[2]), cpac = dot3(cp[0], cp[1], cp[2], ac[0], ac[1], ac[2]);
            const T fu = (acac * cpab - abac * cpac) / det, fv = (abab * cpac - abac * cpab) / det;
            if (fu >= T(0) && fv >= T(0) && fu + fv <= T(1)) {
                const T d0 = (cp[0] - fu * ab[0]) - fv * ac[0], d1 = (cp[1] - fu * ab[1]) - fv * ac[1], d2 = (cp[2] - fu * ab[2]) - fv * ac[2];
                const T mag = ((Num<T>::abs_(c[0]) + Num<T>::abs_(c[1])) + Num<T>::abs_(c[2])) + ((Num<T>::abs_(p[0]) + Num<T>::abs_(p[1])) + Num<T>::abs_(p[2])) + r;
                const T rs = r + T(32) * Num<T>::kEps * mag;
                if (dot3(d0, d1, d2, d0, d1, d2) <= rs * rs) offer(tau, fu, fv);
            }
        }
    }

    const T dd = dot3(dir[0], dir[1], dir[2], dir[0], dir[1], dir[2]);
    const T bp[3] = { ap[0] - ab[0], ap[1] - ab[1], ap[2] - ab[2] };                    // c0 - B
    const T cp[3] = { ap[0] - ac[0], ap[1] - ac[1], ap[2] - ac[2] };                    // c0 - C
    const T bc[3] = { ac[0] - ab[0], ac[1] - ab[1], ac[2] - ab[2] };
    // the cylinder around the edge {a, a + e}, m = c0 - a: the ball of radius r met by the parts of m and dir perpendicular to e
    auto edge = [&](const T (&m)[3], const T (&e)[3], T ee, int which) {
        if (!(ee > T(0))) return;
        const T me = dot3(m[0], m[1], m[2], e[0], e[1], e[2]) / ee, de = dot3(dir[0], dir[1], dir[2], e[0], e[1], e[2]) / ee;
        const T mp[3] = { m[0] - me * e[0], m[1] - me * e[1], m[2] - me * e[2] };
        const T dp[3] = { dir[0] - de * e[0], dir[1] - de * e[1], dir[2] - de * e[2] };
        const T dpdp = dot3(dp[0], dp[1], dp[2], dp[0], dp[1], dp[2]);
        T x;
        if (!(dpdp > T(64) * Num<T>::kEps * Num<T>::kEps * dd) || !sweep_enter(mp, dp, dpdp, r2, x)) return;
        const T w = me + x * de;
        if (!(w >= T(0) && w <= T(1)) || !(x >= T(0))) return;
        if (which == 0) offer(x, w, T(0));
        else if (which == 1) offer(x, T(0), w);
        else offer(x, T(1) - w, w);
    };
    edge(ap, ab, abab, 0);
    edge(ap, ac, acac, 1);
    edge(bp, bc, dot3(bc[0], bc[1], bc[2], bc[0], bc[1], bc[2]), 2);

    T x;
    if (sweep_enter(ap, dir, dd, r2, x) && x >= T(0)) offer(x, T(0), T(0));          // A
    if (sweep_enter(bp, dir, dd, r2, x) && x >= T(0)) offer(x, T(1), T(0));          // B
    if (sweep_enter(cp, dir, dd, r2, x) && x >= T(0)) offer(x, T(0), T(1));          // C

    t = best;
    return found;
}

// First contact of the ball with the solid sphere {centre, R}: the ray against the ball of radius R + r, t = tmin when c0 is in it.
template <typename T>
__device__ inline bool sphere_cast_sphere(const T (&sp)[4], const T (&c0)[3], const T (&dir)[3], T tmin, T limit, T r, T& t) {
    if (!(tmin <= limit)) return false;
    const T m[3] = { c0[0] - sp[0], c0[1] - sp[1], c0[2] - sp[2] };
    const T rr = sp[3] + r, rr2 = rr * rr;
    if (dot3(m[0], m[1], m[2], m[0], m[1], m[2]) <= rr2) { t = tmin; return true; }
    T x;
    if (!sweep_enter(m, dir, dot3(dir[0], dir[1], dir[2], dir[0], dir[1], dir[2]), rr2, x) || !(x >= T(0))) return false;
    t = tmin + x;
    return t <= limit;
}

// The sweep test on BVH-order primitive i; (u, v) = 0 for a sphere.
template <typename T, int Leaf>
__device__ inline bool sphere_cast_test(const T* prims, uint32_t i, const T (&org)[3], const T (&c0)[3], const T (&dir)[3], T tmin, T limit, T r,
                                        T& t, T& u, T& v) {
    if (Leaf == LEAF_TRIANGLE) {
        T p[12];
        load_prim12(prims + 12ull * i, p);
        return sphere_cast_tri(p, org, c0, dir, tmin, limit, r, t, u, v);
    }
    T s[4];
    load_prim4(prims + 4ull * i, s);
    u = T(0); v = T(0);
    return sphere_cast_sphere(s, c0, dir, tmin, limit, r, t);
}

// One query, one lane: nearest_walk keyed by the t at which the ray enters a child's box grown by r on every side, with `best` (at
// first the ray's tmax) as its limit: both grown boxes are tested by slab_pair against [tmin, best], a child is entered iff
// l0 <= l1, of two entered children the one entered first is taken and the other stacked with its entry t. A primitive lowers best
// on t < best || (t == best && i < best_prim): among the primitives the walk TESTS, the lowest BVH-order index of those at the
// smallest computed t wins, whatever the visiting order. A subtree is skipped when the computed entry t of its grown box exceeds
// best (or the slab test, whose grown bounds b -+ r are themselves rounded, misses it), so a primitive whose computed contact t
// rounds below the entry t of its own leaf's box can hide one at an equal or one-ulp-earlier t in another leaf, as in
// closest_body.inc: the record is the brute force's (argmin by (t, index)) exactly when the arithmetic is exact, otherwise its
// residual |dist(c(t), prim) - r| is within the tolerance of INTEGRATION.md 3l.
// A NaN tmin or tmax, a NaN or negative radius: not walked, the miss record {BVH_AMD_INVALID, tmax, 0, 0}. Slot `slot` of the
// launch (ray order[slot], or slot itself); `lane` indexes the HBM spill (Deep), `tid` the LDS arrays.
// cnt += {pair records fetched, primitives tested, leaves visited}.
template <typename T, int Leaf, bool Robust, bool Stats, bool Deep>
__device__ inline void sphere_cast_lane(const SphereCastArgs<T>& a, unsigned long long slot, uint32_t* lds_node, T* lds_t, int tid,
                                        unsigned long long lane, unsigned long long (&cnt)[3]) {
    const unsigned long long qi = a.order ? a.order[slot] : slot;
    T r[8];
    load_ray(a.queries + 8ull * qi, r);
    const T org[3] = { r[0], r[1], r[2] }, dir[3] = { r[3], r[4], r[5] };
    const T tmin = r[6], ray_tmax = r[7];
    const T rad = a.radii ? a.radii[qi] : a.radius;
    T inv[3], aux[3];
    uint32_t oct[3];
    ray_constants<T, Robust, 3>(org, dir, inv, aux, oct);
    const bool valid = tmin == tmin && ray_tmax == ray_tmax && rad >= T(0);
    const T c0[3] = { org[0] + tmin * dir[0], org[1] + tmin * dir[1], org[2] + tmin * dir[2] };
    uint32_t best_prim = BVH_AMD_INVALID;
    T best = ray_tmax, best_u = T(0), best_v = T(0);

    nearest_walk<T, kClosestLds, Stats, Deep>(a, valid, lds_node, lds_t, uint32_t(kBlock), tid, lane, a.deep_t, best, cnt,
        [&](const T (&lb)[6], const T (&rb)[6], T& l0, T& r0, bool& hl, bool& hr) {
            const T gl[6] = { lb[0] - rad, lb[1] + rad, lb[2] - rad, lb[3] + rad, lb[4] - rad, lb[5] + rad };
            const T gr[6] = { rb[0] - rad, rb[1] + rad, rb[2] - rad, rb[3] + rad, rb[4] - rad, rb[5] + rad };
            T l1, r1;
            slab_pair<T, Robust, 3>(gl, gr, org, inv, aux, oct, tmin, best, l0, l1, r0, r1);
            hl = l0 <= l1; hr = r0 <= r1;
        },
        [&](uint32_t i) {
            T t = T(0), u = T(0), v = T(0);
            if (sphere_cast_test<T, Leaf>(a.prims, i, org, c0, dir, tmin, best, rad, t, u, v) && (t < best || (t == best && i < best_prim))) {
                best = t; best_prim = i; best_u = u; best_v = v;
            }
        });
    if (best_prim != BVH_AMD_INVALID) store_record(a.hits + qi, a.prim_ids ? a.prim_ids[best_prim] : best_prim, best, best_u, best_v);
    else store_record(a.hits + qi, BVH_AMD_INVALID, ray_tmax, T(0), T(0));
}

} // namespace

} // namespace bvh_amd
