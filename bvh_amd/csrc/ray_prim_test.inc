// The leaf test of the ray queries that keep the ray UNSHORTENED (all-hits: the hit lambda of ray_hits_lane; nearest-hits:
// ray_nearest_test), on one BVH-order primitive: a PrecomputedTri through tri_test.inc (tri.h:56-74) or a Sphere {c, r} (sphere.h:32-49,
// as trace_body.inc writes it). In scope: T, Leaf, prims, i, org, dir, tmin, tmax (the includer's own copy of the ray's tmax for this
// one test: tri_test.inc writes it) and, written when the primitive is accepted, hit_t, hit_u, hit_v (a triangle's {t, u, v}, a
// sphere's {t0, t1 = min(exit, tmax), 0}) and accepted = true.
// Text, not a function, for tri_test.inc's reason: with the all-hits lambda calling a function the two sites shared, several
// ray_hits_kernel variants came out of register allocation differently; as text the compiler sees there what it saw before.
if (Leaf == LEAF_TRIANGLE) {
    T p[12];
    load_prim12(prims + 12ull * i, p);
#define BVH_TRI_ACCEPTED accepted = true
#include "tri_test.inc"
#undef BVH_TRI_ACCEPTED
} else {
    T s[4];
    load_prim4(prims + 4ull * i, s);
    const T o0 = org[0] - s[0], o1 = org[1] - s[1], o2 = org[2] - s[2];
    const T qa = dot3(dir[0], dir[1], dir[2], dir[0], dir[1], dir[2]);
    const T qb = T(2) * dot3(dir[0], dir[1], dir[2], o0, o1, o2);
    const T qc = dot3(o0, o1, o2, o0, o1, o2) - s[3] * s[3];
    const T delta = qb * qb - T(4) * qa * qc;
    if (delta >= 0) {
        const T iv = -T(0.5) / qa;
        const T root = Num<T>::sqrt_(delta);
        const T t0 = pick_max((qb + root) * iv, tmin);
        const T t1 = pick_min((qb - root) * iv, tmax);
        if (t0 <= t1) { hit_t = t0; hit_u = t1; hit_v = T(0); accepted = true; }
    }
}
