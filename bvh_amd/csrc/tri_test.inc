// The triangle test of the ray walks (tri.h:56-74 on one PrecomputedTri {p0, e1, e2, n}), one copy for trace_body.inc and
// instanced_body.inc. In scope: T, p[12], org, dir, tmin and, written in place when the hit is accepted, tmax, hit_t, hit_u, hit_v;
// BVH_TRI_ACCEPTED: the includer's statement that notes which primitive (and instance) it was.
// Text, not a function, because that is the shape that costs nothing: with the hit state passed by reference the instanced kernels
// come out of register allocation differently (two of them a wave per SIMD lower), a flag for the caller to branch on adds two selects
// and four mask operations per test there, and results handed back by value cost the batch kernels registers and scratch.
{
    const T c0 = p[0] - org[0], c1 = p[1] - org[1], c2 = p[2] - org[2];
    const T rx = dir[1] * c2 - dir[2] * c1, ry = dir[2] * c0 - dir[0] * c2, rz = dir[0] * c1 - dir[1] * c0;
    const T inv_det = T(1) / dot3(p[9], p[10], p[11], dir[0], dir[1], dir[2]);
    const T u = dot3(rx, ry, rz, p[6], p[7], p[8]) * inv_det;
    const T v = dot3(rx, ry, rz, p[3], p[4], p[5]) * inv_det;
    const T w = T(1) - u - v;
    const T tol = -Num<T>::kEps;
    if (u >= tol && v >= tol && w >= tol) {
        const T t = dot3(p[9], p[10], p[11], c0, c1, c2) * inv_det;
        if (t >= tmin && t <= tmax) { tmax = t; hit_t = t; hit_u = u; hit_v = v; BVH_TRI_ACCEPTED; }
    }
}
