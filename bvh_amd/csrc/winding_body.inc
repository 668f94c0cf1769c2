// Per-lane bodies of the winding-number queries (winding.hip): the generalized winding number of a triangle mesh at a point, evaluated
// hierarchically (Barill et al., "Fast Winding Numbers for Soups and Clouds", 2018, first order: one dipole per far node), and the
// per-node moments it needs. Three parts:
//   * wind_atan2: atan2 as plain arithmetic (no libm call: the device's bytes must equal this text compiled for the host);
//   * the moments: the fold of a leaf's triangles and the bottom-up climb over arrival tickets (as refit_body.inc climbs), from the
//     pair records alone: the tree is only read;
//   * the walk: one query per lane, depth-first, the left child before the right, nothing pruned against what was found.
// Kept as an include so that tests/cpp/winding_body_host.cpp compiles the very same text for the host (one emulated lane per query /
// per node). Expects what point_walk.inc expects and three hooks for the climb:
//   BVH_WIND_LOAD(ptr)         a scalar another climber may have written (device: agent-scope relaxed atomic load)
//   BVH_WIND_STORE(ptr, v)     a scalar another climber may read        (device: agent-scope relaxed atomic store)
//   BVH_WIND_ARRIVE(counter)   this lane's accesses complete, then the arrival ticket: returns the count before it
// Compiled with -ffp-contract=off on both sides; the fused operations below are written out (Num<T>::fma_), division and square root
// are correctly rounded on both sides.
//
// Orientation: a PrecomputedTri holds n = cross(p0 - p1, p2 - p0) = -(ab x ac). The area vector of a triangle is A = (ab x ac) / 2 =
// -n / 2, and the winding number is +1 inside a closed mesh whose ab x ac point outward.
#pragma once

#include "point_walk.inc"

namespace bvh_amd {

namespace {

// ---- atan2 ----------------------------------------------------------------------------------------------------------------------------
// atan(t) = t + t * (u * Q(u)), u = t^2, |t| <= tan(pi / 8): Chebyshev fits of atan(sqrt(u)) / sqrt(u) on [0, tan^2(pi / 8)] whose
// leading coefficient rounds to 1 (largest error of the fit 6.2e-10 for float, 4.6e-20 for double, before rounding).
template <typename T> struct WindAtan;
template <> struct WindAtan<float> {
    static constexpr float kPi = 3.14159274f, kPi2 = 1.57079637f, kPi4 = 0.785398185f, kCut = 0.414213568f;
    __device__ static float q(float u) {
        float p = -0.0602630523f;
        p = Num<float>::fma_(p, u, 0.105698288f);
        p = Num<float>::fma_(p, u, -0.142395327f);
        p = Num<float>::fma_(p, u, 0.199981830f);
        p = Num<float>::fma_(p, u, -0.333333069f);
        return p;
    }
};
template <> struct WindAtan<double> {
    static constexpr double kPi = 3.141592653589793, kPi2 = 1.5707963267948966, kPi4 = 0.7853981633974483, kCut = 0.41421356237309503;
    __device__ static double q(double u) {
        double p = 0.01511376509660092467;
        p = Num<double>::fma_(p, u, -0.03338782450121195152);
        p = Num<double>::fma_(p, u, 0.04499500728984032009);
        p = Num<double>::fma_(p, u, -0.05217312574061591002);
        p = Num<double>::fma_(p, u, 0.05876834004614160664);
        p = Num<double>::fma_(p, u, -0.06666205259976526188);
        p = Num<double>::fma_(p, u, 0.07692281099937743250);
        p = Num<double>::fma_(p, u, -0.09090908059031191027);
        p = Num<double>::fma_(p, u, 0.11111111085322108759);
        p = Num<double>::fma_(p, u, -0.14285714285329708164);
        p = Num<double>::fma_(p, u, 0.19999999999997013892);
        p = Num<double>::fma_(p, u, -0.33333333333333324206);
        return p;
    }
};

// atan2(y, x) with the signs and special values of IEEE 754 / C: +-0 for y = +-0 and x > 0 or +0, +-pi for y = +-0 and x < 0 or -0,
// +-pi/2 on the y axis, pi/4 steps for equal magnitudes (infinities included), NaN for a NaN. Octant reduction to mn / mx in [0, 1],
// then ONE division: above tan(pi / 8) the quotient is (mn - mx) / (mn + mx) = tan(angle - pi / 4), so the polynomial only ever sees
// |t| <= tan(pi / 8); nothing overflows for finite input. Largest absolute error measured against a float64 / multi-precision atan2: tests/test_winding_host.py.
template <typename T>
__device__ inline T wind_atan2(T y, T x) {
    using K = WindAtan<T>;
    const T ax = Num<T>::abs_(x), ay = Num<T>::abs_(y);
    const bool steep = ay > ax;
    const T mx = steep ? ay : ax, mn = steep ? ax : ay;       // (a NaN ends up in mn or mx, and in the quotient)
    T num = mn, den = mx, base = T(0);
    if (mx == T(0)) { num = T(0); den = T(1); }               // atan2(+-0, +-0)
    else if (mn == mx) { num = T(0); den = T(1); base = K::kPi4; }   // (inf, inf) too
    else if (mn > K::kCut * mx) {                             // (halved first where the sum overflows: exact, both are huge there)
        num = mn - mx; den = mn + mx; base = K::kPi4;
        if (!Num<T>::finite(den)) { num = T(0.5) * mn - T(0.5) * mx; den = T(0.5) * mn + T(0.5) * mx; }
    }
    const T t = num / den;
    const T u = t * t;
    T r = base + Num<T>::fma_(t, u * K::q(u), t);
    if (steep) r = K::kPi2 - r;
    if (Num<T>::sign(x)) r = K::kPi - r;
    return Num<T>::copysign_(r, y);
}

// The solid angle of triangle p (a PrecomputedTri) seen from q, signed: positive when q is on the side ab x ac points away from
// (Van Oosterom & Strackee): 2 atan2(det(a, b, c), |a||b||c| + (a.b)|c| + (a.c)|b| + (b.c)|a|) with a, b, c the vertices minus q.
// b = a - e1 and c = a + e2, so det(a, b, c) = det(a, -e1, e2) = -(a . n): the record's normal serves. A zero determinant (q in the
// triangle's plane, q at a vertex, a degenerate triangle) contributes 0 whatever the denominator's sign: in the plane outside the
// triangle that is the value, inside it (on the surface) it is the mean of the two sides.
// Finite as long as the products of three distances are: with d the largest distance from q to a vertex, 8 d^3 must be
// representable (float: d below about 3e12) and d^2 must not underflow.
template <typename T>
__device__ inline T wind_solid_angle(const T (&p)[12], const T (&q)[3]) {
    const T a[3] = { p[0] - q[0], p[1] - q[1], p[2] - q[2] };
    const T b[3] = { a[0] - p[3], a[1] - p[4], a[2] - p[5] };
    const T c[3] = { a[0] + p[6], a[1] + p[7], a[2] + p[8] };
    const T det = -dot3(a[0], a[1], a[2], p[9], p[10], p[11]);
    if (det == T(0)) return T(0);
    const T la = Num<T>::sqrt_(dot3(a[0], a[1], a[2], a[0], a[1], a[2]));
    const T lb = Num<T>::sqrt_(dot3(b[0], b[1], b[2], b[0], b[1], b[2]));
    const T lc = Num<T>::sqrt_(dot3(c[0], c[1], c[2], c[0], c[1], c[2]));
    const T ab = dot3(a[0], a[1], a[2], b[0], b[1], b[2]);
    const T ac = dot3(a[0], a[1], a[2], c[0], c[1], c[2]);
    const T bc = dot3(b[0], b[1], b[2], c[0], c[1], c[2]);
    const T den = ((la * lb * lc + ab * lc) + ac * lb) + bc * la;
    return T(2) * wind_atan2(det, den);
}

// ---- the moments ----------------------------------------------------------------------------------------------------------------------
// Row c + 1 of the moments holds node c: {cx, cy, cz, r2, Nx, Ny, Nz, area}; row 0 is zero, so that the siblings 2p + 1, 2p + 2 of
// pair record p share the aligned 16-scalar line at scalar 16 (p + 1). N = sum of the area vectors A_t, area = sum |A_t|; the centre
// c = s / area with s = sum |A_t| g_t (g_t: the centroid), or the centre of the node's box when area is 0; r2 = the squared distance
// from c to the farthest corner of the node's box: a radius about c that needs no second pass over the triangles and bounds them as
// long as the boxes do (after a build or refit_tris). s travels in `sums` (4 scalars per node, per-stream scratch).
constexpr int kWindRow = 8;

// The index word of node c: the root's is the tree's, any other sits in its half of pair record (c - 1) / 2.
template <typename T>
__device__ inline uint32_t wind_node_word(const PairNode<T>* pairs, uint32_t root_index, uint32_t c) {
    if (c == 0) return root_index;
    const PairNode<T>& rec = pairs[(c - 1) / 2];
    return (c & 1) ? rec.li : rec.ri;
}

// The box of node c {minx, maxx, miny, maxy, minz, maxz}: its half of pair record (c - 1) / 2; the root is in no record and takes
// the union of its children's (what a build or a refit gives it). A root that is a leaf (`word` has a count) takes the box of its
// triangles' vertices as the walk rebuilds them (p0, p0 - e1, p0 + e2).
template <typename T>
__device__ inline void wind_node_box(const PairNode<T>* pairs, const T* tris, size_t prim_total, uint32_t c, uint32_t word, T (&box)[6]) {
    if (c != 0) {
        const PairNode<T>& rec = pairs[(c - 1) / 2];
        const T* half = (c & 1) ? rec.lb : rec.rb;
#pragma unroll
        for (int k = 0; k < 6; ++k) box[k] = half[k];
        return;
    }
    if ((word & kCountMask) == 0) {
        const PairNode<T>& rec = pairs[word >> (kCountBits + 1)];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            box[2 * k] = rec.lb[2 * k] < rec.rb[2 * k] ? rec.lb[2 * k] : rec.rb[2 * k];
            box[2 * k + 1] = rec.lb[2 * k + 1] > rec.rb[2 * k + 1] ? rec.lb[2 * k + 1] : rec.rb[2 * k + 1];
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { box[2 * k] = Num<T>::kMax; box[2 * k + 1] = -Num<T>::kMax; }
    const size_t first = word >> kCountBits;
    for (uint32_t s = 0; s < (word & kCountMask) && first + s < prim_total; ++s) {
        T p[12];
        load_prim12(tris + 12 * (first + s), p);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const T v[3] = { p[k], p[k] - p[3 + k], p[k] + p[6 + k] };
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                box[2 * k] = box[2 * k] < v[j] ? box[2 * k] : v[j];
                box[2 * k + 1] = box[2 * k + 1] > v[j] ? box[2 * k + 1] : v[j];
            }
        }
    }
}

// One component of a triangle's centroid, (p0 + p1 + p2) / 3 = p0 + (e2 - e1) / 3, to about one rounding of the RESULT: also where the
// centroid is much nearer to zero than the triangle is wide (a triangle across a coordinate plane), where the plain expression is only
// good to a rounding of the edges. The difference, the quotient and the sum each carry their rounding error (two-sums; the remainder of
// a correctly rounded division by fma).
template <typename T>
__device__ inline T wind_centroid(T p0, T e1, T e2) {
    const T d = e2 - e1, dv = d - e2, de = (e2 - (d - dv)) + (-e1 - dv);       // d + de = e2 - e1 exactly
    const T q = d / T(3), qr = Num<T>::fma_(T(-3), q, d);                        // d = 3 q + qr exactly
    const T g = p0 + q, gv = g - p0, ge = (p0 - (g - gv)) + (q - gv);          // g + ge = p0 + q exactly
    return g + (ge + (qr + de) / T(3));
}

// {N, area, s} of the triangles [first, first + count) in ascending index (slots beyond prim_total are skipped: never in a
// validated tree). mom = {Nx, Ny, Nz, area}, s = {sx, sy, sz}.
template <typename T>
__device__ inline void wind_fold_leaf(const T* tris, size_t prim_total, size_t first, uint32_t count, T (&mom)[4], T (&s)[3]) {
    mom[0] = mom[1] = mom[2] = mom[3] = T(0);
    s[0] = s[1] = s[2] = T(0);
    for (uint32_t j = 0; j < count; ++j) {
        if (first + j >= prim_total) break;
        T p[12];
        load_prim12(tris + 12 * (first + j), p);
        const T len = T(0.5) * Num<T>::sqrt_(dot3(p[9], p[10], p[11], p[9], p[10], p[11]));       // |A_t|
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            mom[k] = mom[k] + T(-0.5) * p[9 + k];                                                  // A_t = -n / 2
            const T g = wind_centroid(p[k], p[3 + k], p[6 + k]);
            s[k] = s[k] + len * g;
        }
        mom[3] = mom[3] + len;
    }
}

// Centre and radius from {area, s} and the node's box, then the node's row and its s: what a climber above may read goes through
// BVH_WIND_STORE.
template <typename T>
__device__ inline void wind_store_node(T* moments, T* sums, uint32_t c, const T (&mom)[4], const T (&s)[3], const T (&box)[6]) {
    T row[kWindRow];
    T r2 = T(0);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const T ck = mom[3] > T(0) ? s[k] / mom[3] : T(0.5) * box[2 * k] + T(0.5) * box[2 * k + 1];
        const T lo = ck - box[2 * k], hi = box[2 * k + 1] - ck;
        const T e = lo > hi ? lo : hi;
        r2 = r2 + e * e;
        row[k] = ck;
    }
    row[3] = r2;
    row[4] = mom[0]; row[5] = mom[1]; row[6] = mom[2]; row[7] = mom[3];
    T* out = moments + size_t(kWindRow) * (size_t(c) + 1);
#pragma unroll
    for (int k = 0; k < kWindRow; ++k) BVH_WIND_STORE(out + k, row[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) BVH_WIND_STORE(sums + 4 * size_t(c) + k, s[k]);
}

// One lane per node of the array. A leaf folds its triangles, stores its row and climbs: at every ancestor the second child to arrive
// computes the node as LEFT + RIGHT (whichever arrived first), stores it and goes on. parent[] holds 0xFFFFFFFF for a node no inner
// node references (the root, and the top of an unused subtree: the climb ends there).
template <typename T>
__device__ inline void wind_prepare_lane(const PairNode<T>* pairs, uint32_t root_index, const T* tris, size_t prim_total, const uint32_t* parent,
                                         uint32_t* arrived, uint32_t n, T* moments, T* sums, uint32_t i) {
    const uint32_t word = wind_node_word(pairs, root_index, i);
    const uint32_t count = word & kCountMask;
    if (count == 0) return;
    T mom[4], s[3], box[6];
    wind_fold_leaf<T>(tris, prim_total, size_t(word >> kCountBits), count, mom, s);
    wind_node_box<T>(pairs, tris, prim_total, i, word, box);
    wind_store_node<T>(moments, sums, i, mom, s, box);
    uint32_t cur = parent[i];
    while (cur != 0xFFFFFFFFu) {
        if (BVH_WIND_ARRIVE(&arrived[cur]) == 0) return;      // first child: the sibling's lane finishes this node
        const uint32_t w = wind_node_word(pairs, root_index, cur);
        const size_t f = size_t(w >> kCountBits);
        if (f + 1 >= n) return;                               // (never in a validated tree)
        const T* l = moments + size_t(kWindRow) * (f + 1) + 4;
        const T* r = l + kWindRow;
#pragma unroll
        for (int k = 0; k < 4; ++k) mom[k] = BVH_WIND_LOAD(l + k) + BVH_WIND_LOAD(r + k);
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] = BVH_WIND_LOAD(sums + 4 * f + k) + BVH_WIND_LOAD(sums + 4 * (f + 1) + k);
        wind_node_box<T>(pairs, tris, prim_total, cur, w, box);
        wind_store_node<T>(moments, sums, cur, mom, s, box);
        cur = parent[cur];
    }
}

// ---- the walk -------------------------------------------------------------------------------------------------------------------------
// Stack entries of a lane held in LDS (pair indices only), as the list queries hold theirs (list_walk.inc).
constexpr int kWindLds = 16;

template <typename T>
struct WindingArgs : PointArgs<T> {
    const T* moments;                          // (node_count + 1) x 8
    T beta2;                                   // wind_beta2(beta)
    T* w;                                      // one winding number per query, caller order
    typename HitOf<T>::Type* hits;             // optional: closest_points' records of the same queries; t is negated where w >= 1/2
};

// beta^2 in the tree's type (+inf for beta = +inf); the launch computes it on the host.
template <typename T>
__host__ __device__ inline T wind_beta2(double beta) { const T b = T(beta); return b * b; }

template <typename T>
__device__ inline void wind_load_row(const T* moments, uint32_t c, T (&m)[kWindRow]) {
    T lo[4], hi[4];
    const T* row = moments + size_t(kWindRow) * (size_t(c) + 1);
    load_prim4(row, lo);
    load_prim4(row + 4, hi);
#pragma unroll
    for (int k = 0; k < 4; ++k) { m[k] = lo[k]; m[4 + k] = hi[k]; }
}

// One query, one lane. Node c (the root first) is tested against its row: when |c - q|^2 > beta^2 r2 it adds the dipole term
// N . (c - q) / |c - q|^3 (as (N . d) / d2 / sqrt(d2): no cube to underflow); otherwise a leaf adds the exact solid angle of each of
// its triangles in ascending index, and an inner node is opened: the left child's subtree first, the right child stacked (as the index
// of the pair record both sit in). With beta = +inf, beta^2 r2 is +inf or, for r2 = 0, NaN: neither is exceeded, every leaf is summed
// exactly. w = sum / 4 pi, accumulated in T in this order: it depends on the tree, the triangles, the moments, beta and the query only.
// A query with a NaN or infinite coordinate gets w = NaN and its hit record is left alone. Slot `slot` of the launch (query
// order[slot], or slot itself); `lane` indexes the HBM spill (Deep), `tid` the LDS array. cnt += {pair records opened, triangles
// summed exactly, far terms added}.
template <typename T, bool Stats, bool Deep>
__device__ inline void winding_lane(const WindingArgs<T>& a, unsigned long long slot, uint32_t* lds_node, int tid, unsigned long long lane,
                                    unsigned long long (&cnt)[3]) {
    const unsigned long long qi = a.order ? a.order[slot] : slot;
    T qq[4];
    load_prim4(a.queries + 4ull * qi, qq);
    const T q[3] = { qq[0], qq[1], qq[2] };
    if (!(Num<T>::finite(q[0]) && Num<T>::finite(q[1]) && Num<T>::finite(q[2]))) {
        store_stream(a.w + qi, T(__builtin_nanf("")));
        return;
    }

    uint32_t spill_node[kPointSmall - kWindLds];
    uint32_t sp = 0;
    auto push = [&](uint32_t pair) {
        if (sp < kWindLds) lds_node[sp * kBlock + tid] = pair;
        else if (!Deep || sp < kPointSmall) spill_node[stack_small_at<kWindLds>(sp)] = pair;
        else a.deep_nodes[stack_deep_at(a, lane, sp)] = pair;
        ++sp;
    };
    auto pop = [&](uint32_t& pair) -> bool {
        if (sp == 0) return false;
        --sp;
        if (sp < kWindLds) pair = lds_node[sp * kBlock + tid];
        else if (!Deep || sp < kPointSmall) pair = spill_node[stack_small_at<kWindLds>(sp)];
        else pair = a.deep_nodes[stack_deep_at(a, lane, sp)];
        return true;
    };

    T sum = T(0);
    uint32_t c = 0, word = a.root_index;
    for (;;) {
        T m[kWindRow];
        wind_load_row(a.moments, c, m);
        const T d[3] = { m[0] - q[0], m[1] - q[1], m[2] - q[2] };
        const T d2 = dot3(d[0], d[1], d[2], d[0], d[1], d[2]);
        if (d2 > a.beta2 * m[3]) {
            sum = sum + dot3(m[4], m[5], m[6], d[0], d[1], d[2]) / d2 / Num<T>::sqrt_(d2);
            if (Stats) ++cnt[2];
        } else if ((word & kCountMask) != 0) {
            const uint32_t first = word >> kCountBits, count = word & kCountMask;
#pragma clang loop vectorize(disable) interleave(disable)
            for (uint32_t i = first; i < first + count; ++i) {
                T p[12];
                load_prim12(a.prims + 12ull * i, p);
                sum = sum + wind_solid_angle(p, q);
            }
            if (Stats) cnt[1] += count;
        } else {
            const uint32_t pair = word >> (kCountBits + 1);
            if (Stats) ++cnt[0];
            push(pair);
            c = 2 * pair + 1;
            word = a.pairs[pair].li;
            continue;
        }
        uint32_t pair = 0;
        if (!pop(pair)) break;
        c = 2 * pair + 2;
        word = a.pairs[pair].ri;
    }
    const T w = sum / (T(4) * WindAtan<T>::kPi);
    store_stream(a.w + qi, w);
    if (a.hits && w >= T(0.5)) a.hits[qi].t = -a.hits[qi].t;
}

} // namespace

} // namespace bvh_amd
