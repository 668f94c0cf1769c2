// Per-lane body of the batched closest-point query (closest.hip): the squared distance of a point to one primitive — a PrecomputedTri
// {p0, e1 = p0 - p1, e2 = p2 - p0, n} or a Sphere {c, r} — and the depth-first walk of one query through the pair records. Kept as an
// include so that tests/cpp/closest_body_host.cpp compiles the very same text for the host (one emulated lane per query).
// Expects trace_device.h (Num, dot3, load_pair, load_prim12, load_prim4, store_hit, kBlock) and common.h, or the test's stand-ins
// for it (PairNode, HitOf, kCountBits, kCountMask, LEAF_*). Compiled with -ffp-contract=off on both sides: one rounding per operation,
// division and square root correctly rounded, so host and device produce the same bits.
#pragma once

namespace bvh_amd {

namespace {

// Stack entries of a lane held in LDS ({node word, box distance^2} in two [depth][lane] arrays, conflict-free), the rest of the
// first 64 in per-lane scratch, entries beyond 64 (trees deeper than 64 levels only) in HBM. A walk pushes at most one entry per
// level, so the tree's depth bounds the stack. 8 entries in LDS (16 KB per block of float queries, 24 KB of double: 7 / 5-6 waves per
// SIMD, the VGPRs' limit) against 16 (5 / 3 waves, bound by LDS): 2^24 uniform queries on the 1M soup 12.10 -> 10.46 ms, on 1M f64
// spheres 15.10 -> 13.24 ms (DESIGN.md, "Closest-point queries").
constexpr int kClosestLds = 8;
constexpr int kClosestSmall = 64;

template <typename T>
struct ClosestArgs {
    const PairNode<T>* pairs;
    const T* prims;                            // BVH order: PrecomputedTri (12 scalars) or Sphere<T, 3> (4 scalars)
    const T* queries;                          // {x, y, z, max_distance} per query, caller order
    typename HitOf<T>::Type* hits;             // one record per query, caller order
    unsigned long long n;                      // slots of this launch: [first, first + n)
    unsigned long long first;
    const uint32_t* order;                     // optional: slot -> query index (coherence sort); results are unaffected
    const uint32_t* prim_ids;                  // optional: report prim_ids[i] instead of the BVH-order index i (BVH_AMD_RAY_ORIGINAL_IDS)
    bvh_amd_counters* counters;                // Stats kernels only
    uint32_t* deep_nodes;                      // Deep kernels only: deep_cap entries per lane of the launch beyond the 64 of LDS + scratch
    T* deep_d2;
    uint32_t deep_cap;
    uint32_t root_index;
};

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

// One query, one lane: depth-first walk, nearer child first, the farther one pushed with its box distance^2; a child or popped entry
// farther than the best primitive so far is dropped. best starts at max_distance^2; among primitives at the same squared distance the
// lowest BVH-order index wins, whatever the visiting order. Slot `slot` of the launch (query order[slot], or slot itself); `lane`
// indexes the HBM spill (Deep), `tid` the LDS arrays. cnt += {pair records fetched, primitives tested, leaves visited}.
template <typename T, int Leaf, bool Stats, bool Deep>
__device__ inline void closest_lane(const ClosestArgs<T>& a, unsigned long long slot, uint32_t* lds_node, T* lds_d2, int tid,
                                    unsigned long long lane, unsigned long long (&cnt)[3]) {
    const unsigned long long qi = a.order ? a.order[slot] : slot;
    T qq[4];
    load_prim4(a.queries + 4ull * qi, qq);
    const T q[3] = { qq[0], qq[1], qq[2] };
    const T max_d = qq[3];
    uint32_t best_prim = BVH_AMD_INVALID;
    T best = max_d * max_d, best_u = T(0), best_v = T(0);
    const bool valid = q[0] == q[0] && q[1] == q[1] && q[2] == q[2] && max_d >= T(0);   // NaN coordinates / radius, negative radius: miss

    uint32_t spill_node[kClosestSmall - kClosestLds];
    T spill_d2[kClosestSmall - kClosestLds];
    uint32_t sp = 0;
    auto deep_at = [&](uint32_t i) { return lane * a.deep_cap + (i < a.deep_cap ? i : a.deep_cap - 1); };
    auto push = [&](uint32_t node, T d2) {
        if (sp < kClosestLds) { lds_node[sp * kBlock + tid] = node; lds_d2[sp * kBlock + tid] = d2; }
        else if (!Deep || sp < kClosestSmall) {
            const uint32_t i = sp - kClosestLds < uint32_t(kClosestSmall - kClosestLds - 1) ? sp - kClosestLds : uint32_t(kClosestSmall - kClosestLds - 1);
            spill_node[i] = node; spill_d2[i] = d2;
        } else { const unsigned long long i = deep_at(sp - kClosestSmall); a.deep_nodes[i] = node; a.deep_d2[i] = d2; }
        ++sp;
    };
    // the next stacked entry that can still hold something nearer than `best` (false: the walk is over)
    auto pop = [&](uint32_t& node) -> bool {
        while (sp > 0) {
            --sp;
            uint32_t e;
            T d2;
            if (sp < kClosestLds) { e = lds_node[sp * kBlock + tid]; d2 = lds_d2[sp * kBlock + tid]; }
            else if (!Deep || sp < kClosestSmall) {
                const uint32_t i = sp - kClosestLds < uint32_t(kClosestSmall - kClosestLds - 1) ? sp - kClosestLds : uint32_t(kClosestSmall - kClosestLds - 1);
                e = spill_node[i]; d2 = spill_d2[i];
            } else { const unsigned long long i = deep_at(sp - kClosestSmall); e = a.deep_nodes[i]; d2 = a.deep_d2[i]; }
            if (d2 <= best) { node = e; return true; }
        }
        return false;
    };

    uint32_t node = a.root_index;
    bool live = valid;
    while (live) {
        while ((node & kCountMask) == 0) {                    // inner node: both children in one record
            T lb[6], rb[6];
            uint32_t li = 0, ri = 0;
            load_pair(a.pairs + (node >> (kCountBits + 1)), lb, rb, li, ri);
            if (Stats) ++cnt[0];
            const T dl = box_dist2(lb, q), dr = box_dist2(rb, q);
            const bool hl = dl <= best, hr = dr <= best;
            if (hl && hr) {
                if (dr < dl) { push(li, dl); node = ri; }
                else { push(ri, dr); node = li; }
            } else if (hl) node = li;
            else if (hr) node = ri;
            else if (!pop(node)) { live = false; break; }
        }
        if (!live) break;
        const uint32_t first = node >> kCountBits, count = node & kCountMask;
        if (Stats) ++cnt[2];
        for (uint32_t i = first; i < first + count; ++i) {
            if (Stats) ++cnt[1];
            T d2, u = T(0), v = T(0);
            if (Leaf == LEAF_TRIANGLE) {
                T p[12];
                load_prim12(a.prims + 12ull * i, p);
                d2 = tri_dist2(p, q, u, v);
            } else {
                T s[4];
                load_prim4(a.prims + 4ull * i, s);
                d2 = sphere_dist2(s, q);
            }
            if (d2 < best || (d2 == best && i < best_prim)) { best = d2; best_prim = i; best_u = u; best_v = v; }
        }
        live = pop(node);
    }
    if (best_prim != BVH_AMD_INVALID) {
        store_hit(a.hits + qi, a.prim_ids ? a.prim_ids[best_prim] : best_prim, Num<T>::sqrt_(best), best_u, best_v);
    } else {
        store_hit(a.hits + qi, BVH_AMD_INVALID, max_d, T(0), T(0));
    }
}

} // namespace

} // namespace bvh_amd
