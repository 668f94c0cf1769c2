// Per-lane bodies of the instanced ray queries (instanced.hip): the preparation of one instance (world-to-object matrix, world box,
// centre) and the two-level walk of one ray — a top tree over instance boxes, and at an instance the ray carried into object space and
// walked through that geometry's own tree. Kept as an include so that tests/cpp/instanced_body_host.cpp compiles the very same text
// for the host (one emulated lane per ray / instance). Expects what point_walk.inc expects (trace_device.h: Num, dot3, load_pair,
// load_prim12, load_ray, store_hit; common.h or the harnesses' stand-ins). The stack's tiers and index arithmetic are point_walk.inc's;
// the ray constants and the slab step are trace_device.h's (ray_constants, slab_pair), the triangle test is tri_test.inc: all shared with trace_body.inc.
// Compiled with -ffp-contract=off on both sides: one rounding per operation, so host and device produce the same bits.
#pragma once

#include "point_walk.inc"

namespace bvh_amd {

namespace {

// Stack entries of a lane held in LDS (node words, [depth][lane]), the rest of 64 in scratch, beyond in HBM (point_walk.inc). 8 is
// the measured optimum of closest_points (closest_body.inc); nothing has been measured for this walk, whose entries are half as wide
// (8 KB per block), so the LDS does not bound the occupancy either way (DESIGN.md, "Instanced ray queries").
constexpr int kInstLds = 8;
// Geometries whose table travels by value in the kernel arguments (40 bytes each: 640 of the 4096 bytes a launch may pass); larger
// tables are written to stream-ordered scratch by a copy kernel that itself takes them by value, kInstSmallGeoms at a time.
constexpr int kInstSmallGeoms = 16;

// One geometry: its traversal records, BVH-order PrecomputedTri, prim ids, root index word, and the box of its root node
// {minx, maxx, miny, maxy, minz, maxz} (read by the preparation only).
template <typename T>
struct InstGeom {
    const PairNode<T>* pairs;
    const T* tris;
    const uint32_t* prim_ids;
    const T* root_box;
    uint32_t root_index;
    uint32_t pad;
};

template <typename T, bool Small> struct InstGeomTable;
template <typename T> struct InstGeomTable<T, true> { InstGeom<T> g[kInstSmallGeoms]; };
template <typename T> struct InstGeomTable<T, false> { const InstGeom<T>* g; };

template <typename T, bool Small>
struct InstancedArgs {
    const PairNode<T>* top_pairs;
    const uint32_t* top_prim_ids;              // slot of a top leaf -> instance
    const T* world2obj;                        // 12 per instance, row-major 3 x 4; first entry NaN: disabled
    const uint32_t* geometry;                  // per instance, or null: all 0
    const T* rays;
    typename HitOf<T>::Type* hits;
    uint32_t* hit_instances;
    unsigned long long n;                      // rays of this launch: [first, first + n)
    unsigned long long first;
    bvh_amd_counters* counters;                // Stats kernels only
    uint32_t* deep_nodes;                      // Deep kernels only: deep_cap entries per lane of the launch beyond the 64 of LDS + scratch
    uint32_t deep_cap;
    uint32_t top_root;
    uint32_t n_geoms;
    uint32_t original_ids;                     // BVH_AMD_RAY_ORIGINAL_IDS: prim = prim_ids of the hit geometry [BVH-order index]
    InstGeomTable<T, Small> geoms;
};

// One ray, one lane. Walks the top tree as Bvh::intersect<Any, Robust> does (the root box is never tested, near child first and the
// far one stacked, ties to the left, any-hit never reorders); at a top leaf takes its slots in order; an enabled instance with a
// geometry of the table gets the ray in its object space (org' = W org + w, dir' = W dir through dot3, tmin and the current tmax as
// they are: the direction is not normalised, so t means the same in both spaces), and its tree is walked from its root index word
// with the same rules and the batch kernels' triangle test. An accepted hit shortens tmax for everything after it, in both levels.
//
// One stack serves both levels: entering an instance pushes a marker — the rest of the top leaf as a leaf word, (next slot) << 4 |
// slots left, possibly none — and the geometry's walk treats the stack height above it (`base`) as empty. Popping the marker restores
// the world-space ray: the constants are RECOMPUTED from the stored ray (one 32 / 64-byte load that hits the cache it came through and
// three divisions per instance left) rather than kept: keeping org, dir, inv and aux would hold 12 more scalars (24 VGPRs for double)
// live through the geometry's walk, where the walk spends its time. The stack holds at most depth(top) + 1 + depth(geometry) entries.
//
// A ray with a NaN tmin or tmax fails every test there is: it ends before its first fetch and counts nothing. cnt += {pair records
// fetched, triangles tested, leaves visited}, both levels; a top leaf counts once, entering an instance nothing.
template <typename T, bool Any, bool Robust, bool Stats, bool Deep, bool Small>
__device__ inline void instanced_lane(const InstancedArgs<T, Small>& a, unsigned long long ri, uint32_t* lds_node, int tid, unsigned long long lane,
                                      unsigned long long (&cnt)[3]) {
    T r[8];
    load_ray(a.rays + 8 * ri, r);
    T org[3] = { r[0], r[1], r[2] }, dir[3] = { r[3], r[4], r[5] }, inv[3], aux[3];
    uint32_t oct[3];
    const T tmin = r[6];
    T tmax = r[7];
    const bool nan_ray = !(tmin == tmin) || !(tmax == tmax);
    ray_constants<T, Robust, 3>(org, dir, inv, aux, oct);

    uint32_t hit_prim = BVH_AMD_INVALID, hit_inst = BVH_AMD_INVALID;
    T hit_t = tmax, hit_u = T(0), hit_v = T(0);

    uint32_t spill_node[kPointSmall - kInstLds];
    uint32_t sp = 0, base = 0;
    auto push = [&](uint32_t node) {
        if (sp < kInstLds) lds_node[sp * kBlock + tid] = node;
        else if (!Deep || sp < kPointSmall) spill_node[stack_small_at<kInstLds>(sp)] = node;
        else a.deep_nodes[stack_deep_at(a, lane, sp)] = node;
        ++sp;
    };
    auto pop = [&]() -> uint32_t {
        --sp;
        if (sp < kInstLds) return lds_node[sp * kBlock + tid];
        if (!Deep || sp < kPointSmall) return spill_node[stack_small_at<kInstLds>(sp)];
        return a.deep_nodes[stack_deep_at(a, lane, sp)];
    };

    const PairNode<T>* pairs = a.top_pairs;
    const T* tris = nullptr;
    uint32_t node = a.top_root, inst = BVH_AMD_INVALID;
    bool object = false;                                      // walking a geometry's tree, in its object space
    bool live = !nan_ray;
    while (live) {
        bool ended = false;                                   // this level's walk has nothing stacked any more
        while ((node & kCountMask) == 0) {                    // inner node: both children in one record (bvh.h:132-150)
            T lb[6], rb[6], l0, l1, r0, r1;
            uint32_t li = 0, ri2 = 0;
            load_pair(pairs + (node >> (kCountBits + 1)), lb, rb, li, ri2);
            if (Stats) ++cnt[0];
            slab_pair<T, Robust, 3>(lb, rb, org, inv, aux, oct, tmin, tmax, l0, l1, r0, r1);
            const bool hl = l0 <= l1, hr = r0 <= r1;
            if (hl) {
                uint32_t near_i = li;
                if (hr) {
                    uint32_t far_i = ri2;
                    if (!Any && l0 > r0) { near_i = ri2; far_i = li; }
                    push(far_i);
                }
                node = near_i;
            } else if (hr) {
                node = ri2;
            } else if (sp == base) {
                ended = true;
                break;
            } else {
                node = pop();
            }
        }
        uint32_t slots = 0;                                   // the top leaf, or what is left of one, to take instances from
        bool at_top_leaf = false;
        if (!ended) {
            if (object) {                                     // a geometry's leaf (tri.h:56-74)
                const uint32_t first = node >> kCountBits, count = node & kCountMask;
                if (Stats) ++cnt[2];
                for (uint32_t i = first; i < first + count; ++i) {
                    if (Stats) ++cnt[1];
                    T p[12];
                    load_prim12(tris + 12ull * i, p);
#define BVH_TRI_ACCEPTED hit_prim = i; hit_inst = inst
#include "tri_test.inc"
#undef BVH_TRI_ACCEPTED
                }
                if (Any && hit_prim != BVH_AMD_INVALID) break;
                if (sp == base) ended = true;
                else node = pop();
            } else {
                if (Stats) ++cnt[2];
                slots = node;
                at_top_leaf = true;
            }
        }
        if (ended) {
            if (!object) break;                               // the top tree's walk is over
            slots = pop();                                    // the marker: back to world space, on with the top leaf
            object = false;
            base = 0;
            pairs = a.top_pairs;
            load_ray(a.rays + 8 * ri, r);
            org[0] = r[0]; org[1] = r[1]; org[2] = r[2]; dir[0] = r[3]; dir[1] = r[4]; dir[2] = r[5];
            ray_constants<T, Robust, 3>(org, dir, inv, aux, oct);
            at_top_leaf = true;
        }
        if (at_top_leaf) {
            uint32_t s = slots >> kCountBits;
            const uint32_t end = s + (slots & kCountMask);
            for (; s < end; ++s) {
                inst = a.top_prim_ids[s];
                const uint32_t gi = a.geometry ? a.geometry[inst] : 0u;
                if (gi >= a.n_geoms) continue;
                T w[12];
                load_prim12(a.world2obj + 12ull * inst, w);
                if (!(w[0] == w[0])) continue;                // disabled instance
                push(((s + 1) << kCountBits) | (end - s - 1));
                base = sp;
                object = true;
                const T o0 = org[0], o1 = org[1], o2 = org[2], d0 = dir[0], d1 = dir[1], d2 = dir[2];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    org[k] = dot3(w[4 * k], w[4 * k + 1], w[4 * k + 2], o0, o1, o2) + w[4 * k + 3];
                    dir[k] = dot3(w[4 * k], w[4 * k + 1], w[4 * k + 2], d0, d1, d2);
                }
                ray_constants<T, Robust, 3>(org, dir, inv, aux, oct);
                pairs = a.geoms.g[gi].pairs;
                tris = a.geoms.g[gi].tris;
                node = a.geoms.g[gi].root_index;
                break;
            }
            if (!object) {                                    // no instance left in this leaf
                if (sp == 0) break;
                node = pop();
            }
        }
    }
    if (hit_prim != BVH_AMD_INVALID && a.original_ids) {
        const uint32_t gi = a.geometry ? a.geometry[hit_inst] : 0u;
        hit_prim = a.geoms.g[gi].prim_ids[hit_prim];
    }
    store_hit(a.hits + ri, hit_prim, hit_t, hit_u, hit_v);
    a.hit_instances[ri] = hit_inst;
}

// The NaN of a disabled instance, by its bits: the same on the host and on the device.
__device__ inline float quiet_nan(float) { return __uint_as_float(0x7FC00000u); }
__device__ inline double quiet_nan(double) { return __longlong_as_double(0x7FF8000000000000ll); }

template <typename T, bool Small>
struct InstancePrepareArgs {
    const T* obj2world;                        // 12 per instance, row-major 3 x 4: x_world = M x_object + t
    const uint32_t* geometry;                  // per instance, or null: all 0
    T* world2obj;
    T* bboxes;                                 // {min.xyz, max.xyz} per instance, what bvhXX_build_device / bvhXX_refit_boxes take
    T* centers;
    unsigned long long n;
    uint32_t n_geoms;
    InstGeomTable<T, Small> geoms;
};

// One instance, one lane: the inverse of its affine map, its world box, that box's centre.
//
// Inverse: adjugate over determinant, in T. A zero determinant, or anything non-finite among the inputs, the inverse or the box,
// DISABLES the instance: twelve NaNs (the walk skips an instance whose first entry is NaN), and the zero-extent box at its
// translation, or at the origin when the translation is not finite — builders and refits never see a NaN. An instance whose
// geometry index is outside the table keeps its inverse (it does not depend on the geometry) and gets the same zero-extent box.
//
// World box of the geometry's root box [lo, hi]: centre / half-extent form, c = (lo + hi) / 2, h = (hi - lo) / 2, c'_i = sum_j m_ij c_j + t_i,
// h'_i = sum_j |m_ij| h_j, box_i = [c'_i - h'_i - pad_i, c'_i + h'_i + pad_i]. The pad makes it conservative under rounding. With
// u = eps / 2 the unit roundoff and S_i = sum_j |m_ij| max(|lo_j|, |hi_j|) + |t_i| (which bounds every magnitude below: |c_j| + h_j
// = max(|lo_j|, |hi_j|)), the longest chain to a bound of the box is: lo + hi (1 rounding; the halving is exact), the product with
// m_ij (1), the two additions of dot3 that round (2; the first adds to 0), + t_i (1) — c' is within gamma_5 S_i of the exact centre;
// h' likewise within gamma_4 S_i (no translation); then c' -/+ h' (1) and -/+ pad (1), each rounding a value of magnitude <= S_i (1 + ...).
// Together at most (5 + 4 + 1 + 1) u S_i = 11 u S_i to first order, so the exact image lies inside once pad_i >= 11 u S_i (1 + O(u)).
// pad_i = 12 eps S~_i = 24 u S~_i with S~_i the computed S_i (a sum of non-negative terms, within gamma_6 of S_i): more than twice
// the bound, which leaves room for whoever checks it in another precision, and well inside the 32 eps S_i the boxes are allowed.
template <typename T, bool Small>
__device__ inline void instance_prepare_lane(const InstancePrepareArgs<T, Small>& a, unsigned long long i) {
    T m[12];
    load_prim12(a.obj2world + 12ull * i, m);
    const uint32_t gi = a.geometry ? a.geometry[i] : 0u;
    // cofactors of the linear part, row by row; det = row 0 . its cofactors
    const T c00 = m[5] * m[10] - m[6] * m[9], c01 = m[6] * m[8] - m[4] * m[10], c02 = m[4] * m[9] - m[5] * m[8];
    const T c10 = m[2] * m[9] - m[1] * m[10], c11 = m[0] * m[10] - m[2] * m[8], c12 = m[1] * m[8] - m[0] * m[9];
    const T c20 = m[1] * m[6] - m[2] * m[5], c21 = m[2] * m[4] - m[0] * m[6], c22 = m[0] * m[5] - m[1] * m[4];
    const T det = dot3(m[0], m[1], m[2], c00, c01, c02);
    const T idet = T(1) / det;
    T w[12];
    w[0] = c00 * idet; w[1] = c10 * idet; w[2] = c20 * idet;              // inverse = transposed cofactors / det
    w[4] = c01 * idet; w[5] = c11 * idet; w[6] = c21 * idet;
    w[8] = c02 * idet; w[9] = c12 * idet; w[10] = c22 * idet;
#pragma unroll
    for (int k = 0; k < 3; ++k) w[4 * k + 3] = -dot3(w[4 * k], w[4 * k + 1], w[4 * k + 2], m[3], m[7], m[11]);
    bool ok = det != T(0);
#pragma unroll
    for (int k = 0; k < 12; ++k) ok = ok && Num<T>::finite(m[k]) && Num<T>::finite(w[k]);

    const bool t_finite = Num<T>::finite(m[3]) && Num<T>::finite(m[7]) && Num<T>::finite(m[11]);
    T lo[3], hi[3], cen[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) lo[k] = hi[k] = cen[k] = t_finite ? m[4 * k + 3] : T(0);
    if (ok && gi < a.n_geoms) {
        const T* rb = a.geoms.g[gi].root_box;
        T c[3], h[3], mx[3], blo[3], bhi[3], bc[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const T l = rb[2 * j], g = rb[2 * j + 1];
            c[j] = (l + g) * T(0.5);
            h[j] = (g - l) * T(0.5);
            const T al = Num<T>::abs_(l), ag = Num<T>::abs_(g);
            mx[j] = al > ag ? al : ag;
        }
        bool box_ok = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const T a0 = Num<T>::abs_(m[4 * k]), a1 = Num<T>::abs_(m[4 * k + 1]), a2 = Num<T>::abs_(m[4 * k + 2]);
            const T cw = dot3(m[4 * k], m[4 * k + 1], m[4 * k + 2], c[0], c[1], c[2]) + m[4 * k + 3];
            const T hw = dot3(a0, a1, a2, h[0], h[1], h[2]);
            const T pad = (T(12) * Num<T>::kEps) * (dot3(a0, a1, a2, mx[0], mx[1], mx[2]) + Num<T>::abs_(m[4 * k + 3]));
            blo[k] = (cw - hw) - pad;
            bhi[k] = (cw + hw) + pad;
            bc[k] = cw;
            box_ok = box_ok && Num<T>::finite(blo[k]) && Num<T>::finite(bhi[k]) && blo[k] <= bhi[k];
        }
        if (box_ok) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { lo[k] = blo[k]; hi[k] = bhi[k]; cen[k] = bc[k]; }
        } else {
            ok = false;                                       // (a root box that is empty, NaN or overflows: nothing to hit)
        }
    }
    if (!ok) {
#pragma unroll
        for (int k = 0; k < 12; ++k) w[k] = quiet_nan(T(0));
    }
    T* wo = a.world2obj + 12ull * i;
#pragma unroll
    for (int k = 0; k < 12; ++k) wo[k] = w[k];
    T* bb = a.bboxes + 6ull * i;
    T* cc = a.centers + 3ull * i;
#pragma unroll
    for (int k = 0; k < 3; ++k) { bb[k] = lo[k]; bb[3 + k] = hi[k]; cc[k] = cen[k]; }
}

} // namespace

} // namespace bvh_amd
