// The coherence key of a ray (traverse.hip: ray_keys_kernel) and of a point, which is a ray with dir = +0 and class_bits = 0
// (closest.hip: closest_keys_kernel): one copy of the key for both. Expects trace_device.h (Num) to have been included.
#pragma once

namespace bvh_amd {

namespace {

// Coherence key of a ray: Morton code of its origin cell (128^3 grid over the root box; round 3: 7 bits per axis are 1 % better than 6
// on the soup for the same three passes, profiles/r03_entry_key_probe.txt) above the direction octant, 24 bits, three
// 8-bit radix passes. Rays of one key start in the same cell and descend the same way first; any order gives the same per-ray
// results. Measured with one ticket range per XCD on 2^24 uniform rays, rays physically permuted (tools/ray_order_probe.py,
// kernel ms): 1M-triangle soup 12.09 as given, 7.52 / 7.28 / 7.25 with 4 / 5 / 6 bits per axis + octant; 10M-triangle mesh 13.92,
// 7.79 / 7.41 / 7.09; octant-major and direction-cube keys lose (soup 7.81, mesh 8.25). The third pass costs ~0.13 ms.
// `hilbert_bits` > 0 (developer experiment, bvh_amd_experiment("key_curve", 1)): the cell's index along the 3D Hilbert curve of that
// many bits per axis instead of its Morton code (Skilling's axes-to-transpose transform): consecutive keys are always adjacent cells.
// Round 5 — `class_bits` > 0: LONG RAYS FIRST. The drain of the persistent grid (profiles/r05_tail_timeline_before.txt: every wave draws its
// last ticket at ~6.5 of 7.5 ms, then needs a median of 0.45 ms to finish the rays it holds; 7.5 % of the grid's time is lost there)
// is as long as the longest walks still in flight, and on the scenes that are reordered at all a walk's length goes with the length of
// the ray's chord through the root box. So the key carries, right below the three top bits of the cell index (the bits that roughly
// select the XCD's ticket range), the chord class of the ray, longest class first, and the cell index gives up its lowest `class_bits`
// bits (neighbours along the curve merge): every XCD still sweeps its part of space in curve order, once per class, and the tickets
// drawn last are the short rays. Per-ray results do not depend on the order.
// `tail_frac` >= 0 with class_bits == 1 — A TAIL CLASS: the order inside every prefix is long / short / TAIL. Tail rays are those whose
// chord through the root box is not longer than tail_frac box diagonals: with 0 the rays that have no chord at all (they miss the box, or
// their [tmin, tmax] is empty: one step, no record fetch), with 0.05 also the ~10 % of a uniform batch that walk a third as far as the
// short class's longest. They are what an XCD should hold when its range runs out: cheap, and numerous enough to keep the machine busy
// while the last real walks finish. The class takes two bits of the key (0 long, 1 short, 2 tail) and the cell index gives up two low
// bits instead of one: [3 prefix bits][2 class bits][cell bits - 2][3 octant bits]. The ticket range of an XCD is the stretch of one
// prefix (traverse.hip: ticket_ranges_kernel), so "last in the prefix" is "last in the range".
// Degenerate rays land in defined classes (tests/test_ticket_ranges_host.py): a NaN origin component clips nothing along its axis (the
// comparisons are false) and counts as cell 0; a NaN or all-zero direction gives a NaN or zero length: not long, hence — with a tail
// class — tail; a NaN tmin / tmax gives no chord (nothing compares greater than it): tail as well.
#if defined(__HIPCC__)
__device__ inline float rcp_fast(float x) { return __builtin_amdgcn_rcpf(x); }       // v_rcp_f32; ordering keys only
#else
inline float rcp_fast(float x) { return 1.0f / x; }                                   // (the host harness of tests/cpp/ticket_ranges_host.cpp)
#endif
__device__ inline double rcp_fast(double x) { return 1.0 / x; }
template <typename T>
__device__ inline uint32_t ray_key(const T (&r)[8], T lx, T ly, T lz, T sx, T sy, T sz, uint32_t cells, int hilbert_bits, int class_bits, T class_scale,
                                   T tail_frac = T(-1)) {
    const T q[3] = { (r[0] - lx) * sx, (r[1] - ly) * sy, (r[2] - lz) * sz };
    uint32_t code = 0;
    uint32_t cell[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        T v = q[k];
        v = v > T(0) ? v : T(0);                              // (NaN origins land in cell 0)
        cell[k] = v >= T(cells - 1) ? cells - 1 : static_cast<uint32_t>(v);
    }
    if (hilbert_bits > 0) {
        uint32_t X[3] = { cell[2], cell[1], cell[0] };        // X[0] ends up in the most significant bit of every triple
        const uint32_t M = 1u << (hilbert_bits - 1);
        for (uint32_t Q = M; Q > 1; Q >>= 1) {
            const uint32_t P = Q - 1;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (X[a] & Q) X[0] ^= P;
                else { const uint32_t t = (X[0] ^ X[a]) & P; X[0] ^= t; X[a] ^= t; }
            }
        }
        X[1] ^= X[0]; X[2] ^= X[1];
        uint32_t t = 0;
        for (uint32_t Q = M; Q > 1; Q >>= 1) if (X[2] & Q) t ^= Q - 1;
        X[0] ^= t; X[1] ^= t; X[2] ^= t;
        cell[2] = X[0]; cell[1] = X[1]; cell[0] = X[2];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t c = cell[k];
        uint32_t s = (c & 1u) | ((c & 2u) << 2) | ((c & 4u) << 4) | ((c & 8u) << 6) | ((c & 16u) << 8) | ((c & 32u) << 10) | ((c & 64u) << 12) | ((c & 128u) << 14);
        code |= s << k;
    }
    const uint32_t oct = (Num<T>::sign(r[3]) ? 1u : 0u) | (Num<T>::sign(r[4]) ? 2u : 0u) | (Num<T>::sign(r[5]) ? 4u : 0u);
    if (class_bits > 0) {
        // chord of the ray through the root box against the box diagonal: slab test against [l, l + cells / s] with the ray's own tmin /
        // tmax. The key only ORDERS rays, so this is the one place of the library that uses the hardware's approximate reciprocal
        // (v_rcp_f32, 1 ulp) instead of an IEEE division — the kernel is bound by its instructions (16.8 M rays x ~400), not by the 512 MB
        // it reads — and the one-bit case compares squares instead of taking two square roots.
        const T l[3] = { lx, ly, lz }, sc[3] = { sx, sy, sz };
        T t0 = r[6], t1 = r[7], d2 = T(0), diag2 = T(0);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const T ext = sc[k] > T(0) ? T(cells) * rcp_fast(sc[k]) : T(0);
            const T inv = rcp_fast(r[3 + k]);
            const T a = (l[k] - r[k]) * inv, b = (l[k] + ext - r[k]) * inv;
            const T lo_t = a < b ? a : b, hi_t = a < b ? b : a;         // (NaN from 0 * inf compares false: that slab does not clip)
            t0 = lo_t > t0 ? lo_t : t0; t1 = hi_t < t1 ? hi_t : t1;
            d2 += r[3 + k] * r[3 + k]; diag2 += ext * ext;
        }
        const uint32_t top = (1u << class_bits) - 1u;
        uint32_t cls = 0;
        int field_bits = class_bits;                                    // bits of the key the class takes from the cell index
        const T len = t1 > t0 ? t1 - t0 : T(0);
        if (class_bits == 1) {
            const T len2 = len * len * d2;                              // the squared chord
            cls = len2 * class_scale * class_scale >= diag2 && diag2 > T(0) ? 0u : 1u;      // long / short
            if (tail_frac >= T(0)) {
                if (cls != 0u && !(len2 > tail_frac * tail_frac * diag2)) cls = 2u;         // tail (no chord at all, a NaN length included)
                field_bits = 2;
            }
        } else {
            const T rel = diag2 > T(0) ? len * Num<T>::sqrt_(d2) / Num<T>::sqrt_(diag2) * class_scale : T(0);
            cls = rel >= T(top) ? top : rel > T(0) ? static_cast<uint32_t>(rel) : 0u;
            cls = top - cls;                                            // longest class first
        }
        const int code_bits = 3 * (hilbert_bits > 0 ? hilbert_bits : 31 - __clz(cells));
        const uint32_t high = code >> (code_bits - 3), low = (code & ((1u << (code_bits - 3)) - 1u)) >> field_bits;
        code = (((high << field_bits) | cls) << (code_bits - 3 - field_bits)) | low;
    }
    return (code << 3) | oct;
}

} // namespace

} // namespace bvh_amd
