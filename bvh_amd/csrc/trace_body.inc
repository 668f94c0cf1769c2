// Body of the batch traversal kernel of traverse.hip. Kept as an include so that tests/cpp/trace_body_host.cpp can compile the
// very same text for the host (one emulated lane, or a wavefront of 64 fibers).
// In scope: T, Any, Robust, Leaf, Stats, D, Deep and the kernel argument `a`; BVH_TRACE_COOP (a constant expression: the kernel's
// Coop parameter; false where the includer does not define it).
#ifndef BVH_TRACE_COOP
#define BVH_TRACE_COOP false
#endif
    constexpr int kDepth = kLdsDepth;
    constexpr int kSpill = 64 - kDepth;            // kDepth + kSpill = 64 = the reference's SmallStack capacity
    __shared__ uint32_t lds_stack[kDepth * kBlock];
    uint32_t spill[kSpill];
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const uint64_t lanes_below = (uint64_t{1} << lane) - 1;

    // per-slot ray state
    bool have = false, done = false, drained = false, nan_ray = false;
    // The tickets of a launch are cut into a.parts consecutive ranges with a counter each; a block starts in the range of its
    // XCD (blocks are observed to be placed round-robin, block b on XCD b % 8; nothing but speed depends on it) and moves on to
    // the next range when one runs dry. With coherence-sorted rays each L2 then serves one stretch of the order instead of
    // one eighth of every stretch (measured, 16M sorted rays on the 1M soup: 9.84 -> 9.62 ms; 4M rays on the 262k-triangle
    // Sponza proxy: 1.11 -> 0.76 ms. More ranges than XCDs lose again: 32 -> 9.66 ms, 512 -> 10.3 ms).
    // The ranges are equal slices of the tickets, or, where the launch gives a.range_starts, the stretches of the sorted order that
    // hold one key prefix each (ray_key.h): a range then ends on its own prefix's cheapest rays, not on the first — long — rays of the
    // next prefix. The staggered drain below counts what is left up to the range's real end either way.
    uint32_t part = a.parts > 1 ? blockIdx.x % a.parts : 0, parts_left = a.parts;
    // (Reserving several refills' worth of tickets per atomic was measured and lost everywhere: a reservation that ends inside
    //  a refill leaves lanes idle, and waves sitting on reservations widen the stretch of the order in flight.)
    unsigned long long ray_id = 0;
    T org[3], dir[3], inv[3], aux[3];            // aux = inv_dir_pad (robust) or inv_org (fast)
    T tmin = 0, tmax = 0;
    uint32_t oct[3] = {0, 0, 0};
    uint32_t top = 0, sp = 0;
    uint32_t hit_prim = BVH_AMD_INVALID;
    T hit_t = 0, hit_u = 0, hit_v = 0;
    unsigned long long n_pairs = 0, n_tests = 0, n_leaves = 0;
#if defined(BVH_AMD_DEVELOPER) && defined(__HIPCC__)
    // drain-tail timeline (profiles/r05_tail_timeline.txt): when does each wave start, draw its last ticket, leave
    unsigned long long wt_begin = 0, wt_last_refill = 0, wt_rays = 0, wt_refill_ticks = 0, wt_refills = 0;
    if (a.wave_times) wt_begin = __builtin_amdgcn_s_memrealtime();
#endif

    // (launch_traverse sizes `deep` from the depth of the tree, and every tree that reaches the device has passed the structural
    //  checks of wire.hip — children in range, no pair referenced twice, hence no cycle below the root — so the stack
    //  cannot exceed that depth; the clamps below only keep an index inside its array)
    // launch_traverse knows the depth of the tree: the variant without Deep only ever runs on trees of at most 64 levels, whose
    // stack cannot exceed the 64 entries of LDS + scratch, so its push/pop carry no overflow bookkeeping (the clamp only keeps
    // a malformed, e.g. cyclic, user-supplied tree from writing outside the scratch array). Deep: entries beyond 64 live in HBM
    // (the address of the deep slot is formed inside the cold branch: nothing about it stays live in the hot loop).
    auto deep_slot = [&](uint32_t i) { return a.deep + (size_t{blockIdx.x} * kBlock + tid) * a.deep_cap + i; };
    auto push = [&](uint32_t v) {
        if (sp < kDepth) lds_stack[sp * kBlock + tid] = v;
        else if (!Deep) spill[min(sp - kDepth, static_cast<uint32_t>(kSpill - 1))] = v;
        else if (sp < kDepth + kSpill) spill[sp - kDepth] = v;
        else *deep_slot(min(sp - (kDepth + kSpill), a.deep_cap - 1)) = v;
        ++sp;
    };
    auto pop = [&]() -> uint32_t {
        --sp;
        // (the LDS word is read unconditionally, as a volatile LDS access: left to choose between an LDS and a scratch address, the compiler forms one
        //  flat pointer and the pop — the head of the dependent chain to the next node — becomes a flat load that waits for
        //  both memory counters)
        uint32_t v = lds_word(&lds_stack[min(sp, static_cast<uint32_t>(kDepth - 1)) * kBlock + tid]);
        if (sp >= kDepth) {
            if (!Deep) v = spill[min(sp - kDepth, static_cast<uint32_t>(kSpill - 1))];
            else if (sp < kDepth + kSpill) v = spill[sp - kDepth];
            else v = *deep_slot(min(sp - (kDepth + kSpill), a.deep_cap - 1));
        }
        return v;
    };

    for (;;) {
        // ---- refill idle slots with new rays (one atomic per wave) --------------------------------
        const uint64_t idle = __ballot(!have);
        const int n_idle = __popcll(idle);
        if (!drained && (n_idle >= a.refill_threshold || n_idle == kWave)) {
#if defined(BVH_AMD_DEVELOPER) && defined(__HIPCC__)
            unsigned long long wt_t0 = 0;
            if (a.wave_times) wt_t0 = __builtin_amdgcn_s_memrealtime();
#endif
            unsigned long long base = 0, part_end = a.n;
            if (a.one_shot) {
                // small batches (launch_planned): every wave traces the 64 rays its position in the grid names, once — no ticket counter,
                // no refill: the wave's life is its longest ray's walk, not the walks of the three or four rays a persistent lane
                // strings together, and the hardware backfills the CU with the next block as soon as one is done
                base = (static_cast<unsigned long long>(blockIdx.x) * (kBlock / kWave) + (tid >> 6)) * kWave;
                drained = true;
            } else {
                if (lane == 0) base = atomicAdd(a.work + part * kTicketStride, static_cast<unsigned long long>(n_idle));
                // the range's first ticket and its end: an equal slice, or — a reordered launch — the stretch of the order that holds one
                // key prefix (a.range_starts, written on the device after the sort; any length, also none at all). Read here, in the
                // refill branch, every time: nothing about a range stays live in the inner-node loop.
                unsigned long long part_begin = part * a.part_size;
                part_end = min(a.n, (part + 1ull) * a.part_size);
                if (a.range_starts) { part_begin = a.range_starts[part]; part_end = a.range_starts[part + 1]; }
                base = __shfl(base, 0) + part_begin;
                if (base + n_idle >= part_end) {                     // this range is used up: the next one, or nothing left at all
                    part = part + 1 == a.parts ? 0 : part + 1;
                    if (--parts_left == 0) drained = true;
                } else if (a.stagger && part_end - (base + n_idle) < static_cast<unsigned long long>(a.stagger) * ((blockIdx.x * 8u) / gridDim.x)) {
                    // STAGGERED DRAIN (round 5): the eighth of the grid this block belongs to stops drawing tickets once fewer than
                    // class x stagger are left in the range it draws from, finishes the rays it holds and leaves. The persistent grid
                    // then does not run dry everywhere at once (every wave down to a few lanes, eight of them still sharing each SIMD's
                    // issue slots: ~3 us per step of the longest walks) — by the time the last tickets are drawn one or two waves per
                    // SIMD are left, and the final walks step at their memory latency.
                    drained = true;
                }
            }
            if (!have) {
                const unsigned long long ticket = base + __popcll(idle & lanes_below);
                if (ticket < part_end) {
                    const bool once = (a.stream_hints & 1u) != 0;
                    const unsigned long long my = a.order ? (once ? load_word_nt(a.order + ticket) : a.order[ticket]) : ticket;
                    T r[8];
                    if (D == 3) { if (once) load_ray_nt(a.rays + 8 * my, r); else load_ray(a.rays + 8 * my, r); }
                    else {
                        T q[6];
                        load_ray2(a.rays + 6 * my, q);
                        r[0] = q[0]; r[1] = q[1]; r[2] = T(0); r[3] = q[2]; r[4] = q[3]; r[5] = T(0); r[6] = q[4]; r[7] = q[5];
                    }
#pragma unroll
                    for (int k = 0; k < D; ++k) { org[k] = r[k]; dir[k] = r[3 + k]; }
                    ray_constants<T, Robust, D>(org, dir, inv, aux, oct);
                    tmin = r[6]; tmax = r[7];
                    nan_ray = !(tmin == tmin) || !(tmax == tmax);
                    ray_id = my;
                    have = true; done = false;
                    sp = 0;
                    top = a.root_index;                                 // bvh.h:128-131: push(start); pop()
                    hit_prim = BVH_AMD_INVALID; hit_t = tmax; hit_u = 0; hit_v = 0;
                }
            }
#if defined(BVH_AMD_DEVELOPER) && defined(__HIPCC__)
            if (a.wave_times) {               // (the ray's registers are consumed above: the loads of this refill have arrived by now)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                wt_last_refill = __builtin_amdgcn_s_memrealtime(); wt_rays += __popcll(__ballot(have)) - (kWave - n_idle);
                wt_refill_ticks += wt_last_refill - wt_t0; ++wt_refills;
            }
#endif
        }
        if (__ballot(have) == 0) {
            if (drained) break;
            continue;                                                // (the range ran dry under this wave: ask the next one)
        }

        // ---- inner nodes (bvh.h:132-150) ------------------------------------------------------------
        // All lanes step together; a lane that reaches a leaf (or finishes) parks. The loop is left as soon as
        // enough lanes are parked at leaves, so the leaf code runs for many lanes at once without anyone waiting
        // for the slowest descent (the order of operations of each ray is unchanged).
        for (;;) {
            const bool inner = have && !done && (top & kCountMask) == 0;
            const uint64_t inner_mask = __ballot(inner);
            if (!inner_mask) break;
            const int parked = __popcll(__ballot(have && !done && (top & kCountMask) != 0));
            if (parked >= a.leaf_threshold) break;        // (also leaving to refill when most lanes are idle was measured: no gain)
            T lb[6], rb[6];
            uint32_t li = 0, ri = 0;
            // Coop: the four lanes of a quad fetch each other's records, one line request per record instead of four lane
            // requests (trace_device.h: coop_load_pair); idle and parked lanes only help loading
            if constexpr (BVH_TRACE_COOP) coop_load_pair(a.pairs, a.pair_bytes, inner ? (top >> (kCountBits + 1)) : 0xFFFFFFFFu, lane, lb, rb, li, ri);
            if (inner) {
                if constexpr (!BVH_TRACE_COOP) load_pair(a.pairs + (top >> (kCountBits + 1)), lb, rb, li, ri);
                if (Stats) ++n_pairs;
                T l0, l1, r0, r1;
                slab_pair<T, Robust, D>(lb, rb, org, inv, aux, oct, tmin, tmax, l0, l1, r0, r1);
                const bool hl = !nan_ray && l0 <= l1, hr = !nan_ray && r0 <= r1;   // bvh.h:177-180 (a NaN bound fails every test)
                if (hl) {
                    uint32_t near_i = li;
                    if (hr) {
                        uint32_t far_i = ri;
                        if (!Any && l0 > r0) { near_i = ri; far_i = li; }
                        push(far_i);
                    }
                    top = near_i;
                } else if (hr) {
                    top = ri;
                } else if (sp == 0) {
                    done = true;
                } else {
                    top = pop();
                }
            }
        }

        // ---- leaf (bvh.h:152-155 + test/benchmark.cpp:281-291) ------------------------------------------
        if (have && !done && (top & kCountMask) != 0) {
            const uint32_t first = top >> kCountBits, count = top & kCountMask;
            if (Stats) ++n_leaves;
            for (uint32_t i = first; i < first + count; ++i) {
                if (Stats) ++n_tests;
                if (Leaf == LEAF_TRIANGLE) {                            // tri.h:56-74
                    T p[12];
                    // (loading the TRIANGLES non-temporally as well was measured and costs 23-35 %: neighbouring rays share them through the L2;
                    //  profiles/r04_experiments_call4_hints.txt)
                    load_prim12(a.prims + static_cast<unsigned long long>(a.prim_stride) * i, p);
#define BVH_TRI_ACCEPTED hit_prim = i
#include "tri_test.inc"
#undef BVH_TRI_ACCEPTED
                } else {                                                // sphere.h:32-49
                    T qa, qb, qc;
                    if (D == 3) {
                        T s[4];
                        load_prim4(a.prims + 4ull * i, s);
                        const T o0 = org[0] - s[0], o1 = org[1] - s[1], o2 = org[2] - s[2];
                        qa = dot3(dir[0], dir[1], dir[2], dir[0], dir[1], dir[2]);
                        qb = T(2) * dot3(dir[0], dir[1], dir[2], o0, o1, o2);
                        qc = dot3(o0, o1, o2, o0, o1, o2) - s[3] * s[3];
                    } else {                                            // Sphere<T, 2>: {center[2], radius}
                        const T* s = a.prims + 3ull * i;
                        const T o0 = org[0] - s[0], o1 = org[1] - s[1];
                        qa = dot2(dir[0], dir[1], dir[0], dir[1]);
                        qb = T(2) * dot2(dir[0], dir[1], o0, o1);
                        qc = dot2(o0, o1, o0, o1) - s[2] * s[2];
                    }
                    const T delta = qb * qb - T(4) * qa * qc;
                    if (delta >= 0) {
                        const T iv = -T(0.5) / qa;
                        const T root = Num<T>::sqrt_(delta);
                        const T t0 = pick_max((qb + root) * iv, tmin);
                        const T t1 = pick_min((qb - root) * iv, tmax);
                        if (t0 <= t1) { tmax = t0; hit_t = t0; hit_u = t1; hit_v = 0; hit_prim = i; }
                    }
                }
            }
            if (Any && hit_prim != BVH_AMD_INVALID) done = true;
            else if (sp == 0) done = true;
            else top = pop();
        }

        // ---- retire finished rays --------------------------------------------------------------------
        if (have && done) {
            if (a.stream_hints & 1u) store_hit_nt(a.hits + ray_id, hit_prim, hit_t, hit_u, hit_v);
            else store_hit(a.hits + ray_id, hit_prim, hit_t, hit_u, hit_v);
            have = false;
        }
    }

#if defined(BVH_AMD_DEVELOPER) && defined(__HIPCC__)
    if (a.wave_times && lane == 0) {
        uint32_t xcc = 0;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        unsigned long long* w = a.wave_times + 6ull * (blockIdx.x * (kBlock / kWave) + (tid >> 6));
        w[0] = wt_begin; w[1] = wt_last_refill; w[2] = __builtin_amdgcn_s_memrealtime(); w[3] = (static_cast<unsigned long long>(xcc & 0xFu) << 32) | (wt_rays & 0xFFFFFFFFull);
        w[4] = wt_refill_ticks; w[5] = wt_refills;
    }
#endif
    if (Stats) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            n_pairs += __shfl_down(n_pairs, off);
            n_tests += __shfl_down(n_tests, off);
            n_leaves += __shfl_down(n_leaves, off);
        }
        if (lane == 0) {
            atomicAdd(&a.counters->node_pairs, n_pairs);
            atomicAdd(&a.counters->prim_tests, n_tests);
            atomicAdd(&a.counters->leaves, n_leaves);
        }
    }
