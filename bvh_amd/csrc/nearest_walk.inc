// What the per-lane bodies of the nearest queries share (closest_body.inc, ray_nearest_body.inc, sphere_cast_body.inc,
// tri_distance_body.inc; knn_body.inc holds a copy of this text, for a measured reason it states): the one walk that
// visits the nearer child first, stacks the farther one with its key and drops whatever lies beyond a limit the caller lowers as it
// finds primitives. A key is a box's squared distance to the query point or to the query triangle's box, or the t at which a ray
// enters it (grown by the ball's radius: sphere-cast); the limit is the best squared distance or contact so far (closest,
// tri-distance, sphere-cast), or the key of the worst of the k candidates held (knn, nearest-hits: knn_heap.inc). The bodies
// supply the query, the two tests and the write-out. It is the keyed counterpart of list_walk.inc, which prunes nothing and stacks
// node words alone. Also here: kClosestLds, the LDS tier of the stack that closest, sphere-cast and tri-distance size by. Kept as an
// include so that the host harnesses (tests/cpp/closest_body_host.cpp, ray_nearest_body_host.cpp, sphere_cast_body_host.cpp,
// tri_distance_body_host.cpp) compile the very same text, through the bodies. Expects what point_walk.inc expects.
#pragma once

#include "point_walk.inc"

namespace bvh_amd {

namespace {

// Stack entries of a lane held in LDS ({node word, box distance^2} in two [depth][lane] arrays), the rest in scratch and HBM
// (point_walk.inc has the tiers). 8 entries in LDS (16 KB per block of float queries, 24 KB of double: 7 / 5-6 waves per
// SIMD, the VGPRs' limit) against 16 (5 / 3 waves, bound by LDS): 2^24 uniform queries on the 1M soup 12.10 -> 10.46 ms, on 1M f64
// spheres 15.10 -> 13.24 ms (DESIGN.md, "Closest-point queries").
constexpr int kClosestLds = 8;

// One query, one lane: depth-first walk from the root. nodes(lb, rb, kl, kr, hl, hr) tests the two child boxes of a record
// ({minx, maxx, miny, maxy, minz, maxz} each) against the query and the limit as it stands: the children's keys and whether each is
// entered. Of two entered children the walk takes the right one iff kr < kl (ties: left) and stacks the other with its key. A stacked
// entry is kept when it is popped iff key <= limit (not <: a primitive at the very limit with a lower index stays reachable wherever
// its box is not computed beyond it). Inside a leaf the BVH-order index ascends; leaf(i) tests primitive i and lowers `limit` (the
// caller's variable, read here through the reference) when it accepts it. Nothing is written: the caller's state is the result.
// No NaN reaches the comparison in `pop`: an entry is stacked only beside an entered sibling, and every nodes() enters a child only
// on a comparison its key takes part in (dl <= limit; l0 <= l1), which a NaN fails; the limit starts as max_distance^2 of a query
// whose max_distance >= 0, or as the non-NaN tmax of a ray, an invalid query is not walked (valid = false: leaf is never called),
// and leaf() lowers it only to a value that passed a comparison (d2 < best, d2 <= r2, tmin <= t <= tmax, t0 <= t1). So `key <= limit`
// and `!(key > limit)` are one predicate here.
// The stack's three tiers are point_walk.inc's: the first Lds entries in the two LDS arrays ({node word, key}, entry s of lane tid at
// s * stride + tid), the rest of kPointSmall in scratch, beyond that (Deep) in a.deep_nodes and deep_key, `lane` of the launch.
// push / pop are written here, on arrays this function names: see point_walk.inc on why they are not behind a struct.
// cnt += {pair records fetched, primitives tested, leaves visited}.
template <typename T, int Lds, bool Stats, bool Deep, typename Args, typename Nodes, typename Leaf>
__device__ inline void nearest_walk(const Args& a, bool valid, uint32_t* lds_node, T* lds_key, uint32_t stride, int tid, unsigned long long lane,
                                    T* deep_key, const T& limit, unsigned long long (&cnt)[3], Nodes nodes, Leaf leaf) {
    uint32_t spill_node[kPointSmall - Lds];
    T spill_key[kPointSmall - Lds];
    uint32_t sp = 0;
    auto push = [&](uint32_t node, T key) {
        if (sp < Lds) { lds_node[sp * stride + tid] = node; lds_key[sp * stride + tid] = key; }
        else if (!Deep || sp < kPointSmall) { const uint32_t i = stack_small_at<Lds>(sp); spill_node[i] = node; spill_key[i] = key; }
        else { const unsigned long long i = stack_deep_at(a, lane, sp); a.deep_nodes[i] = node; deep_key[i] = key; }
        ++sp;
    };
    // the next stacked entry that can still hold something within the limit (false: the walk is over)
    auto pop = [&](uint32_t& node) -> bool {
        while (sp > 0) {
            --sp;
            uint32_t e;
            T key;
            if (sp < Lds) { e = lds_node[sp * stride + tid]; key = lds_key[sp * stride + tid]; }
            else if (!Deep || sp < kPointSmall) { const uint32_t i = stack_small_at<Lds>(sp); e = spill_node[i]; key = spill_key[i]; }
            else { const unsigned long long i = stack_deep_at(a, lane, sp); e = a.deep_nodes[i]; key = deep_key[i]; }
            if (key <= limit) { node = e; return true; }
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
            T kl, kr;
            bool hl, hr;
            nodes(lb, rb, kl, kr, hl, hr);
            if (hl && hr) {
                if (kr < kl) { push(li, kl); node = ri; }
                else { push(ri, kr); node = li; }
            } else if (hl) node = li;
            else if (hr) node = ri;
            else if (!pop(node)) { live = false; break; }
        }
        if (!live) break;
        const uint32_t first = node >> kCountBits, count = node & kCountMask;
        if (Stats) ++cnt[2];
        for (uint32_t i = first; i < first + count; ++i) {
            if (Stats) ++cnt[1];
            leaf(i);
        }
        live = pop(node);
    }
}

} // namespace

} // namespace bvh_amd
