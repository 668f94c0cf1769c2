// The parents pass of the bottom-up climbs over arrival tickets (refit_prims.hip: k_refit_parents, winding.hip: k_winding_parents):
// compute_parents (reinsertion_optimizer.h:72-86) over a parent[] pre-filled with 0xFFFFFFFF, so that the root and the top of a subtree
// nothing references keep that mark. Expects kCountBits / kCountMask (common.h).
#pragma once

namespace bvh_amd {

// Node i of n with index word `index` (the reference layout's, or its 32-bit form in a traversal record): an inner node marks itself
// as the parent of its two children first_id, first_id + 1.
template <typename Index>
__device__ inline void climb_note_parent(Index index, uint32_t i, uint32_t n, uint32_t* parent) {
    if ((index & kCountMask) != 0) return;
    const size_t f = static_cast<size_t>(index >> kCountBits);
    if (f == 0 || f + 1 >= n) return;                         // (never in a validated tree)
    parent[f] = i;
    parent[f + 1] = i;
}

} // namespace bvh_amd
