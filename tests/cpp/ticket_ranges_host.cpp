// TEST INFRASTRUCTURE (CPU, no GPU): the ticket ranges of a reordered launch and the reordering key, compiled for the HOST from the
// device's own text. It takes the stand-ins and the emulated grid of tests/cpp/trace_body_host.cpp as they are (one emulated lane, or 64
// fibers with -DBVH_HOST_WAVE64; blocks run one after another, the last one first) and adds two entry points:
//   * ticket_ranges_host_trace — bvh_amd/csrc/trace_body.inc with EXPLICIT range starts (TraceArgs::range_starts), in ticket order or
//     through an order array, stagger on or off: what launch_traverse gives the kernel after ticket_ranges_kernel has run;
//   * ticket_ranges_host_keys — bvh_amd/csrc/ray_key.h on a batch of rays.
// tests/test_ticket_ranges_host.py drives it. Nothing here is shipped.
#include "trace_body_host.cpp"

inline int __clz(uint32_t x) { return x ? __builtin_clz(x) : 32; }
#include "../../bvh_amd/csrc/ray_key.h"

extern "C" {

// float / triangles / 3D, closest hit, robust, counters on: `parts` ranges [starts[p], starts[p + 1]) of the tickets 0..n-1 (starts holds
// parts + 1 words; NULL = equal slices), `order` (or NULL) maps a ticket to its ray. Grid and stagger: trace_body_host_set_grid.
int ticket_ranges_host_trace(const void* pairs64, uint32_t root_index, const float* tris12, const float* rays8, size_t n_rays, int parts, const uint32_t* starts,
                             const uint32_t* order, void* hits16, unsigned long long* counters3) {
    using namespace bvh_amd;
    if (parts < 1 || parts > 8) return 1;
    unsigned long long work[8 * kTicketStride] = {};
    bvh_amd_counters cnt = {0, 0, 0};
    TraceArgs<float> a;
    a.pairs = static_cast<const PairNode<float>*>(pairs64);
    a.prims = tris12; a.rays = rays8; a.hits = static_cast<bvh_hit3f*>(hits16);
    a.n = n_rays; a.work = work; a.parts = static_cast<uint32_t>(parts);
    a.part_size = parts > 1 ? ((n_rays + parts - 1) / parts + 63) / 64 * 64 : n_rays;
    a.range_starts = starts;
    a.counters = &cnt; a.order = order; a.deep = nullptr; a.deep_cap = 0; a.root_index = root_index;
    a.refill_threshold = kHostRefill; a.leaf_threshold = kHostLeaf;
    a.coop = 0; a.prim_stride = 12; a.stream_hints = 0; a.stagger = g_stagger; a.one_shot = 0; a.wave_times = nullptr;
    run_variant<float, LEAF_TRIANGLE, 3, false>(a, 0, 1);
    counters3[0] = cnt.node_pairs; counters3[1] = cnt.prim_tests; counters3[2] = cnt.leaves;
    return 0;
}

// keys[i] = ray_key(rays8[8 i ..]) over the box [lo, lo + cells / scale): the arguments of ray_keys_kernel (traverse.hip).
void ticket_ranges_host_keys(const float* rays8, size_t n, const float* lo3, const float* scale3, uint32_t cells, int hilbert_bits, int class_bits, float class_scale,
                             float tail_frac, uint32_t* keys) {
    for (size_t i = 0; i < n; ++i) {
        float r[8];
        for (int k = 0; k < 8; ++k) r[k] = rays8[8 * i + k];
        keys[i] = bvh_amd::ray_key<float>(r, lo3[0], lo3[1], lo3[2], scale3[0], scale3[1], scale3[2], cells, hilbert_bits, class_bits, class_scale, tail_frac);
    }
}

} // extern "C"
