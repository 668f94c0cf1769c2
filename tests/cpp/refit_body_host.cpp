// TEST INFRASTRUCTURE (CPU, no GPU): compiles the text of the primitive-driven refit — bvh_amd/csrc/refit_body.inc: the per-leaf
// fold, the record-half store and the ticket climb — for the HOST and runs it with one emulated lane per node, the lanes one after
// another (the arrival counters then simply count). What it can show: the very source the device runs folds a leaf's primitives in
// the reference's order with its comparisons, writes each box into the right half of the right traversal record and leaves every
// inner box = left.extend(right). What it cannot show: the hand-off between workgroups (tests/test_gpu_refit_prims.py, and the ISA
// check in tests/test_refit_prims_host.py). tests/test_refit_prims_host.py drives it.
//
// Built by the tests with: g++ -std=c++20 -O1 -mavx2 -mfma -ffp-contract=off -fno-strict-aliasing -shared -fPIC -pthread.
#include <cstddef>
#include <cstdint>
#include <vector>

// ---- single-lane stand-ins for what hip_runtime.h provides ------------------------------------------------------------
#define __device__

// ---- stand-ins for bvh_amd/csrc/common.h (which needs the HIP headers) ------------------------------------------------------
namespace bvh_amd {
constexpr unsigned kCountBits = 4;
constexpr uint32_t kCountMask = 15u;
template <typename T> struct IndexOf;
template <> struct IndexOf<float>  { using Type = uint32_t; };
template <> struct IndexOf<double> { using Type = uint64_t; };
template <typename T> struct HostNode { T bounds[6]; typename IndexOf<T>::Type index; };
static_assert(sizeof(HostNode<float>) == 28 && sizeof(HostNode<double>) == 56);
template <typename T> struct PairNode;
template <> struct PairNode<float> { float lb[6], rb[6]; uint32_t li, ri; uint32_t pad[2]; };
template <> struct PairNode<double> { double lb[6], rb[6]; uint32_t li, ri; uint32_t pad[6]; };
static_assert(sizeof(PairNode<float>) == 64 && sizeof(PairNode<double>) == 128);
enum { REFIT_BOXES3 = 0, REFIT_BOXES2 = 1, REFIT_TRIS = 2 };
} // namespace bvh_amd

#define BVH_REFIT_LOAD(ptr) (*(ptr))
#define BVH_REFIT_STORE(ptr, v) (*(ptr) = (v))
#define BVH_REFIT_ARRIVE(counter) ((*(counter))++)

#include "../../bvh_amd/csrc/refit_body.inc"

namespace {

using namespace bvh_amd;

template <typename T, int Src>
void run(void* nodes_, void* pairs_, uint32_t n, const void* src, size_t n_src, const uint32_t* prim_ids, size_t prim_total) {
    auto nodes = static_cast<HostNode<T>*>(nodes_);
    auto pairs = static_cast<PairNode<T>*>(pairs_);
    std::vector<uint32_t> parent(n, 0xFFFFFFFFu), arrived(n, 0u);       // refit_prims.hip: the two memsets + k_refit_parents
    for (uint32_t i = 0; i < n; ++i) {
        if ((nodes[i].index & kCountMask) != 0) continue;
        const size_t f = static_cast<size_t>(nodes[i].index >> kCountBits);
        if (f == 0 || f + 1 >= n) continue;
        parent[f] = i; parent[f + 1] = i;
    }
    for (uint32_t i = 0; i < n; ++i)
        refit_lane<T, Src>(nodes, pairs, parent.data(), arrived.data(), n, static_cast<const T*>(src), n_src, prim_ids, prim_total, i);
}

template <typename T>
int run_src(int src_kind, void* nodes, void* pairs, uint32_t n, const void* src, size_t n_src, const uint32_t* prim_ids, size_t prim_total) {
    switch (src_kind) {
    case REFIT_BOXES3: run<T, REFIT_BOXES3>(nodes, pairs, n, src, n_src, prim_ids, prim_total); return 0;
    case REFIT_BOXES2: run<T, REFIT_BOXES2>(nodes, pairs, n, src, n_src, prim_ids, prim_total); return 0;
    case REFIT_TRIS:   run<T, REFIT_TRIS>(nodes, pairs, n, src, n_src, prim_ids, prim_total); return 0;
    }
    return -1;
}

template <typename T>
int fold_src(int src_kind, const void* src_, size_t n_src, const uint32_t* prim_ids, size_t prim_total, size_t first, uint32_t count, void* out6) {
    auto src = static_cast<const T*>(src_);
    T (&box)[6] = *static_cast<T (*)[6]>(out6);
    switch (src_kind) {
    case REFIT_BOXES3: refit_fold_leaf<T, REFIT_BOXES3>(src, n_src, prim_ids, prim_total, first, count, box); return 0;
    case REFIT_BOXES2: refit_fold_leaf<T, REFIT_BOXES2>(src, n_src, prim_ids, prim_total, first, count, box); return 0;
    case REFIT_TRIS:   refit_fold_leaf<T, REFIT_TRIS>(src, n_src, prim_ids, prim_total, first, count, box); return 0;
    }
    return -1;
}

} // namespace

extern "C" {

// nodes: n reference-layout nodes (28 / 56 bytes, 2D trees widened with z = 0), pairs: (n - 1) / 2 traversal records; both in place
int refit_host_run(int is_double, int src_kind, void* nodes, void* pairs, uint32_t n, const void* src, size_t n_src, const uint32_t* prim_ids,
                   size_t prim_total) {
    return is_double ? run_src<double>(src_kind, nodes, pairs, n, src, n_src, prim_ids, prim_total)
                     : run_src<float>(src_kind, nodes, pairs, n, src, n_src, prim_ids, prim_total);
}

// the fold of one leaf alone: out6 = {min.x, max.x, min.y, max.y, min.z, max.z}
int refit_host_fold(int is_double, int src_kind, const void* src, size_t n_src, const uint32_t* prim_ids, size_t prim_total, size_t first,
                    uint32_t count, void* out6) {
    return is_double ? fold_src<double>(src_kind, src, n_src, prim_ids, prim_total, first, count, out6)
                     : fold_src<float>(src_kind, src, n_src, prim_ids, prim_total, first, count, out6);
}

} // extern "C"
