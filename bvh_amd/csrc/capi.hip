// The C-ABI of libbvh_amd.so (include/bvh_amd.h). Thin: argument checks, handle ownership, host mirror
// bookkeeping; all compute is in the HIP kernels (traverse.hip, prep.hip, build_*.hip). No CPU fallback.
#include "common.h"

#include <cstring>
#include <memory>
#include <type_traits>

namespace bvh_amd {

template <typename T> int reinsertion_optimize_device(HostNode<T>* d_nodes, size_t node_count, hipStream_t stream, int dim);
template <typename T>
int reinsertion_optimize_config_device(HostNode<T>* d_nodes, size_t node_count, hipStream_t stream, int dim, double batch_size_ratio, size_t iterations);
void reinsertion_stats(unsigned out[2]);
void last_optimize_profile(bvh_amd_optimize_profile* out);
template <typename T>
int build_minitree_explicit(BvhImpl<T>& out, const T* d_bboxes, const T* d_centers, size_t n, const bvh_build_config& cfg, bool prune, T ratio,
                            bool optimize, uint32_t log2_grid, hipStream_t stream);
template <typename T>
int extract_device(BvhImpl<T>& out, const HostNode<T>* d_nodes, size_t node_count, const uint32_t* d_ids, size_t root_id, hipStream_t stream);
template <typename T> int refit_device(HostNode<T>* d_nodes, size_t node_count, hipStream_t stream);
template <typename T> int reachable_node_count(const HostNode<T>* d_nodes, size_t node_count, hipStream_t stream, size_t* out);
template <typename T> int relayout_on_device(BvhImpl<T>& b, const HostNode<T>* d_nodes, hipStream_t stream);

namespace {
thread_local std::string g_error;
}

void set_error(const std::string& msg) { g_error = msg; }
int fail(int code, const std::string& msg) { g_error = msg; return code; }
std::string current_error() { return g_error; }

namespace {

struct ThreadPoolTag { size_t thread_count; };   // opaque `bvh_thread_pool`: only its presence matters

// ---- the four families of the reference's C API (c_api/bvh.cpp:7-10): scalar T, dimension D. All of them are the same BvhImpl<T>:
// a 2D one has dim = 2, its inputs are widened to z = 0 on the device, and the host mirror its caller sees is BvhImpl::nodes2 in the
// reference's 20/40-byte layout. Everything below that depends on the family asks this trait.
template <typename T, int D> struct CTypes;
template <> struct CTypes<float, 3>  { using Bvh = bvh3f; using Node = bvh_node3f; using BBox = bvh_bbox3f; using Vec = bvh_vec3f; using Ray = bvh_ray3f; };
template <> struct CTypes<double, 3> { using Bvh = bvh3d; using Node = bvh_node3d; using BBox = bvh_bbox3d; using Vec = bvh_vec3d; using Ray = bvh_ray3d; };
template <> struct CTypes<float, 2>  { using Bvh = bvh2f; using Node = bvh_node2f; using BBox = bvh_bbox2f; using Vec = bvh_vec2f; using Ray = bvh_ray2f; };
template <> struct CTypes<double, 2> { using Bvh = bvh2d; using Node = bvh_node2d; using BBox = bvh_bbox2d; using Vec = bvh_vec2d; using Ray = bvh_ray2d; };

template <typename T, int D>
struct Family : CTypes<T, D> {
    using MirrorNode = std::conditional_t<D == 3, HostNode<T>, HostNode2<T>>;     // what `Node*` points at
    static constexpr int kBox = 2 * D, kVec = D, kRay = 2 * D + 2;                 // components of a BBox / Vec / Ray
    static_assert(sizeof(typename CTypes<T, D>::BBox) == kBox * sizeof(T) && sizeof(typename CTypes<T, D>::Vec) == kVec * sizeof(T) &&
                  sizeof(typename CTypes<T, D>::Ray) == kRay * sizeof(T));
    static constexpr int kRefitBoxes = D == 3 ? REFIT_BOXES3 : REFIT_BOXES2;
    static std::vector<MirrorNode>& mirror(const BvhImpl<T>& b) { if constexpr (D == 3) return b.nodes; else return b.nodes2; }
    static int sync_mirror(const BvhImpl<T>& b) { if constexpr (D == 3) return b.sync_host(); else return b.sync_host2(); }
    static int sphere_bounds(const T* d_prims, size_t n, T* d_bb, T* d_cc, hipStream_t s) {      // spheres {c, r} / circles {c, r}
        if constexpr (D == 3) return launch_sphere_bounds<T>(d_prims, n, d_bb, d_cc, s); else return launch_circle_bounds<T>(d_prims, n, d_bb, d_cc, s);
    }
};

template <typename T, int D> BvhImpl<T>* impl(typename Family<T, D>::Bvh* b) { return reinterpret_cast<BvhImpl<T>*>(b); }
template <typename T, int D> const BvhImpl<T>* impl(const typename Family<T, D>::Bvh* b) { return reinterpret_cast<const BvhImpl<T>*>(b); }
template <typename T, int D> typename Family<T, D>::Bvh* handle(BvhImpl<T>* b) { return reinterpret_cast<typename Family<T, D>::Bvh*>(b); }

// `who` works on a BVH of the current device only (`required` = false: an empty batch may name any BVH).
template <typename T>
int on_current_device(const BvhImpl<T>& b, const char* who, bool required = true) {
    int cur = -1;
    BVH_HIP_TRY(hipGetDevice(&cur), BVH_AMD_ERR_HIP);
    if (required && cur != b.device) return fail(BVH_AMD_ERR_ARG, std::string(who) + ": BVH lives on another device than the current one");
    return BVH_AMD_OK;
}

// Two temporary device buffers of one call, freed on every path out of it (after whatever the call waits for first).
template <typename T>
struct DeviceTemps {
    T *first = nullptr, *second = nullptr;
    DeviceTemps() = default;
    DeviceTemps(const DeviceTemps&) = delete;
    ~DeviceTemps() { if (first) (void)hipFree(first); if (second) (void)hipFree(second); }
};

bvh_build_config default_config() {               // default_builder.h:23-30, top_down_sah_builder.h:27-40
    bvh_build_config c;
    c.quality = BVH_BUILD_QUALITY_HIGH;
    c.min_leaf_size = 1;
    c.max_leaf_size = 8;
    c.parallel_threshold = 1024;
    return c;
}

// Runs `build` with the caller's SplitHeuristic in force (NULL = the reference's default {0, 1}).
template <typename Build>
auto with_sah(const bvh_amd_sah_config* sah, Build&& build) -> decltype(build()) {
    SahParams p;
    if (sah) {
        if (sah->log_cluster_size >= 64) { set_error("build: sah.log_cluster_size must be below 64 (split_heuristic.h:21, make_bitmask<size_t>)"); return nullptr; }
        p.log_cluster = static_cast<uint32_t>(sah->log_cluster_size);
        p.cost_ratio = sah->cost_ratio;
    }
    SahScope scope(p);
    return build();
}

// BinnedSahBuilder<Node, BinCount>::build (binned_sah_builder.h:18, :32-38) with a BinCount other than the reference's default
template <typename Build>
auto with_bins(const bvh_amd_sah_config* sah, size_t bin_count, Build&& build) -> decltype(build()) {
    if (bin_count != 4 && bin_count != 8 && bin_count != 16 && bin_count != 32) {
        set_error("build: bin_count must be 4, 8, 16 or 32 (BinnedSahBuilder's BinCount, binned_sah_builder.h:18)");
        return nullptr;
    }
    return with_sah(sah, [&] { ambient_sah().bin_count = static_cast<uint32_t>(bin_count); return build(); });
}

// `d_bboxes` / `d_centers` hold 2 * D / D components per primitive; the builders work on 6 / 3 (2D: widened into temporaries first).
template <typename T, int D>
typename Family<T, D>::Bvh* build_device(const T* d_bboxes, const T* d_centers, size_t n, const bvh_build_config* config,
                                         bvh_amd_builder builder, void* stream_)
{
    if (!d_bboxes || !d_centers || n == 0) { set_error("build: empty input (the reference's behaviour is undefined for 0 primitives)"); return nullptr; }
    bvh_build_config cfg = config ? *config : default_config();
    if (cfg.min_leaf_size < 1 || cfg.min_leaf_size > cfg.max_leaf_size || cfg.max_leaf_size > 15) {
        set_error("build: need 1 <= min_leaf_size <= max_leaf_size <= 15 (4-bit primitive count, index.h:38)");
        return nullptr;
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    auto b = std::make_unique<BvhImpl<T>>();
    b->dim = D;
    int rc;
    if constexpr (D == 3) {
        rc = build_on_device<T>(*b, d_bboxes, d_centers, n, cfg, builder, stream);
    } else {
        DeviceTemps<T> tmp;
        auto& [d_bb6, d_cc3] = tmp;
        BVH_HIP_TRY_PTR(hipMalloc(&d_bb6, n * 6 * sizeof(T)));
        hipError_t e = hipMalloc(&d_cc3, n * 3 * sizeof(T));
        rc = e == hipSuccess ? launch_widen_inputs<T>(d_bboxes, d_centers, n, d_bb6, d_cc3, stream)
                             : fail(BVH_AMD_ERR_HIP, std::string("build: ") + hipGetErrorString(e));
        if (rc == BVH_AMD_OK) rc = build_on_device<T>(*b, d_bb6, d_cc3, n, cfg, builder, stream);
        (void)hipStreamSynchronize(stream);
    }
    return rc == BVH_AMD_OK ? handle<T, D>(b.release()) : nullptr;
}

template <typename T>
typename Family<T, 3>::Bvh* build_minitree(const T* d_bboxes, const T* d_centers, size_t n, const bvh_amd_minitree_config* config, void* stream) {
    if (!d_bboxes || !d_centers || n == 0) { set_error("build: empty input"); return nullptr; }
    bvh_amd_minitree_config c = config ? *config : bvh_amd_minitree_config{1, 8, 1, 0.01, 1024, 4, 0, 1.0};
    if (c.min_leaf_size < 1 || c.min_leaf_size > c.max_leaf_size || c.max_leaf_size > 15) {
        set_error("build: need 1 <= min_leaf_size <= max_leaf_size <= 15 (4-bit primitive count, index.h:38)");
        return nullptr;
    }
    if (c.log2_grid_dim < 1 || c.log2_grid_dim > 10) {       // mini_tree_builder.h:169 asserts <= digits(MortonCode) / 3; 0 would be one cell
        set_error("build_minitree: log2_grid_dim must be in [1, 10] (three coordinates in a 32-bit Morton code, mini_tree_builder.h:169)");
        return nullptr;
    }
    bvh_build_config cfg = default_config();
    cfg.min_leaf_size = c.min_leaf_size; cfg.max_leaf_size = c.max_leaf_size; cfg.parallel_threshold = c.parallel_threshold;
    if (c.log_cluster_size >= 64) { set_error("build: log_cluster_size must be below 64 (split_heuristic.h:21)"); return nullptr; }
    SahParams sah;
    sah.log_cluster = static_cast<uint32_t>(c.log_cluster_size); sah.cost_ratio = c.cost_ratio;
    SahScope scope(sah);
    auto b = std::make_unique<BvhImpl<T>>();
    if (build_minitree_explicit<T>(*b, d_bboxes, d_centers, n, cfg, c.enable_pruning != 0, static_cast<T>(c.pruning_area_ratio), false,
                                   static_cast<uint32_t>(c.log2_grid_dim), static_cast<hipStream_t>(stream)) != BVH_AMD_OK)
        return nullptr;
    return handle<T, 3>(b.release());
}

template <typename T, int D>
typename Family<T, D>::Bvh* build_host(bvh_thread_pool* pool, const typename Family<T, D>::BBox* bboxes,
                                       const typename Family<T, D>::Vec* centers, size_t n, const bvh_build_config* config)
{
    using F = Family<T, D>;
    if (!bboxes || !centers || n == 0) { set_error("build: empty input"); return nullptr; }
    DeviceTemps<T> tmp;
    auto& [d_bb, d_cc] = tmp;
    BVH_HIP_TRY_PTR(hipMalloc(&d_bb, n * F::kBox * sizeof(T)));
    hipError_t e = hipMalloc(&d_cc, n * F::kVec * sizeof(T));
    if (e == hipSuccess) e = hipMemcpy(d_bb, bboxes, n * F::kBox * sizeof(T), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_cc, centers, n * F::kVec * sizeof(T), hipMemcpyHostToDevice);
    typename F::Bvh* out = nullptr;
    if (e == hipSuccess)
        out = build_device<T, D>(d_bb, d_cc, n, config, pool ? BVH_AMD_BUILDER_DEFAULT_PARALLEL : BVH_AMD_BUILDER_DEFAULT_SERIAL, nullptr);
    else
        set_error(std::string("build: ") + hipGetErrorString(e));
    (void)hipDeviceSynchronize();
    return out;
}

// A BVH around the mirror of `b`, filled in the family's layout by the caller (from_nodes / deserialize): uploaded, and handed out.
template <typename T, int D>
typename Family<T, D>::Bvh* adopt_mirror(std::unique_ptr<BvhImpl<T>> b) {
    b->dim = D;
    if constexpr (D == 2) b->widen_host();
    if (upload_bvh<T>(*b, nullptr) != BVH_AMD_OK) return nullptr;
    if constexpr (D == 2) b->nodes2_valid = true;
    return handle<T, D>(b.release());
}

template <typename T, int D>
typename Family<T, D>::Bvh* from_nodes(const void* nodes, size_t nn, const size_t* prim_ids, size_t np) {
    using F = Family<T, D>;
    if (!nodes || nn == 0 || (!prim_ids && np)) { set_error("from_nodes: null/empty input"); return nullptr; }
    auto b = std::make_unique<BvhImpl<T>>();
    F::mirror(*b).resize(nn);
    std::memcpy(F::mirror(*b).data(), nodes, nn * sizeof(typename F::MirrorNode));
    b->prim_ids.assign(prim_ids, prim_ids + np);
    return adopt_mirror<T, D>(std::move(b));
}

// Byte stream of Bvh::serialize (bvh.h:221-229): [node_count][prim_count] in Index::Type, Node<T, D> records, prim ids.
template <typename T, int D>
size_t stream_size(const BvhImpl<T>& b) {
    using I = typename IndexOf<T>::Type;
    return 2 * sizeof(I) + b.node_count * sizeof(typename Family<T, D>::MirrorNode) + b.prim_count * sizeof(I);
}

template <typename T, int D>
size_t serialize(const BvhImpl<T>& b, void* out, size_t cap) {
    using F = Family<T, D>;
    using I = typename IndexOf<T>::Type;
    const size_t need = stream_size<T, D>(b);
    if (!out || cap < need) return need;
    if (F::sync_mirror(b) != BVH_AMD_OK) return 0;
    const auto& nodes = F::mirror(b);
    auto p = static_cast<uint8_t*>(out);
    I hdr[2] = { static_cast<I>(nodes.size()), static_cast<I>(b.prim_ids.size()) };
    std::memcpy(p, hdr, sizeof(hdr)); p += sizeof(hdr);
    std::memcpy(p, nodes.data(), nodes.size() * sizeof(nodes[0])); p += nodes.size() * sizeof(nodes[0]);
    for (size_t id : b.prim_ids) { I v = static_cast<I>(id); std::memcpy(p, &v, sizeof(v)); p += sizeof(v); }
    return need;
}

template <typename T, int D>
typename Family<T, D>::Bvh* deserialize(const void* bytes, size_t size) {
    using F = Family<T, D>;
    using I = typename IndexOf<T>::Type;
    constexpr size_t node_bytes = sizeof(typename F::MirrorNode);
    if (!bytes || size < 2 * sizeof(I)) { set_error("deserialize: truncated stream"); return nullptr; }
    auto p = static_cast<const uint8_t*>(bytes);
    I hdr[2];
    std::memcpy(hdr, p, sizeof(hdr)); p += sizeof(hdr);
    const size_t nn = hdr[0], np = hdr[1];
    if (nn > size / node_bytes || np > size / sizeof(I) ||                     // (bounded first: a crafted header must not overflow the sum)
        size < 2 * sizeof(I) + nn * node_bytes + np * sizeof(I)) { set_error("deserialize: truncated stream"); return nullptr; }
    auto b = std::make_unique<BvhImpl<T>>();
    F::mirror(*b).resize(nn);
    std::memcpy(F::mirror(*b).data(), p, nn * node_bytes); p += nn * node_bytes;
    b->prim_ids.resize(np);
    for (size_t i = 0; i < np; ++i) { I v; std::memcpy(&v, p, sizeof(v)); p += sizeof(v); b->prim_ids[i] = static_cast<size_t>(v); }
    return adopt_mirror<T, D>(std::move(b));
}

template <typename T, int D>
void save(const BvhImpl<T>& b, FILE* f) {
    std::vector<uint8_t> buf(stream_size<T, D>(b));
    serialize<T, D>(b, buf.data(), buf.size());
    fwrite(buf.data(), 1, buf.size(), f);
}

template <typename T, int D>
typename Family<T, D>::Bvh* load(FILE* f) {
    using I = typename IndexOf<T>::Type;
    constexpr size_t node_bytes = sizeof(typename Family<T, D>::MirrorNode);
    I hdr[2] = {0, 0};
    if (fread(hdr, sizeof(I), 2, f) != 2) { set_error("load: truncated stream"); return nullptr; }
    std::vector<uint8_t> buf;
    try { buf.resize(2 * sizeof(I) + size_t(hdr[0]) * node_bytes + size_t(hdr[1]) * sizeof(I)); }
    catch (const std::exception&) { set_error("load: the header asks for more memory than there is"); return nullptr; }   // (never across the C ABI)
    std::memcpy(buf.data(), hdr, sizeof(hdr));
    size_t rest = buf.size() - sizeof(hdr);
    if (fread(buf.data() + sizeof(hdr), 1, rest, f) != rest) { set_error("load: truncated stream"); return nullptr; }
    return deserialize<T, D>(buf.data(), buf.size());
}

// The reference-layout nodes resident on the device, with possible host-side edits pushed.
template <typename T>
int make_nodes_resident(BvhImpl<T>& b) {
    if (b.node_count == 0) return fail(BVH_AMD_ERR_ARG, "empty bvh");
    if (b.dim == 2 && b.host_valid && b.nodes2_valid) b.widen_host();    // 2D: the caller edits the narrow mirror
    const size_t bytes = b.node_count * sizeof(HostNode<T>);
    if (b.d_nodes && b.d_nodes_count != b.node_count) {        // nodes were appended / removed on the host
        (void)hipFree(b.d_nodes);
        b.d_nodes = nullptr;
    }
    if (!b.d_nodes) {                                          // BVH came from the host (from_nodes / load): make it resident
        if (!b.host_valid || b.nodes.size() != b.node_count) return fail(BVH_AMD_ERR_ARG, "the BVH has neither a resident nor a host copy of its nodes");
        BVH_HIP_TRY(hipMalloc(&b.d_nodes, bytes), BVH_AMD_ERR_HIP);
        b.d_nodes_count = b.node_count;
        BVH_HIP_TRY(hipMemcpy(b.d_nodes, b.nodes.data(), bytes, hipMemcpyHostToDevice), BVH_AMD_ERR_HIP);
    } else if (b.host_valid) {                                 // the host mirror may have been edited through bvh_node* pointers
        BVH_HIP_TRY(hipMemcpy(b.d_nodes, b.nodes.data(), bytes, hipMemcpyHostToDevice), BVH_AMD_ERR_HIP);
    } else {
        return BVH_AMD_OK;                                     // resident nodes written by the device builders / a validated upload
    }
    // whatever came from the host mirror may have been edited by the caller (bvh_node*_set_*): the kernels that walk these nodes
    // (refit, optimize, extract, the traversal records built from them) rely on the structure wire.hip checks
    return validate_resident_nodes<T>(b.d_nodes, b.node_count, b.prim_count, nullptr, "sync (host mirror -> device)");
}

// Bvh::serialize into / Bvh::deserialize out of DEVICE memory (wire.hip): the broadcast payload never visits the host.
template <typename T>
size_t serialize_device(BvhImpl<T>* pb, void* d_out, size_t cap, void* stream) {
    if (!pb) { set_error("serialize_device: null bvh"); return 0; }
    const size_t need = wire_size<T>(*pb);
    if (!d_out || cap < need) return need;
    if (make_nodes_resident<T>(*pb)) return 0;
    return serialize_to_device<T>(*pb, d_out, cap, static_cast<hipStream_t>(stream));
}

// Runs `op` (optimize / refit) on the resident reference-layout nodes, then refreshes the traversal records and (if it was
// valid) the host mirror.
template <typename T, typename Op>
int on_resident_nodes(BvhImpl<T>* pb, Op op) {
    if (!pb) return fail(BVH_AMD_ERR_ARG, "null bvh");
    BvhImpl<T>& b = *pb;
    int rc = b.wait_refit();                                   // (a pending root refresh of refit_boxes / refit_tris must not overwrite the one below)
    if (rc) return rc;
    rc = make_nodes_resident<T>(b);
    if (rc) return rc;
    const size_t bytes = b.node_count * sizeof(HostNode<T>);
    rc = op(b.d_nodes, b.node_count);
    if (rc) return rc;
    rc = relayout_on_device<T>(b, b.d_nodes, nullptr);
    if (rc) return rc;
    HostNode<T> root;
    BVH_HIP_TRY(hipMemcpy(&root, b.d_nodes, sizeof(root), hipMemcpyDeviceToHost), BVH_AMD_ERR_HIP);
    b.root_index = static_cast<uint32_t>(root.index);
    for (int k = 0; k < 6; ++k) b.root_bounds[k] = root.bounds[k];
    if (b.host_valid) BVH_HIP_TRY(hipMemcpy(b.nodes.data(), b.d_nodes, bytes, hipMemcpyDeviceToHost), BVH_AMD_ERR_HIP);
    b.nodes2_valid = false;
    return BVH_AMD_OK;
}

template <typename T> BvhImpl<T>* extract(BvhImpl<T>* pb, size_t root_id) {
    if (!pb) { set_error("extract: null bvh"); return nullptr; }
    BvhImpl<T>& b = *pb;
    if (b.wait_refit()) return nullptr;                        // (a refit_* in flight on a non-blocking stream is not ordered before the copy-out below)
    if (make_nodes_resident<T>(b)) return nullptr;
    if (!b.d_prim_ids) { set_error("extract: the BVH has no device prim ids"); return nullptr; }
    auto out = std::make_unique<BvhImpl<T>>();
    out->dim = b.dim;
    if (extract_device<T>(*out, b.d_nodes, b.node_count, b.d_prim_ids, root_id, nullptr)) return nullptr;
    return out.release();
}

// The ReinsertionOptimizer walks parent links from every candidate to the root (reinsertion_optimizer.h:107-188). On an array that
// also holds nodes nothing reachable references — tolerated on the way in (wire.hip), like the reference tolerates them — the
// reference's zero-initialised parents_ (:74) would make such a node a child of the root and corrupt the tree, and a cycle among
// unreachable nodes would never reach the root at all. Refused here, before anything is touched: optimize wants a proper tree.
template <typename T> int whole_array_is_one_tree(const HostNode<T>* d, size_t n) {
    size_t reachable = 0;
    const int rc = reachable_node_count<T>(d, n, nullptr, &reachable);
    if (rc) return rc;
    if (reachable != n)
        return fail(BVH_AMD_ERR_UNSUPPORTED, "optimize: " + std::to_string(n - reachable) + " of the " + std::to_string(n) +
                    " nodes are not reachable from the root (unused sibling pairs); extract_bvh(0) first, or remove them");
    return BVH_AMD_OK;
}
template <typename T> int optimize(BvhImpl<T>* b) {
    const int dim = b ? b->dim : 3;
    return on_resident_nodes<T>(b, [dim](HostNode<T>* d, size_t n) {
        const int rc = whole_array_is_one_tree<T>(d, n);
        return rc ? rc : reinsertion_optimize_device<T>(d, n, nullptr, dim);
    });
}
template <typename T> int optimize_config(BvhImpl<T>* b, const bvh_amd_optimize_config* config) {
    const int dim = b ? b->dim : 3;
    const bvh_amd_optimize_config c = config ? *config : bvh_amd_optimize_config{0.05, 3};
    return on_resident_nodes<T>(b, [dim, c](HostNode<T>* d, size_t n) {
        const int rc = whole_array_is_one_tree<T>(d, n);
        return rc ? rc : reinsertion_optimize_config_device<T>(d, n, nullptr, dim, c.batch_size_ratio, c.max_iter_count);
    });
}
template <typename T> int refit(BvhImpl<T>* b) {
    return on_resident_nodes<T>(b, [](HostNode<T>* d, size_t n) { return refit_device<T>(d, n, nullptr); });
}

// bvhXX_refit_boxes / bvh3X_refit_tris: leaf boxes from primitives in HBM, inner boxes bottom-up, reference-layout nodes and traversal
// records updated in place on the caller's stream (refit_prims.hip). What depends on the topology only — max_depth, the measured
// launch plan, d_prim_ids, the work slots — is kept; the host mirror is marked stale and refilled lazily by sync_host().
// One-offs, not paid per frame: the largest prim id (one read-back, cached per tree), and, when the mirror holds the only or a
// possibly edited copy of the nodes (host_valid), the push + validation + re-layout that bvhXX_refit does on every call.
template <typename T>
int refit_prims(BvhImpl<T>* pb, int src_kind, const T* d_src, size_t n_src, T* d_tris12_out, void* stream_, const char* who) {
    if (!pb) return fail(BVH_AMD_ERR_ARG, std::string(who) + ": null bvh");
    if (!d_src) return fail(BVH_AMD_ERR_ARG, std::string(who) + ": null primitive array");
    BvhImpl<T>& b = *pb;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (const int rc = on_current_device(b, who)) return rc;
    if (b.node_count == 0 || !b.d_prim_ids) return fail(BVH_AMD_ERR_ARG, std::string(who) + ": BVH has no device copy");
    if (const int rc = source_array_check(b, n_src, "primitives", who, stream)) return rc;
    // (no wait for an earlier refit_*'s root copy here: note_refit() below supersedes it, and the host blocks on nothing in the steady
    //  state; the mirror can only be valid after sync_host(), which has waited)
    const bool from_host = b.host_valid || !b.d_nodes || b.d_nodes_count != b.node_count;
    int rc = from_host ? b.wait_refit() : BVH_AMD_OK;
    if (rc) return rc;
    rc = make_nodes_resident<T>(b);
    if (rc) return rc;
    if (from_host || (b.pair_count && !b.d_pairs)) {           // index words may have been edited: the records are rebuilt (and the plan with them)
        const long long largest = b.max_prim_id.load();
        rc = relayout_on_device<T>(b, b.d_nodes, stream);
        if (rc) return rc;
        b.max_prim_id = largest;                               // (prim_ids cannot be edited through the mirror)
    }
    rc = refit_prims_device<T>(b.d_nodes, b.d_pairs, b.node_count, src_kind, d_src, n_src, b.d_prim_ids, b.prim_count, stream);
    if (rc == BVH_AMD_OK && d_tris12_out) rc = launch_precompute_tris<T>(d_src, b.d_prim_ids, b.prim_count, d_tris12_out, stream);
    // the boxes on the device are ahead of the mirror from here on, also after a failed launch
    b.host_valid = false;
    b.nodes2_valid = false;
    const int rc2 = b.note_refit(stream);
    return rc ? rc : rc2;
}

template <typename T>
int traversal_cost_checked(const BvhImpl<T>* b, double* cost_out, void* stream) {
    if (!b || !cost_out) return fail(BVH_AMD_ERR_ARG, "traversal_cost: null bvh or output");
    if (const int rc = on_current_device(*b, "traversal_cost")) return rc;
    return traversal_cost<T>(*b, cost_out, static_cast<hipStream_t>(stream));
}

template <typename T>
int prepare_trace_checked(const BvhImpl<T>* b, size_t n_rays_hint, void* stream) {
    if (!b) return fail(BVH_AMD_ERR_ARG, "prepare_trace: null bvh");
    if (const int rc = on_current_device(*b, "prepare_trace")) return rc;
    return prepare_trace<T>(*b, n_rays_hint, static_cast<hipStream_t>(stream));
}

// Host-side edits (bvh_node* setters, append/remove) live in the mirror; this pushes them to the device copy.
template <typename T> int sync_device(BvhImpl<T>* pb) {
    if (!pb) return fail(BVH_AMD_ERR_ARG, "sync_device: null bvh");
    BvhImpl<T>& b = *pb;
    int rc = b.dim == 2 ? b.sync_host2() : b.sync_host();
    if (rc) return rc;
    if (b.dim == 2) b.widen_host();
    if (b.d_nodes) { (void)hipFree(b.d_nodes); b.d_nodes = nullptr; }
    return upload_bvh<T>(b, nullptr);
}

// ---- the host mirror through the family's `Node*` (c_api/bvh.h:170-218). A caller's edits reach the device with sync_device --------
template <typename T, int D> auto* mirror_node(typename Family<T, D>::Node* n) { return reinterpret_cast<typename Family<T, D>::MirrorNode*>(n); }
template <typename T, int D> auto* mirror_node(const typename Family<T, D>::Node* n) { return reinterpret_cast<const typename Family<T, D>::MirrorNode*>(n); }

template <typename T, int D> void set_prim_count(typename Family<T, D>::Node* n, size_t c) {
    using I = typename IndexOf<T>::Type;
    auto h = mirror_node<T, D>(n);
    h->index = (h->index & ~static_cast<I>(kCountMask)) | (static_cast<I>(c) & kCountMask);
}
template <typename T, int D> void set_first_id(typename Family<T, D>::Node* n, size_t f) {
    auto h = mirror_node<T, D>(n);
    h->index = (static_cast<typename IndexOf<T>::Type>(f) << kCountBits) | (h->index & kCountMask);
}
template <typename T, int D> bool is_leaf(const typename Family<T, D>::Node* n) { return (mirror_node<T, D>(n)->index & kCountMask) != 0; }
template <typename T, int D> size_t get_prim_count(const typename Family<T, D>::Node* n) { return mirror_node<T, D>(n)->index & kCountMask; }
template <typename T, int D> size_t get_first_id(const typename Family<T, D>::Node* n) { return mirror_node<T, D>(n)->index >> kCountBits; }

// A BBox is {min[D], max[D]}, a node's bounds are {min, max} per axis.
template <typename T, int D> void set_bbox(typename Family<T, D>::Node* n, const typename Family<T, D>::BBox* bb) {
    auto h = mirror_node<T, D>(n);
    T v[2 * D];
    std::memcpy(v, bb, sizeof(v));
    for (int k = 0; k < D; ++k) { h->bounds[2 * k] = v[k]; h->bounds[2 * k + 1] = v[D + k]; }
}
template <typename T, int D> typename Family<T, D>::BBox get_bbox(const typename Family<T, D>::Node* n) {
    auto h = mirror_node<T, D>(n);
    T v[2 * D];
    for (int k = 0; k < D; ++k) { v[k] = h->bounds[2 * k]; v[D + k] = h->bounds[2 * k + 1]; }
    typename Family<T, D>::BBox r;
    std::memcpy(&r, v, sizeof(r));
    return r;
}

template <typename T, int D> typename Family<T, D>::Node* get_node(BvhImpl<T>* b, size_t i) {
    if (Family<T, D>::sync_mirror(*b) != BVH_AMD_OK) return nullptr;
    return reinterpret_cast<typename Family<T, D>::Node*>(&Family<T, D>::mirror(*b)[i]);
}
template <typename T, int D> void append_node(BvhImpl<T>* b) {
    auto& nodes = Family<T, D>::mirror(*b);
    if (Family<T, D>::sync_mirror(*b) != BVH_AMD_OK) return;
    nodes.emplace_back();
    b->node_count = nodes.size();
}
template <typename T, int D> void remove_last_node(BvhImpl<T>* b) {
    auto& nodes = Family<T, D>::mirror(*b);
    if (Family<T, D>::sync_mirror(*b) != BVH_AMD_OK || nodes.empty()) return;
    nodes.pop_back();
    b->node_count = nodes.size();
}
template <typename T, int D> void copy_nodes(const BvhImpl<T>* b, void* out) {
    const auto& nodes = Family<T, D>::mirror(*b);
    if (Family<T, D>::sync_mirror(*b) != BVH_AMD_OK) return;
    std::memcpy(out, nodes.data(), nodes.size() * sizeof(nodes[0]));
}
// (the prim ids are filled by sync_host() in every family)
template <typename T> size_t get_prim_id(const BvhImpl<T>* b, size_t i) {
    if (b->sync_host() != BVH_AMD_OK) return BVH_INVALID_PRIM_ID;
    return b->prim_ids[i];
}
template <typename T> void copy_prim_ids(const BvhImpl<T>* b, size_t* out) {
    if (b->sync_host() != BVH_AMD_OK) return;
    std::memcpy(out, b->prim_ids.data(), b->prim_ids.size() * sizeof(size_t));
}

// bvhXX_intersect_rays_*: a batch of the family's rays (2 * D + 2 components each) through the tree; 2D has circles only (LEAF_SPHERE).
template <typename T, int D>
int intersect(const typename Family<T, D>::Bvh* bvh, int leaf, const T* d_prims, const typename Family<T, D>::Ray* d_rays, size_t n,
              unsigned flags, typename HitOf<T>::Type* d_hits, bvh_amd_counters* d_counters, void* stream)
{
    if (!bvh) return fail(BVH_AMD_ERR_ARG, "intersect_rays: null bvh");
    const BvhImpl<T>& b = *impl<T, D>(bvh);
    if (const int rc = on_current_device(b, "intersect_rays")) return rc;
    return launch_traverse<T>(b, leaf, d_prims, reinterpret_cast<const T*>(d_rays), n, flags, d_hits, d_counters,
                              static_cast<hipStream_t>(stream));
}

// The tree behind a point query `who` (closest_points, radius_search, knn): it must live on the current device, unless the batch is empty.
template <typename T>
int point_query_tree(const typename Family<T, 3>::Bvh* bvh, size_t n, const char* who, const BvhImpl<T>** b)
{
    if (!bvh) return fail(BVH_AMD_ERR_ARG, std::string(who) + ": null bvh");
    *b = impl<T, 3>(bvh);
    return on_current_device(**b, who, n != 0);
}

template <typename T>
int closest(const typename Family<T, 3>::Bvh* bvh, int leaf, const T* d_prims, const T* d_queries4, size_t n, unsigned flags,
            typename HitOf<T>::Type* d_hits, bvh_amd_counters* d_counters, void* stream)
{
    const BvhImpl<T>* b = nullptr;
    if (const int rc = point_query_tree<T>(bvh, n, "closest_points", &b)) return rc;
    return launch_closest<T>(*b, leaf, d_prims, d_queries4, n, flags, d_hits, d_counters, static_cast<hipStream_t>(stream));
}

template <typename T>
int radius_search(const typename Family<T, 3>::Bvh* bvh, int leaf, const T* d_prims, const T* d_queries4, size_t n, unsigned flags, uint32_t* d_counts,
                  const uint64_t* d_offsets, uint32_t* d_list_prims, T* d_list_dist, bvh_amd_counters* d_counters, void* stream)
{
    const BvhImpl<T>* b = nullptr;
    if (const int rc = point_query_tree<T>(bvh, n, "radius_search", &b)) return rc;
    return launch_radius<T>(*b, leaf, d_prims, d_queries4, n, flags, d_counts, d_offsets, d_list_prims, d_list_dist, d_counters,
                            static_cast<hipStream_t>(stream));
}

template <typename T>
int knn(const typename Family<T, 3>::Bvh* bvh, int leaf, const T* d_prims, const T* d_queries4, size_t n, unsigned k, unsigned flags, uint32_t* d_out_prims,
        T* d_out_dist, uint32_t* d_counts, bvh_amd_counters* d_counters, void* stream)
{
    const BvhImpl<T>* b = nullptr;
    if (const int rc = point_query_tree<T>(bvh, n, "knn", &b)) return rc;
    return launch_knn<T>(*b, leaf, d_prims, d_queries4, n, k, flags, d_out_prims, d_out_dist, d_counts, d_counters, static_cast<hipStream_t>(stream));
}

template <typename T>
int winding_prepare(const typename Family<T, 3>::Bvh* bvh, const T* d_tris12, T* d_moments, size_t moments_rows, void* stream)
{
    const BvhImpl<T>* b = nullptr;
    if (const int rc = point_query_tree<T>(bvh, 1, "winding_prepare", &b)) return rc;
    return launch_winding_prepare<T>(*b, d_tris12, d_moments, moments_rows, static_cast<hipStream_t>(stream));
}

template <typename T>
int winding_numbers(const typename Family<T, 3>::Bvh* bvh, const T* d_tris12, const T* d_moments, size_t moments_rows, const T* d_queries4, size_t n,
                    double beta, unsigned flags, T* d_w, typename HitOf<T>::Type* d_hits, bvh_amd_counters* d_counters, void* stream)
{
    const BvhImpl<T>* b = nullptr;
    if (const int rc = point_query_tree<T>(bvh, n, "winding_numbers", &b)) return rc;
    return launch_winding<T>(*b, d_tris12, d_moments, moments_rows, d_queries4, n, beta, flags, d_w, d_hits, d_counters, static_cast<hipStream_t>(stream));
}

template <typename T>
int ray_hits(const typename Family<T, 3>::Bvh* bvh, int leaf, const T* d_prims, const typename Family<T, 3>::Ray* d_rays, size_t n, unsigned flags,
             uint32_t* d_counts, const uint64_t* d_offsets, typename HitOf<T>::Type* d_list_hits, bvh_amd_counters* d_counters, void* stream)
{
    const BvhImpl<T>* b = nullptr;
    if (const int rc = point_query_tree<T>(bvh, n, "intersect_rays_all", &b)) return rc;
    return launch_ray_hits<T>(*b, leaf, d_prims, reinterpret_cast<const T*>(d_rays), n, flags, d_counts, d_offsets, d_list_hits, d_counters,
                              static_cast<hipStream_t>(stream));
}

template <typename T>
int ray_nearest(const typename Family<T, 3>::Bvh* bvh, int leaf, const T* d_prims, const typename Family<T, 3>::Ray* d_rays, size_t n, unsigned k,
                unsigned flags, typename HitOf<T>::Type* d_out_hits, uint32_t* d_counts, bvh_amd_counters* d_counters, void* stream)
{
    const BvhImpl<T>* b = nullptr;
    if (const int rc = point_query_tree<T>(bvh, n, "intersect_rays_nearest", &b)) return rc;
    return launch_ray_nearest<T>(*b, leaf, d_prims, reinterpret_cast<const T*>(d_rays), n, k, flags, d_out_hits, d_counts, d_counters,
                                 static_cast<hipStream_t>(stream));
}

template <typename T>
int sphere_cast(const typename Family<T, 3>::Bvh* bvh, int leaf, const T* d_prims, const typename Family<T, 3>::Ray* d_rays, size_t n, T radius,
                const T* d_radii, unsigned flags, typename HitOf<T>::Type* d_hits, bvh_amd_counters* d_counters, void* stream)
{
    const BvhImpl<T>* b = nullptr;
    if (const int rc = point_query_tree<T>(bvh, n, "sphere_cast", &b)) return rc;
    return launch_sphere_cast<T>(*b, leaf, d_prims, reinterpret_cast<const T*>(d_rays), n, radius, d_radii, flags, d_hits, d_counters,
                                 static_cast<hipStream_t>(stream));
}

// bvh3X_overlap_boxes / bvh3X_overlap_self: d_queries6 = NULL and n = the tree's primitive count in self mode.
template <typename T>
int overlap(const typename Family<T, 3>::Bvh* bvh, bool self, const T* d_bboxes, size_t n_boxes, const T* d_queries6, size_t n, unsigned flags,
            uint32_t* d_counts, const uint64_t* d_offsets, uint32_t* d_list_prims, bvh_amd_counters* d_counters, void* stream)
{
    const char* who = self ? "overlap_self" : "overlap_boxes";
    const BvhImpl<T>* b = nullptr;
    if (const int rc = point_query_tree<T>(bvh, self ? 1 : n, who, &b)) return rc;
    return launch_overlap<T>(*b, self, d_bboxes, n_boxes, d_queries6, self ? b->prim_count : n, flags, d_counts, d_offsets, d_list_prims, d_counters,
                             static_cast<hipStream_t>(stream));
}

// bvh3X_intersect_tris / bvh3X_intersect_tris_self: d_queries9 = NULL and n = the tree's primitive count in self mode.
template <typename T>
int intersect_tris(const typename Family<T, 3>::Bvh* bvh, bool self, const T* d_tris9, size_t n_tris, const T* d_queries9, size_t n, unsigned flags,
                   uint32_t* d_counts, const uint64_t* d_offsets, uint32_t* d_list_prims, bvh_amd_counters* d_counters, void* stream)
{
    const char* who = self ? "intersect_tris_self" : "intersect_tris";
    const BvhImpl<T>* b = nullptr;
    if (const int rc = point_query_tree<T>(bvh, self ? 1 : n, who, &b)) return rc;
    return launch_tri_intersect<T>(*b, self, d_tris9, n_tris, d_queries9, self ? b->prim_count : n, flags, d_counts, d_offsets, d_list_prims, d_counters,
                                   static_cast<hipStream_t>(stream));
}

template <typename T>
int tri_distance(const typename Family<T, 3>::Bvh* bvh, const T* d_tris9, size_t n_tris, const T* d_queries9, size_t n, T max_distance,
                 const T* d_max_distances, unsigned flags, typename HitOf<T>::Type* d_hits, T* d_query_uv, bvh_amd_counters* d_counters, void* stream)
{
    const BvhImpl<T>* b = nullptr;
    if (const int rc = point_query_tree<T>(bvh, n, "tri_distance", &b)) return rc;
    return launch_tri_distance<T>(*b, d_tris9, n_tris, d_queries9, n, max_distance, d_max_distances, flags, d_hits, d_query_uv, d_counters,
                                  static_cast<hipStream_t>(stream));
}

template <typename T>
int region(const typename Family<T, 3>::Bvh* bvh, int leaf, const T* d_prims, size_t n_prims, const T* d_planes, size_t m, size_t n, unsigned flags,
           uint32_t* d_counts, const uint64_t* d_offsets, uint32_t* d_list_prims, uint8_t* d_list_inside, bvh_amd_counters* d_counters, void* stream)
{
    const BvhImpl<T>* b = nullptr;
    if (const int rc = point_query_tree<T>(bvh, n, leaf == LEAF_TRIANGLE ? "region_tris" : "region_spheres", &b)) return rc;
    return launch_region<T>(*b, leaf, d_prims, n_prims, d_planes, m, n, flags, d_counts, d_offsets, d_list_prims, d_list_inside, d_counters,
                            static_cast<hipStream_t>(stream));
}

// bvh3X_instance_prepare / bvh3X_intersect_rays_instanced: struct bvh_amd_geometry3X is GeomRef<T> by layout (a handle is its BvhImpl).
template <typename T, typename Geometry>
const GeomRef<T>* geom_refs(const Geometry* geoms) {
    static_assert(sizeof(Geometry) == sizeof(GeomRef<T>) && offsetof(Geometry, d_tris12) == offsetof(GeomRef<T>, d_tris12));
    return reinterpret_cast<const GeomRef<T>*>(geoms);
}

template <typename T, typename Geometry>
int intersect_instanced(const typename Family<T, 3>::Bvh* top, const Geometry* geoms, size_t n_geoms, const T* d_world2obj, const uint32_t* d_geometry,
                        size_t n_instances, const typename Family<T, 3>::Ray* d_rays, size_t n_rays, unsigned flags, typename HitOf<T>::Type* d_hits,
                        uint32_t* d_hit_instances, bvh_amd_counters* d_counters, void* stream)
{
    const BvhImpl<T>* b = nullptr;
    if (const int rc = point_query_tree<T>(top, n_rays, "intersect_rays_instanced", &b)) return rc;
    return launch_instanced<T>(*b, geom_refs<T>(geoms), n_geoms, d_world2obj, d_geometry, n_instances, reinterpret_cast<const T*>(d_rays), n_rays, flags,
                               d_hits, d_hit_instances, d_counters, static_cast<hipStream_t>(stream));
}

// bvhXX_intersect_ray{,_any}{,_robust} (c_api/bvh.h:277-295 over bvh_impl.h:235-250): one ray, the leaves go to the caller's
// function. The walk runs on the device (ray_callback.hip, ray_step_kernel); `ray` is the family's own struct.
template <typename T, int D>
int intersect_ray_visit(const BvhImpl<T>* b, const void* ray, size_t start, unsigned flags, bool (*leaf_fn)(void*, T*, size_t, size_t),
                        void (*inner_fn)(void*, size_t), void* user) {
    if (!b || !ray) return fail(BVH_AMD_ERR_ARG, "intersect_ray: null bvh or ray");
    if (b->dim != D) return fail(BVH_AMD_ERR_ARG, "intersect_ray: dimension mismatch");
    if (const int rc = on_current_device(*b, "intersect_ray")) return rc;
    if (start == BVH_AMD_START_AT_ROOT) start = b->root_index;
    const T* r = static_cast<const T*>(ray);
    T ray8[8];
    if (D == 3) { for (int k = 0; k < 8; ++k) ray8[k] = r[k]; }
    else { ray8[0] = r[0]; ray8[1] = r[1]; ray8[2] = T(0); ray8[3] = r[2]; ray8[4] = r[3]; ray8[5] = T(0); ray8[6] = r[4]; ray8[7] = r[5]; }
    return trace_ray_callbacks<T>(*b, ray8, static_cast<uint32_t>(start), (flags & BVH_AMD_RAY_ANY_HIT) != 0, (flags & BVH_AMD_RAY_ROBUST) != 0,
                                  leaf_fn, inner_fn, user);
}

// The reference's bvhXX_build never returns NULL and its callers do not check (test/c_api_example.c:114-120): say why before they trip.
template <typename P> P* loud(P* result, const char* what) {
    if (!result) std::fprintf(stderr, "bvh_amd: %s failed: %s\n", what, g_error.c_str());
    return result;
}

// bvhXX_optimize / bvhXX_refit return void in the reference and cannot fail there; here a HIP error or a search-stack overflow would
// leave the tree un-optimised, un-refitted or half updated with nobody the wiser: say why and stop (callers that want to handle
// the failure use the int-returning bvhXX_optimize_config / bvhXX_refit_status).
inline void loud_or_abort(int rc, const char* what) {
    if (rc != BVH_AMD_OK) {
        std::fprintf(stderr, "bvh_amd: %s failed: %s\n", what, g_error.c_str());
        std::abort();
    }
}

// The reference's functions return void and cannot fail; a failure here would otherwise read as "no intersection".
template <typename T, int D, typename Callback>
void intersect_ray_legacy(const BvhImpl<T>* b, const void* ray, const Callback* callback, unsigned flags) {
    int rc = callback && callback->user_fn && b
                 ? intersect_ray_visit<T, D>(b, ray, b->root_index, flags, callback->user_fn, nullptr, callback->user_data)
                 : fail(BVH_AMD_ERR_ARG, "intersect_ray: null bvh or callback");
    if (rc != BVH_AMD_OK) {
        std::fprintf(stderr, "bvh_amd: bvh_intersect_ray failed: %s\n", g_error.c_str());
        std::abort();
    }
}

} // namespace

template <typename T> int nodes_resident(BvhImpl<T>& b) { return make_nodes_resident<T>(b); }
template int nodes_resident<float>(BvhImpl<float>&);
template int nodes_resident<double>(BvhImpl<double>&);

} // namespace bvh_amd

using namespace bvh_amd;

extern "C" {

const char* bvh_amd_last_error(void) { return g_error.c_str(); }
const char* bvh_amd_version(void) { return "bvh_amd 0.1 (gfx950)"; }
const char* bvh_amd_last_kernel_name(void) { return last_kernel_name(); }
int bvh_amd_last_launch_reordered(void) { return last_launch_reordered() ? 1 : 0; }
int bvh_amd_last_query_launches(void) { return last_query_launches(); }
void bvh_amd_kernel_timing(int on) { kernel_timing(on != 0); }
int bvh_amd_kernel_times(float* ms_out, size_t capacity, size_t* count_out) {
    if (!ms_out && capacity) return fail(BVH_AMD_ERR_ARG, "bvh_amd_kernel_times: null output");
    return kernel_times(ms_out, capacity, count_out);
}
void bvh_amd_last_optimize_profile(struct bvh_amd_optimize_profile* out) { if (out) last_optimize_profile(out); }
int bvh_amd_experiment(const char* name, int value) { return set_experiment(name, value); }
int bvh_amd_wave_times(unsigned long long* out, size_t capacity_waves, size_t* n_waves) { return wave_times(out, capacity_waves, n_waves); }
void bvh_amd_tuning(int refill_threshold, int leaf_threshold, int coop_fetch, int ticket_ranges) { set_tuning(refill_threshold, leaf_threshold, coop_fetch, ticket_ranges); }
void bvh_amd_last_launch_plan(int out[4]) { if (out) last_launch_plan(out); }
void bvh_amd_last_plan_search(float ns_per_ray[5], int measurements[5], unsigned* dropped_mask) { last_plan_search(ns_per_ray, measurements, dropped_mask); }
int bvh_amd_reorder_times(float* ms_out, size_t capacity, size_t* count_out) {
    if (!ms_out && capacity) return fail(BVH_AMD_ERR_ARG, "bvh_amd_reorder_times: null output");
    return reorder_times(ms_out, capacity, count_out);
}
void bvh_amd_reinsertion_stats(unsigned out[2]) { if (out) reinsertion_stats(out); }

// Scratch blocks of finished builds stay cached in the current device's stream-ordered pool (common.h: scratch_alloc); this hands
// them back to the driver (waits for the device first).
int bvh_amd_release_cached_memory(void) {
    int dev = 0;
    BVH_HIP_TRY(hipGetDevice(&dev), BVH_AMD_ERR_HIP);
    (void)bvh_amd_comm_cache_clear();                         // the communicators bvhXX_replicate keeps (replicate.hip)
    scratch_cache_flush();
    BVH_HIP_TRY(hipDeviceSynchronize(), BVH_AMD_ERR_HIP);
    hipMemPool_t pool = nullptr;
    if (hipDeviceGetDefaultMemPool(&pool, dev) != hipSuccess) { (void)hipGetLastError(); return BVH_AMD_OK; }
    BVH_HIP_TRY(hipMemPoolTrimTo(pool, 0), BVH_AMD_ERR_HIP);
    BVH_HIP_TRY(hipDeviceSynchronize(), BVH_AMD_ERR_HIP);     // (nothing of the library's is queued between the unmapping and its next allocation)
    return BVH_AMD_OK;
}

size_t bvh_amd_cached_scratch_bytes(void) { return scratch_cache_bytes(); }
size_t bvh_amd_scratch_cache_limit(void) { return scratch_cache_limit(); }

int bvh_amd_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return fail(BVH_AMD_ERR_HIP, hipGetErrorString(e));
    return n;
}

int bvh_amd_device_name(int device, char* out, size_t cap) {
    hipDeviceProp_t p;
    BVH_HIP_TRY(hipGetDeviceProperties(&p, device), BVH_AMD_ERR_HIP);
    snprintf(out, cap, "%s (%s)", p.name, p.gcnArchName);
    return BVH_AMD_OK;
}

void* bvh_amd_device_alloc(size_t bytes) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
    if (e != hipSuccess) { set_error(std::string("device_alloc: ") + hipGetErrorString(e)); return nullptr; }
    return p;
}
void bvh_amd_device_free(void* p) { if (p) (void)hipFree(p); }
int bvh_amd_copy_to_device(void* d, const void* h, size_t bytes) { BVH_HIP_TRY(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice), BVH_AMD_ERR_HIP); return BVH_AMD_OK; }
int bvh_amd_copy_to_host(void* h, const void* d, size_t bytes) { BVH_HIP_TRY(hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost), BVH_AMD_ERR_HIP); return BVH_AMD_OK; }
int bvh_amd_synchronize(void* stream) { BVH_HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)), BVH_AMD_ERR_HIP); return BVH_AMD_OK; }

bvh_thread_pool* bvh_thread_pool_create(size_t thread_count) {
    return reinterpret_cast<bvh_thread_pool*>(new ThreadPoolTag{thread_count});
}
void bvh_thread_pool_destroy(bvh_thread_pool* p) { delete reinterpret_cast<ThreadPoolTag*>(p); }

// What every family exports: forwarders only, the bodies are the templates above.
#define BVH_AMD_IMPL(T, D, S)                                                                                       \
    bvh##S* bvh##S##_build(bvh_thread_pool* pool, const bvh_bbox##S* bb, const bvh_vec##S* cc, size_t n,            \
                           const bvh_build_config* cfg) { return loud(build_host<T, D>(pool, bb, cc, n, cfg), "bvh" #S "_build"); } \
    bvh##S* bvh##S##_build_device(const T* d_bb, const T* d_cc, size_t n, const bvh_build_config* cfg,              \
                                  enum bvh_amd_builder builder, void* stream) {                                     \
        return build_device<T, D>(d_bb, d_cc, n, cfg, builder, stream); }                                           \
    bvh##S* bvh##S##_build_sah(bvh_thread_pool* pool, const bvh_bbox##S* bb, const bvh_vec##S* cc, size_t n,        \
                               const bvh_build_config* cfg, const bvh_amd_sah_config* sah) {                       \
        return with_sah(sah, [&] { return build_host<T, D>(pool, bb, cc, n, cfg); }); }                             \
    bvh##S* bvh##S##_build_device_sah(const T* d_bb, const T* d_cc, size_t n, const bvh_build_config* cfg,          \
                                      enum bvh_amd_builder builder, const bvh_amd_sah_config* sah, void* stream) {  \
        return with_sah(sah, [&] { return build_device<T, D>(d_bb, d_cc, n, cfg, builder, stream); }); }            \
    bvh##S* bvh##S##_build_device_binned(const T* d_bb, const T* d_cc, size_t n, const bvh_build_config* cfg,       \
                                         const bvh_amd_sah_config* sah, size_t bin_count, void* stream) {           \
        return with_bins(sah, bin_count, [&] { return build_device<T, D>(d_bb, d_cc, n, cfg, BVH_AMD_BUILDER_BINNED, stream); }); } \
    bvh##S* bvh##S##_extract(bvh##S* b, size_t root_id) { return handle<T, D>(extract<T>(impl<T, D>(b), root_id)); } \
    bvh##S* bvh##S##_from_nodes(const void* nodes, size_t nn, const size_t* ids, size_t np) {                       \
        return from_nodes<T, D>(nodes, nn, ids, np); }                                                              \
    void bvh##S##_destroy(bvh##S* b) { delete impl<T, D>(b); }                                                      \
    void bvh##S##_optimize(bvh_thread_pool*, bvh##S* b) { loud_or_abort(optimize<T>(impl<T, D>(b)), "bvh" #S "_optimize"); } \
    int bvh##S##_optimize_config(bvh##S* b, const bvh_amd_optimize_config* c) { return optimize_config<T>(impl<T, D>(b), c); } \
    void bvh##S##_refit(bvh##S* b) { loud_or_abort(refit<T>(impl<T, D>(b)), "bvh" #S "_refit"); }                  \
    int bvh##S##_refit_status(bvh##S* b) { return refit<T>(impl<T, D>(b)); }                                        \
    int bvh##S##_sync_device(bvh##S* b) { return sync_device<T>(impl<T, D>(b)); }                                    \
    int bvh##S##_refit_boxes(bvh##S* b, const T* d_bb, size_t n, void* s) {                                         \
        return refit_prims<T>(impl<T, D>(b), Family<T, D>::kRefitBoxes, d_bb, n, nullptr, s, "refit_boxes"); }       \
    void bvh##S##_append_node(bvh##S* b) { append_node<T, D>(impl<T, D>(b)); }                                      \
    void bvh##S##_remove_last_node(bvh##S* b) { remove_last_node<T, D>(impl<T, D>(b)); }                            \
    void bvh_node##S##_set_prim_count(bvh_node##S* n, size_t c) { set_prim_count<T, D>(n, c); }                     \
    void bvh_node##S##_set_first_id(bvh_node##S* n, size_t f) { set_first_id<T, D>(n, f); }                         \
    void bvh_node##S##_set_bbox(bvh_node##S* n, const bvh_bbox##S* bb) { set_bbox<T, D>(n, bb); }                   \
    void bvh##S##_save(const bvh##S* b, FILE* f) { if (b && f) save<T, D>(*impl<T, D>(b), f); }                     \
    bvh##S* bvh##S##_load(FILE* f) { return f ? load<T, D>(f) : nullptr; }                                          \
    size_t bvh##S##_serialize(const bvh##S* b, void* out, size_t cap) { return b ? serialize<T, D>(*impl<T, D>(b), out, cap) : 0; } \
    bvh##S* bvh##S##_deserialize(const void* bytes, size_t size) { return deserialize<T, D>(bytes, size); }         \
    size_t bvh##S##_serialize_device(bvh##S* b, void* d_out, size_t cap, void* stream) { return serialize_device<T>(impl<T, D>(b), d_out, cap, stream); } \
    bvh##S* bvh##S##_deserialize_device(const void* d_bytes, size_t size, void* stream) {                           \
        return handle<T, D>(deserialize_from_device<T>(d_bytes, size, D, static_cast<hipStream_t>(stream))); }      \
    bvh_node##S* bvh##S##_get_node(bvh##S* b, size_t i) { return get_node<T, D>(impl<T, D>(b), i); }                \
    size_t bvh##S##_get_prim_id(const bvh##S* b, size_t i) { return get_prim_id<T>(impl<T, D>(b), i); }             \
    size_t bvh##S##_get_prim_count(const bvh##S* b) { return impl<T, D>(b)->prim_count; }                           \
    size_t bvh##S##_get_node_count(const bvh##S* b) { return impl<T, D>(b)->node_count; }                           \
    bool bvh_node##S##_is_leaf(const bvh_node##S* n) { return is_leaf<T, D>(n); }                                   \
    size_t bvh_node##S##_get_prim_count(const bvh_node##S* n) { return get_prim_count<T, D>(n); }                   \
    size_t bvh_node##S##_get_first_id(const bvh_node##S* n) { return get_first_id<T, D>(n); }                       \
    bvh_bbox##S bvh_node##S##_get_bbox(const bvh_node##S* n) { return get_bbox<T, D>(n); }                          \
    void bvh##S##_copy_nodes(const bvh##S* b, void* out) { copy_nodes<T, D>(impl<T, D>(b), out); }                  \
    void bvh##S##_copy_prim_ids(const bvh##S* b, size_t* out) { copy_prim_ids<T>(impl<T, D>(b), out); }             \
    const uint32_t* bvh##S##_device_prim_ids(const bvh##S* b) { return impl<T, D>(b)->d_prim_ids; }                 \
    int bvh_amd_sphere_bounds##S(const T* sp, size_t n, T* bb, T* cc, void* s) {                                    \
        return Family<T, D>::sphere_bounds(sp, n, bb, cc, static_cast<hipStream_t>(s)); }                           \
    int bvh##S##_intersect_rays_sphere(const bvh##S* b, const T* prims, const bvh_ray##S* rays, size_t n, unsigned flags, \
                                       HitOf<T>::Type* hits, bvh_amd_counters* cnt, void* s) {                      \
        return intersect<T, D>(b, LEAF_SPHERE, prims, rays, n, flags, hits, cnt, s); }

// What only `3f` / `3d` export: triangles (tri.h), the mini-tree grid, the 3D area term, and the point queries.
#define BVH_AMD_IMPL_3D(T, S)                                                                                       \
    bvh##S* bvh##S##_build_minitree_device(const T* d_bb, const T* d_cc, size_t n, const bvh_amd_minitree_config* cfg, void* stream) { \
        return build_minitree<T>(d_bb, d_cc, n, cfg, stream); }                                                     \
    int bvh##S##_refit_tris(bvh##S* b, const T* d_tris9, size_t n, T* d_tris12_out, void* s) {                      \
        return refit_prims<T>(impl<T, 3>(b), REFIT_TRIS, d_tris9, n, d_tris12_out, s, "refit_tris"); }               \
    int bvh##S##_traversal_cost(bvh##S* b, double* cost_out, void* s) { return traversal_cost_checked<T>(impl<T, 3>(b), cost_out, s); } \
    int bvh##S##_prepare_trace(const bvh##S* b, size_t n_rays_hint, void* s) { return prepare_trace_checked<T>(impl<T, 3>(b), n_rays_hint, s); } \
    int bvh_amd_tri_bounds##S(const T* t, size_t n, T* bb, T* cc, void* s) {                                        \
        return launch_tri_bounds<T>(t, n, bb, cc, static_cast<hipStream_t>(s)); }                                   \
    int bvh_amd_precompute_tris##S(const T* t, const uint32_t* perm, size_t n, T* out, void* s) {                   \
        return launch_precompute_tris<T>(t, perm, n, out, static_cast<hipStream_t>(s)); }                           \
    int bvh##S##_intersect_rays_tri(const bvh##S* b, const T* prims, const bvh_ray##S* rays, size_t n, unsigned flags, \
                                    bvh_hit##S* hits, bvh_amd_counters* cnt, void* s) {                             \
        return intersect<T, 3>(b, LEAF_TRIANGLE, prims, rays, n, flags, hits, cnt, s); }                            \
    int bvh##S##_closest_points_tri(const bvh##S* b, const T* prims, const T* queries, size_t n, unsigned flags,       \
                                    bvh_hit##S* hits, bvh_amd_counters* cnt, void* s) {                             \
        return closest<T>(b, LEAF_TRIANGLE, prims, queries, n, flags, hits, cnt, s); }                              \
    int bvh##S##_closest_points_sphere(const bvh##S* b, const T* prims, const T* queries, size_t n, unsigned flags,    \
                                       bvh_hit##S* hits, bvh_amd_counters* cnt, void* s) {                          \
        return closest<T>(b, LEAF_SPHERE, prims, queries, n, flags, hits, cnt, s); }                                \
    int bvh##S##_radius_search_tri(const bvh##S* b, const T* prims, const T* queries, size_t n, unsigned flags, uint32_t* counts, \
                                   const uint64_t* offsets, uint32_t* list_prims, T* list_dist, bvh_amd_counters* cnt, void* s) { \
        return radius_search<T>(b, LEAF_TRIANGLE, prims, queries, n, flags, counts, offsets, list_prims, list_dist, cnt, s); } \
    int bvh##S##_radius_search_sphere(const bvh##S* b, const T* prims, const T* queries, size_t n, unsigned flags, uint32_t* counts, \
                                      const uint64_t* offsets, uint32_t* list_prims, T* list_dist, bvh_amd_counters* cnt, void* s) { \
        return radius_search<T>(b, LEAF_SPHERE, prims, queries, n, flags, counts, offsets, list_prims, list_dist, cnt, s); } \
    int bvh##S##_intersect_rays_all_tri(const bvh##S* b, const T* prims, const bvh_ray##S* rays, size_t n, unsigned flags, uint32_t* counts, \
                                        const uint64_t* offsets, bvh_hit##S* list_hits, bvh_amd_counters* cnt, void* s) {   \
        return ray_hits<T>(b, LEAF_TRIANGLE, prims, rays, n, flags, counts, offsets, list_hits, cnt, s); }          \
    int bvh##S##_intersect_rays_all_sphere(const bvh##S* b, const T* prims, const bvh_ray##S* rays, size_t n, unsigned flags, uint32_t* counts, \
                                           const uint64_t* offsets, bvh_hit##S* list_hits, bvh_amd_counters* cnt, void* s) { \
        return ray_hits<T>(b, LEAF_SPHERE, prims, rays, n, flags, counts, offsets, list_hits, cnt, s); }            \
    int bvh##S##_intersect_rays_nearest_tri(const bvh##S* b, const T* prims, const bvh_ray##S* rays, size_t n, unsigned k, unsigned flags, \
                                            bvh_hit##S* out_hits, uint32_t* counts, bvh_amd_counters* cnt, void* s) {       \
        return ray_nearest<T>(b, LEAF_TRIANGLE, prims, rays, n, k, flags, out_hits, counts, cnt, s); }              \
    int bvh##S##_intersect_rays_nearest_sphere(const bvh##S* b, const T* prims, const bvh_ray##S* rays, size_t n, unsigned k, unsigned flags, \
                                               bvh_hit##S* out_hits, uint32_t* counts, bvh_amd_counters* cnt, void* s) {    \
        return ray_nearest<T>(b, LEAF_SPHERE, prims, rays, n, k, flags, out_hits, counts, cnt, s); }                \
    int bvh##S##_sphere_cast_tri(const bvh##S* b, const T* prims, const bvh_ray##S* rays, size_t n, T radius, const T* radii, unsigned flags, \
                                 bvh_hit##S* hits, bvh_amd_counters* cnt, void* s) {                                \
        return sphere_cast<T>(b, LEAF_TRIANGLE, prims, rays, n, radius, radii, flags, hits, cnt, s); }              \
    int bvh##S##_sphere_cast_sphere(const bvh##S* b, const T* prims, const bvh_ray##S* rays, size_t n, T radius, const T* radii, unsigned flags, \
                                    bvh_hit##S* hits, bvh_amd_counters* cnt, void* s) {                             \
        return sphere_cast<T>(b, LEAF_SPHERE, prims, rays, n, radius, radii, flags, hits, cnt, s); }                \
    int bvh##S##_knn_tri(const bvh##S* b, const T* prims, const T* queries, size_t n, unsigned k, unsigned flags, uint32_t* out_prims, \
                         T* out_dist, uint32_t* counts, bvh_amd_counters* cnt, void* s) {                           \
        return knn<T>(b, LEAF_TRIANGLE, prims, queries, n, k, flags, out_prims, out_dist, counts, cnt, s); }        \
    int bvh##S##_knn_sphere(const bvh##S* b, const T* prims, const T* queries, size_t n, unsigned k, unsigned flags, uint32_t* out_prims, \
                            T* out_dist, uint32_t* counts, bvh_amd_counters* cnt, void* s) {                        \
        return knn<T>(b, LEAF_SPHERE, prims, queries, n, k, flags, out_prims, out_dist, counts, cnt, s); }                \
    int bvh##S##_winding_prepare(const bvh##S* b, const T* tris, T* moments, size_t moments_rows, void* s) {        \
        return winding_prepare<T>(b, tris, moments, moments_rows, s); }                                             \
    int bvh##S##_winding_numbers(const bvh##S* b, const T* tris, const T* moments, size_t moments_rows, const T* queries, size_t n, \
                                 double beta, unsigned flags, T* w, bvh_hit##S* hits, bvh_amd_counters* cnt, void* s) { \
        return winding_numbers<T>(b, tris, moments, moments_rows, queries, n, beta, flags, w, hits, cnt, s); }       \
    int bvh##S##_overlap_boxes(const bvh##S* b, const T* bboxes, size_t n_boxes, const T* queries6, size_t n, unsigned flags, uint32_t* counts, \
                               const uint64_t* offsets, uint32_t* list_prims, bvh_amd_counters* cnt, void* s) {          \
        return overlap<T>(b, false, bboxes, n_boxes, queries6, n, flags, counts, offsets, list_prims, cnt, s); }        \
    int bvh##S##_overlap_self(const bvh##S* b, const T* bboxes, size_t n_boxes, unsigned flags, uint32_t* counts,        \
                              const uint64_t* offsets, uint32_t* list_prims, bvh_amd_counters* cnt, void* s) {           \
        return overlap<T>(b, true, bboxes, n_boxes, nullptr, 0, flags, counts, offsets, list_prims, cnt, s); }                  \
    int bvh##S##_intersect_tris(const bvh##S* b, const T* tris9, size_t n_tris, const T* queries9, size_t n, unsigned flags, uint32_t* counts, \
                                const uint64_t* offsets, uint32_t* list_prims, bvh_amd_counters* cnt, void* s) {         \
        return intersect_tris<T>(b, false, tris9, n_tris, queries9, n, flags, counts, offsets, list_prims, cnt, s); }   \
    int bvh##S##_intersect_tris_self(const bvh##S* b, const T* tris9, size_t n_tris, unsigned flags, uint32_t* counts,   \
                                     const uint64_t* offsets, uint32_t* list_prims, bvh_amd_counters* cnt, void* s) {    \
        return intersect_tris<T>(b, true, tris9, n_tris, nullptr, 0, flags, counts, offsets, list_prims, cnt, s); }     \
    int bvh##S##_tri_distance(const bvh##S* b, const T* tris9, size_t n_tris, const T* queries9, size_t n, T max_distance,            \
                              const T* max_distances, unsigned flags, bvh_hit##S* hits, T* query_uv, bvh_amd_counters* cnt, void* s) { \
        return tri_distance<T>(b, tris9, n_tris, queries9, n, max_distance, max_distances, flags, hits, query_uv, cnt, s); }          \
    int bvh##S##_region_tris(const bvh##S* b, const T* tris9, size_t n_tris, const T* planes, size_t m, size_t n, unsigned flags,     \
                             uint32_t* counts, const uint64_t* offsets, uint32_t* list_prims, uint8_t* list_inside, bvh_amd_counters* cnt, void* s) { \
        return region<T>(b, LEAF_TRIANGLE, tris9, n_tris, planes, m, n, flags, counts, offsets, list_prims, list_inside, cnt, s); }   \
    int bvh##S##_region_spheres(const bvh##S* b, const T* sph4, size_t n_sph, const T* planes, size_t m, size_t n, unsigned flags,    \
                                uint32_t* counts, const uint64_t* offsets, uint32_t* list_prims, uint8_t* list_inside, bvh_amd_counters* cnt, void* s) { \
        return region<T>(b, LEAF_SPHERE, sph4, n_sph, planes, m, n, flags, counts, offsets, list_prims, list_inside, cnt, s); }       \
    int bvh##S##_instance_prepare(const bvh_amd_geometry##S* geoms, size_t n_geoms, const T* obj2world, const uint32_t* geometry,  \
                                  size_t n_instances, T* world2obj, T* bboxes, T* centers, void* s) {                    \
        return launch_instance_prepare<T>(geom_refs<T>(geoms), n_geoms, obj2world, geometry, n_instances, world2obj, bboxes, centers, \
                                          static_cast<hipStream_t>(s)); }                                                \
    int bvh##S##_intersect_rays_instanced(const bvh##S* top, const bvh_amd_geometry##S* geoms, size_t n_geoms, const T* world2obj, \
                                          const uint32_t* geometry, size_t n_instances, const bvh_ray##S* rays, size_t n_rays,     \
                                          unsigned flags, bvh_hit##S* hits, uint32_t* hit_instances, bvh_amd_counters* cnt, void* s) { \
        return intersect_instanced<T>(top, geoms, n_geoms, world2obj, geometry, n_instances, rays, n_rays, flags, hits, hit_instances, cnt, s); }

#define BVH_AMD_IMPL_RAY(T, D, S, CB, VIS)                                                                          \
    void bvh##S##_intersect_ray(const bvh##S* b, const bvh_ray##S* r, const CB* cb) { intersect_ray_legacy<T, D>(impl<T, D>(b), r, cb, 0u); } \
    void bvh##S##_intersect_ray_any(const bvh##S* b, const bvh_ray##S* r, const CB* cb) {                           \
        intersect_ray_legacy<T, D>(impl<T, D>(b), r, cb, BVH_AMD_RAY_ANY_HIT); }                                     \
    void bvh##S##_intersect_ray_robust(const bvh##S* b, const bvh_ray##S* r, const CB* cb) {                        \
        intersect_ray_legacy<T, D>(impl<T, D>(b), r, cb, BVH_AMD_RAY_ROBUST); }                                      \
    void bvh##S##_intersect_ray_any_robust(const bvh##S* b, const bvh_ray##S* r, const CB* cb) {                    \
        intersect_ray_legacy<T, D>(impl<T, D>(b), r, cb, BVH_AMD_RAY_ANY_HIT | BVH_AMD_RAY_ROBUST); }                \
    int bvh##S##_intersect_ray_visit(const bvh##S* b, const bvh_ray##S* r, size_t start, unsigned flags, const VIS* v) { \
        if (!v || !v->leaf_fn) return fail(BVH_AMD_ERR_ARG, "intersect_ray_visit: null visitor");                   \
        return intersect_ray_visit<T, D>(impl<T, D>(b), r, start, flags, v->leaf_fn, v->inner_fn, v->user_data); }

BVH_AMD_IMPL(float, 3, 3f)
BVH_AMD_IMPL(double, 3, 3d)
BVH_AMD_IMPL(float, 2, 2f)
BVH_AMD_IMPL(double, 2, 2d)
BVH_AMD_IMPL_3D(float, 3f)
BVH_AMD_IMPL_3D(double, 3d)
BVH_AMD_IMPL_RAY(float, 3, 3f, bvh_intersect_callbackf, bvh_amd_ray_visitorf)
BVH_AMD_IMPL_RAY(double, 3, 3d, bvh_intersect_callbackd, bvh_amd_ray_visitord)
BVH_AMD_IMPL_RAY(float, 2, 2f, bvh_intersect_callbackf, bvh_amd_ray_visitorf)
BVH_AMD_IMPL_RAY(double, 2, 2d, bvh_intersect_callbackd, bvh_amd_ray_visitord)

int bvh_amd_offsets_from_counts(const uint32_t* d_counts, size_t n, uint64_t* d_offsets, void* stream) {
    return offsets_from_counts(d_counts, n, d_offsets, static_cast<hipStream_t>(stream));
}
int bvh_amd_std_sort_ids3f(const float* d_keys, size_t n, uint32_t* d_ids_out, void* stream) {
    return std_sort_ids<float>(d_ids_out, d_keys, static_cast<uint32_t>(n), 1, 0, 1, static_cast<hipStream_t>(stream));
}
int bvh_amd_std_sort_ids3d(const double* d_keys, size_t n, uint32_t* d_ids_out, void* stream) {
    return std_sort_ids<double>(d_ids_out, d_keys, static_cast<uint32_t>(n), 1, 0, 1, static_cast<hipStream_t>(stream));
}
int bvh_amd_radix_sort_pairs_u32(uint32_t* d_keys, uint32_t* d_vals, size_t n, int bits, void* stream) {
    DeviceTemps<uint32_t> tmp;
    auto& [kt, vt] = tmp;
    BVH_HIP_TRY(hipMalloc(&kt, std::max<size_t>(n, 1) * 4), BVH_AMD_ERR_HIP);
    hipError_t e = hipMalloc(&vt, std::max<size_t>(n, 1) * 4);
    return e == hipSuccess ? radix_sort_pairs<uint32_t>(d_keys, d_vals, kt, vt, static_cast<uint32_t>(n), 1, bits, static_cast<hipStream_t>(stream))
                           : fail(BVH_AMD_ERR_HIP, hipGetErrorString(e));
}

int bvh_amd_radix_order_u32(const uint32_t* d_keys, size_t n, int bits, uint32_t* d_order_out, void* stream) {
    if (n >= (size_t{1} << 31)) return fail(BVH_AMD_ERR_ARG, "bvh_amd_radix_order_u32: fewer than 2^31 keys");
    return radix_order_of_keys(d_keys, static_cast<uint32_t>(n), bits, d_order_out, static_cast<hipStream_t>(stream));
}

int bvh_amd_pinhole_rays3f(const float eye[3], const float dir[3], const float up[3], size_t w, size_t h, bvh_ray3f* d_rays, void* stream) {
    return launch_pinhole_rays<float>(eye, dir, up, w, h, reinterpret_cast<float*>(d_rays), static_cast<hipStream_t>(stream));
}
int bvh_amd_pinhole_rays3d(const double eye[3], const double dir[3], const double up[3], size_t w, size_t h, bvh_ray3d* d_rays, void* stream) {
    return launch_pinhole_rays<double>(eye, dir, up, w, h, reinterpret_cast<double*>(d_rays), static_cast<hipStream_t>(stream));
}
int bvh_amd_shade_eyelight3f(const float* d_tris12, const bvh_ray3f* d_rays, const bvh_hit3f* d_hits, size_t n, uint8_t* d_rgb, void* stream) {
    return launch_shade_eyelight<float>(d_tris12, reinterpret_cast<const float*>(d_rays), d_hits, n, d_rgb, static_cast<hipStream_t>(stream));
}
int bvh_amd_shade_eyelight3d(const double* d_tris12, const bvh_ray3d* d_rays, const bvh_hit3d* d_hits, size_t n, uint8_t* d_rgb, void* stream) {
    return launch_shade_eyelight<double>(d_tris12, reinterpret_cast<const double*>(d_rays), d_hits, n, d_rgb, static_cast<hipStream_t>(stream));
}

int bvh_amd_gather(const void* d_in, const uint32_t* d_perm, size_t n, size_t stride, void* d_out, void* stream) {
    return launch_gather(d_in, d_perm, n, stride, d_out, static_cast<hipStream_t>(stream));
}

} // extern "C"
