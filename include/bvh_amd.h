/* bvh_amd — MI355X-native BVH construction and traversal behind madmann91/bvh's C bindings.
 *
 * This header is the C-ABI boundary of libbvh_amd.so. It has two parts:
 *
 *  (1) the reference's own C API (reference src/bvh/v2/c_api/bvh.h), re-declared here with the same
 *      names, argument meaning and ownership rules so that code written against libbvh_c.so links
 *      against libbvh_amd.so unchanged. Each declaration cites the reference line it replaces.
 *      `struct bvh3f` etc. stay opaque; ours additionally owns the device-resident copy.
 *
 *  (2) additive, callback-free batch entry points (`*_device`, `*_rays_*`). The reference's
 *      per-ray `bvhXX_intersect_ray(bvh, ray, callback)` (c_api/bvh.h:277-295) takes a host function
 *      pointer per leaf: it is served (the walk runs on the device, the leaves come back to the host
 *      callback in the reference's order), but it costs kernel launches per ray; the batch family is what
 *      a maintainer binds for the hot path (INTEGRATION.md shows the binding). Buffers named d_* are DEVICE pointers
 *      (HBM of the current HIP device); all others are host pointers. `stream` is a hipStream_t
 *      passed as void* (NULL = the default stream); batch calls are asynchronous on it.
 *
 * Error behaviour: the reference reports no errors at all. Functions here that
 * return int return 0 on success and a negative code on failure; pointer-returning functions return
 * NULL on failure; `bvh_amd_last_error()` gives the thread's last message. There is NO CPU fallback:
 * if no MI355X/HIP device is usable the calls fail.
 */
#ifndef BVH_AMD_H
#define BVH_AMD_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdbool.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BVH_AMD_API __attribute__((visibility("default")))

#define BVH_ROOT_INDEX 0                     /* c_api/bvh.h:32 */
#define BVH_INVALID_PRIM_ID SIZE_MAX         /* c_api/bvh.h:33 */

/* ---- types shared with the reference (c_api/bvh.h:35-83) ---------------------------------- */
struct bvh3f;
struct bvh3d;
struct bvh_node3f;
struct bvh_node3d;
struct bvh2f;                                   /* c_api/bvh.h:35-43: the 2D families (Node<T, 2>, 20/40-byte nodes) */
struct bvh2d;
struct bvh_node2f;
struct bvh_node2d;
struct bvh_thread_pool;

enum bvh_build_quality { BVH_BUILD_QUALITY_LOW, BVH_BUILD_QUALITY_MEDIUM, BVH_BUILD_QUALITY_HIGH };

struct bvh_build_config {                    /* c_api/bvh.h:53-58 */
    enum bvh_build_quality quality;
    size_t min_leaf_size;
    size_t max_leaf_size;
    size_t parallel_threshold;
};

struct bvh_vec2f { float x, y; };
struct bvh_vec2d { double x, y; };
struct bvh_bbox2f { struct bvh_vec2f min, max; };
struct bvh_bbox2d { struct bvh_vec2d min, max; };
struct bvh_ray2f { struct bvh_vec2f org, dir; float tmin, tmax; };
struct bvh_ray2d { struct bvh_vec2d org, dir; double tmin, tmax; };
struct bvh_vec3f { float x, y, z; };
struct bvh_vec3d { double x, y, z; };
struct bvh_bbox3f { struct bvh_vec3f min, max; };
struct bvh_bbox3d { struct bvh_vec3d min, max; };
struct bvh_ray3f { struct bvh_vec3f org, dir; float tmin, tmax; };
struct bvh_ray3d { struct bvh_vec3d org, dir; double tmin, tmax; };

/* c_api/bvh.h:75-83: leaf callback of the per-ray entry points. user_fn(user_data, &tmax, begin, end) intersects the
 * primitives [begin, end) (BVH order), returns true on a hit and may shorten the ray through the pointer. */
struct bvh_intersect_callbackf {
    void* user_data;
    bool (*user_fn)(void*, float*, size_t begin, size_t end);
};
struct bvh_intersect_callbackd {
    void* user_data;
    bool (*user_fn)(void*, double*, size_t begin, size_t end);
};

/* Additive: the same with the reference's optional InnerFn (bvh.h:72-73): inner_fn(user_data, first_child_id) is called for
 * every visited pair of siblings (nodes first_child_id and first_child_id + 1) before its boxes are tested; may be NULL. */
struct bvh_amd_ray_visitorf {
    void* user_data;
    bool (*leaf_fn)(void*, float*, size_t begin, size_t end);
    void (*inner_fn)(void*, size_t first_child_id);
};
struct bvh_amd_ray_visitord {
    void* user_data;
    bool (*leaf_fn)(void*, double*, size_t begin, size_t end);
    void (*inner_fn)(void*, size_t first_child_id);
};

/* ---- additive types --------------------------------------------------------------------------- */

/* One record per ray. prim = BVH-order primitive index (the `i` the reference's leaf callback
 * receives, bvh.h:152; original id = bvhXX_get_prim_id(bvh, prim)), or BVH_AMD_INVALID on a miss, in
 * which case t = the ray's input tmax. Triangles: (t,u,v) of PrecomputedTri::intersect (tri.h:56-74).
 * Spheres: t = t0, u = t1 of Sphere::intersect (sphere.h:32-49), v = 0. */
#define BVH_AMD_INVALID 0xFFFFFFFFu
struct bvh_hit3f { uint32_t prim; float t, u, v; };
struct bvh_hit3d { uint32_t prim; uint32_t pad; double t, u, v; };

/* Traversal statistics (the reference's optional InnerFn/leaf counters, test/benchmark.cpp:258-296).
 * Sums over the batch: inner-node pair visits, primitive tests, leaf visits. */
struct bvh_amd_counters { unsigned long long node_pairs, prim_tests, leaves; };

enum bvh_amd_ray_flags {
    BVH_AMD_RAY_ANY_HIT = 1u,  /* Bvh::intersect<IsAnyHit = true>: no near/far reordering, stop at first hit */
    BVH_AMD_RAY_ROBUST  = 2u,  /* Bvh::intersect<IsRobust = true>: Ize's robust slab test (node.h:68-77)      */
    BVH_AMD_RAY_SORTED  = 4u,  /* always reorder the batch internally for coherence (a 24-bit origin-cell / direction-octant key,
                                  three radix passes, ~0.45 ms per 16M rays); per-ray results are unchanged. With neither this
                                  flag nor BVH_AMD_RAY_UNSORTED the library decides: it reorders batches of >= 1M rays on trees
                                  whose node records exceed the 32 MB of L2 and through which a random line is expected to fetch
                                  >= 100 records (sum of area(node) / area(root) over the inner nodes): +40..50 % there      */
    BVH_AMD_RAY_UNSORTED = 16u, /* never reorder (rays already coherent, or no scratch memory to spare: 16 bytes per ray)  */
                                /* (SORTED / UNSORTED / ORIGINAL_IDS apply to bvhXX_closest_points_* and bvhXX_radius_search_* queries too) */
    BVH_AMD_RAY_ORIGINAL_IDS = 8u, /* hit.prim = the ORIGINAL primitive id bvh.prim_ids[i] (what c_api_example.c:265-268 looks up per
                                      hit) instead of the BVH-order index i: one more pass over the hit records, on the device    */
    BVH_AMD_TRI_SKIP_SHARED = 32u, /* bvh3X_intersect_tris / bvh3X_intersect_tris_self only (every other entry point refuses it): a
                                      pair of triangles with a common vertex is not listed                                       */
    BVH_AMD_REGION_EXACT = 64u     /* bvh3X_region_tris only (every other entry point refuses it): list a triangle iff it shares a
                                      point with the region, not merely iff no single plane rejects it                          */
};

/* Which reference builder a device build reproduces (bit-exact node/prim order). */
enum bvh_amd_builder {
    BVH_AMD_BUILDER_DEFAULT_SERIAL   = 0, /* DefaultBuilder::build(bboxes, centers, cfg), default_builder.h:49  */
    BVH_AMD_BUILDER_DEFAULT_PARALLEL = 1, /* DefaultBuilder::build(pool, ...), default_builder.h:33             */
    BVH_AMD_BUILDER_BINNED           = 2, /* BinnedSahBuilder::build, binned_sah_builder.h:32                   */
    BVH_AMD_BUILDER_SWEEP            = 3  /* SweepSahBuilder::build, sweep_sah_builder.h:30                     */
};

/* ---- library / device ------------------------------------------------------------------------- */
BVH_AMD_API const char* bvh_amd_last_error(void);
BVH_AMD_API const char* bvh_amd_version(void);
BVH_AMD_API int bvh_amd_device_count(void);            /* < 0 on HIP failure */
BVH_AMD_API int bvh_amd_device_name(int device, char* out, size_t cap);

/* Device memory helpers (thin wrappers over hipMalloc / hipMemcpy) so that C and C++ callers need no HIP headers. */
BVH_AMD_API void* bvh_amd_device_alloc(size_t bytes);                         /* NULL on failure */
BVH_AMD_API void bvh_amd_device_free(void* d_ptr);
BVH_AMD_API int bvh_amd_copy_to_device(void* d_dst, const void* h_src, size_t bytes);
BVH_AMD_API int bvh_amd_copy_to_host(void* h_dst, const void* d_src, size_t bytes);
BVH_AMD_API int bvh_amd_synchronize(void* stream);
/* Builds, optimize, the sorts and reordered ray batches take their scratch from the device's stream-ordered memory pool — always
 * through a stream the LIBRARY owns, never the caller's — and keep freed blocks in a small cache for the next call, each with an
 * event that marks the end of the call that freed it. Consequences a caller can rely on (round 5; c_api/bvh.h:129-132 has no
 * lifetime rule beyond _destroy, and neither has this library): a `stream` argument is only used during the call it is passed to;
 * it may be destroyed afterwards, whatever was built or cached while it lived (tests/c/stream_lifetime.c).
 * The cache holds at most BVH_AMD_CACHE_MB megabytes per device (default: min(1024, 5 % of the HBM free at first use); 0 = no
 * cache). Scratch the cache does not keep goes back to the device's default memory pool and STAYS MAPPED there for the next
 * request: the pool's release threshold is set to "never on its own", because memory that the pool unmaps at some synchronisation
 * and maps again right afterwards was read stale by compute kernels on this platform (profiles/r05_pool_trim_stale_reads.txt). So
 * a process keeps reserved what its largest call needed (a 10M-triangle build cycles ~3 GB of scratch) until it calls
 * bvh_amd_release_cached_memory(), which returns cache and pool to the driver with the device idle before and after.
 * BVH_AMD_POOL=0 disables pool and cache (plain hipMalloc / hipFree).
 *
 * Environment variables a release library reads — all of them: BVH_AMD_CACHE_MB, BVH_AMD_POOL (above); BVH_AMD_CALIBRATE=0 (no
 * measured launch-plan search, the predictor's plan always); BVH_AMD_REINSERT=exact (ReinsertionOptimizer: replay the reference's
 * candidate heap in every iteration instead of only where the heap-free path cannot prove the same result); BVH_AMD_RCCL_LIB (path of librccl for the multi-GPU
 * entry points; else the loader's search path, $ROCM_PATH/lib, /opt/rocm/lib). A/B switches, profiling aids and fault injection
 * exist only in the developer build (python -m bvh_amd.build --developer -> libbvh_amd_dev.so, -DBVH_AMD_DEVELOPER).          */
BVH_AMD_API int bvh_amd_release_cached_memory(void);
BVH_AMD_API size_t bvh_amd_cached_scratch_bytes(void);     /* bytes the block cache holds on the current device right now */
BVH_AMD_API size_t bvh_amd_scratch_cache_limit(void);      /* its bound on the current device */
/* Measurement aid for bench.py (csrc/probe.hip): mean launch time of a dependent walk over a table of 64-byte records (word 0 of
 * a record = index of the next one), one record in flight per lane — the rate the memory system gives the traversal's access
 * pattern when nothing else is in the way. Not used by any product path. */
BVH_AMD_API int bvh_amd_probe_record_walk(const void* d_table, uint32_t n_records, uint32_t steps, int blocks_per_cu, int reps,
                                          float* ms_out, unsigned long long* records_out, void* stream);
/* The same walk with the way a record reaches its lane selectable (csrc/probe.hip): mode 0 per-lane loads (as above), 1 quad-
 * cooperative loads + LDS transpose, 2 / 3 one chain per quad loaded by the quad / by its first lane; `active` = lanes of a wave
 * that own a chain (1..64); 4 quad-cooperative loads + in-register transpose (the shipped fetch); 5 / 6 records of 128 bytes, one chain per
 * octet of lanes loaded by the octet / by its first lane (n_records then counts 128-byte records). A table of a few KB measures the L1,
 * a few MB the L2, beyond 32 MB the fabric side. */
/* One chain per lane that alternates between a small (L2-resident) and a big (beyond the L2s) table, one fetch in flight per lane:
 * do the times of the two levels add (one shared resource: the CU's outstanding lines) or overlap? (csrc/probe.hip) */
BVH_AMD_API int bvh_amd_probe_mixed_walk(const void* d_small, uint32_t n_small, const void* d_big, uint32_t n_big, uint32_t steps, int blocks_per_cu, int reps,
                                         int coop, float* ms_out, unsigned long long* records_out, void* stream);
BVH_AMD_API int bvh_amd_probe_record_walk_ex(const void* d_table, uint32_t n_records, uint32_t steps, int blocks_per_cu, int reps, int mode, int active,
                                             float* ms_out, unsigned long long* records_out, void* stream);

/* ---- multi-GPU (the "required extension" of 8b: device select + replicate) ------------------------------------
 * Ray batches shard embarrassingly (a const Bvh + per-ray state, reference bvh.h:160-182 touches nothing shared); the ONE
 * exchange of the path is a root-to-all broadcast of the scene over RCCL / xGMI: the Bvh::serialize byte stream (reference
 * bvh.h:221-229) written into HBM straight from the resident nodes, and the BVH-ordered primitive array. It runs inside this
 * library (csrc/replicate.hip; librccl is opened on first use); no payload byte visits the host on any rank. A BVH is bound to the device
 * it was built / received on; bvhXX_intersect_rays_* must be called with that device current (bvh_amd_device_select).
 *   one process per GPU: rank 0 calls bvh_amd_comm_unique_id, the 128 bytes travel by any side channel (a file, MPI, torch's
 *     store), every rank calls bvh_amd_comm_create on ITS device, then bvhXX_broadcast; or wrap an ncclComm_t you already have
 *     with bvh_amd_comm_adopt;
 *   one process, N GPUs (what a C caller of the reference API would do): bvhXX_replicate.                                        */
#define BVH_AMD_COMM_ID_BYTES 128
struct bvh_amd_comm;                                   /* an RCCL communicator + its rank / size / device */
BVH_AMD_API int bvh_amd_device_select(int device);     /* hipSetDevice for the calling thread: following builds / uploads live there */
BVH_AMD_API int bvh_amd_device_current(void);          /* < 0 on HIP failure */
BVH_AMD_API int bvh_amd_comm_unique_id(void* id_out /* BVH_AMD_COMM_ID_BYTES */);                   /* ncclGetUniqueId */
BVH_AMD_API struct bvh_amd_comm* bvh_amd_comm_create(const void* id, int n_ranks, int rank);        /* ncclCommInitRank on the current device; NULL on failure */
BVH_AMD_API struct bvh_amd_comm* bvh_amd_comm_adopt(void* nccl_comm /* ncclComm_t, stays yours */);
BVH_AMD_API void bvh_amd_comm_destroy(struct bvh_amd_comm*);
BVH_AMD_API int bvh_amd_comm_rank(const struct bvh_amd_comm*);
BVH_AMD_API int bvh_amd_comm_size(const struct bvh_amd_comm*);
BVH_AMD_API void* bvh_amd_comm_handle(const struct bvh_amd_comm*);                                  /* the ncclComm_t */
/* ncclBroadcast of a raw device buffer, in place, on `stream` (e.g. the scene box the ray generators need) */
BVH_AMD_API int bvh_amd_comm_broadcast(struct bvh_amd_comm*, void* d_buf, size_t bytes, int root, void* stream);
/* bvhXX_replicate keeps its communicators (one set per list of devices: ncclCommInitAll is paid once, not per scene); this destroys
 * them (also done by bvh_amd_release_cached_memory) and returns the number of sets there were.                                   */
BVH_AMD_API int bvh_amd_comm_cache_clear(void);
/* The path librccl was opened from ("" until the first multi-GPU call, or when it could not be opened: bvh_amd_last_error). RCCL is
 * loaded on first use of the entry points of this section — a single-GPU program never needs it to be installed.                 */
BVH_AMD_API const char* bvh_amd_rccl_library(void);
/* Collective: EVERY rank of the communicator calls it. The root passes its BVH and the BVH-ordered primitive array
 * (prim_bytes bytes of device memory); the others pass NULL / NULL / 0. Returns this rank's device-resident BVH — the root's own
 * object on the root, a new one elsewhere (bvhXX_destroy) — and in *d_prims_out this rank's primitive array (the root's own
 * pointer on the root, otherwise a new buffer to release with bvh_amd_device_free); *prim_bytes_out (may be NULL) its size.
 * NULL on failure (bvh_amd_last_error). No rank is left waiting by a peer's failure: a root that has nothing valid to send says so
 * in the header, and after the header every rank prepares its side (family check, receive buffers, the root's serialization) and
 * the ranks agree on one status word (ncclAllReduce, min) BEFORE any payload is posted — if any rank failed, all return NULL. When it returns, the BVH is ready on `stream`'s device and the buffers may be used from any stream.                 */
BVH_AMD_API struct bvh3f* bvh3f_broadcast(struct bvh_amd_comm*, int root, struct bvh3f* bvh, const void* d_prims, size_t prim_bytes,
                                          void** d_prims_out, size_t* prim_bytes_out, void* stream);
BVH_AMD_API struct bvh3d* bvh3d_broadcast(struct bvh_amd_comm*, int root, struct bvh3d* bvh, const void* d_prims, size_t prim_bytes,
                                          void** d_prims_out, size_t* prim_bytes_out, void* stream);
/* One process, several GPUs: copies the scene from the BVH's own device to every other device of `devices` (NULL: 0 ..
 * n_devices - 1; the BVH's device must be among them) with ncclCommInitAll + one grouped ncclBroadcast. bvhs_out[i] /
 * d_prims_out[i] belong to devices[i]; the entry of the BVH's own device holds the original pointers, the others are new
 * (bvhXX_destroy / bvh_amd_device_free with that device current). The calling thread's current device is left unchanged.      */
BVH_AMD_API int bvh3f_replicate(struct bvh3f* bvh, const void* d_prims, size_t prim_bytes, int n_devices, const int* devices,
                                struct bvh3f** bvhs_out, void** d_prims_out);
BVH_AMD_API int bvh3d_replicate(struct bvh3d* bvh, const void* d_prims, size_t prim_bytes, int n_devices, const int* devices,
                                struct bvh3d** bvhs_out, void** d_prims_out);

/* ---- thread pool (c_api/bvh.h:90-91). Kept for signature compatibility; the GPU grid replaces it.
 * A non-NULL pool selects the reference's *parallel* builder semantics (mini-trees). ------------- */
BVH_AMD_API struct bvh_thread_pool* bvh_thread_pool_create(size_t thread_count);
BVH_AMD_API void bvh_thread_pool_destroy(struct bvh_thread_pool*);

/* ---- construction ------------------------------------------------------------------------------ */
/* c_api/bvh.h:106-118. Host arrays in; the build runs on the current HIP device; the returned object
 * holds the reference-layout host mirror (for the accessors below) and the device-resident copy. */
BVH_AMD_API struct bvh3f* bvh3f_build(struct bvh_thread_pool*, const struct bvh_bbox3f* bboxes,
    const struct bvh_vec3f* centers, size_t prim_count, const struct bvh_build_config* config);
BVH_AMD_API struct bvh3d* bvh3d_build(struct bvh_thread_pool*, const struct bvh_bbox3d* bboxes,
    const struct bvh_vec3d* centers, size_t prim_count, const struct bvh_build_config* config);

/* Additive: inputs already resident in HBM (n x {min,max} and n x center, tightly packed). */
BVH_AMD_API struct bvh3f* bvh3f_build_device(const float* d_bboxes, const float* d_centers, size_t prim_count,
    const struct bvh_build_config* config, enum bvh_amd_builder builder, void* stream);
BVH_AMD_API struct bvh3d* bvh3d_build_device(const double* d_bboxes, const double* d_centers, size_t prim_count,
    const struct bvh_build_config* config, enum bvh_amd_builder builder, void* stream);

/* Additive: TopDownSahBuilder::Config::sah, the SplitHeuristic every builder's Config carries (src/bvh/v2/split_heuristic.h:17-38,
 * top_down_sah_builder.h:27-30) and the reference's C struct bvh_build_config has no field for: a range of `size` primitives
 * costs ceil(size / 2^log_cluster_size) primitive intersections, and a node that is not split saves `cost_ratio` (ratio of the
 * cost of a ray-box test over a ray-primitive test). NULL = the reference's defaults {0, 1}. bvhXX_build_sah is bvhXX_build
 * (DefaultBuilder, pool or not) with it; bvhXX_build_device_sah is bvhXX_build_device with it. */
struct bvh_amd_sah_config {
    size_t log_cluster_size;                   /* default 0 */
    double cost_ratio;                         /* default 1 */
};
BVH_AMD_API struct bvh3f* bvh3f_build_sah(struct bvh_thread_pool*, const struct bvh_bbox3f* bboxes, const struct bvh_vec3f* centers,
    size_t prim_count, const struct bvh_build_config* config, const struct bvh_amd_sah_config* sah);
BVH_AMD_API struct bvh3d* bvh3d_build_sah(struct bvh_thread_pool*, const struct bvh_bbox3d* bboxes, const struct bvh_vec3d* centers,
    size_t prim_count, const struct bvh_build_config* config, const struct bvh_amd_sah_config* sah);
BVH_AMD_API struct bvh3f* bvh3f_build_device_sah(const float* d_bboxes, const float* d_centers, size_t prim_count,
    const struct bvh_build_config* config, enum bvh_amd_builder builder, const struct bvh_amd_sah_config* sah, void* stream);
BVH_AMD_API struct bvh3d* bvh3d_build_device_sah(const double* d_bboxes, const double* d_centers, size_t prim_count,
    const struct bvh_build_config* config, enum bvh_amd_builder builder, const struct bvh_amd_sah_config* sah, void* stream);

/* Additive: BinnedSahBuilder<Node, BinCount>::build (src/bvh/v2/binned_sah_builder.h:18, :32-38) with its BinCount template argument
 * as a run-time value: 4, 8 (the reference's default, = bvhXX_build_device_sah with BVH_AMD_BUILDER_BINNED), 16 or 32 bins per axis.
 * Same inputs as bvhXX_build_device_sah; NULL for anything else (bvh_amd_last_error). DefaultBuilder and MiniTreeBuilder always
 * instantiate the default (default_builder.h:52, mini_tree_builder.h:129), so only a direct user of BinnedSahBuilder has this knob. */
BVH_AMD_API struct bvh3f* bvh3f_build_device_binned(const float* d_bboxes, const float* d_centers, size_t prim_count,
    const struct bvh_build_config* config, const struct bvh_amd_sah_config* sah, size_t bin_count, void* stream);
BVH_AMD_API struct bvh3d* bvh3d_build_device_binned(const double* d_bboxes, const double* d_centers, size_t prim_count,
    const struct bvh_build_config* config, const struct bvh_amd_sah_config* sah, size_t bin_count, void* stream);

/* Additive: MiniTreeBuilder::build(pool, bboxes, centers, config) itself (src/bvh/v2/mini_tree_builder.h:29-58) with its own
 * configuration; DefaultBuilder(pool)'s three qualities are three settings of it (default_builder.h:65-73). log2_grid_dim
 * may be 1..10 (three coordinates in the reference's 32-bit Morton code, mini_tree_builder.h:169); the cell histogram takes
 * 8^log2_grid_dim x 8 bytes of HBM. */
struct bvh_amd_minitree_config {
    size_t min_leaf_size, max_leaf_size;       /* TopDownSahBuilder::Config (top_down_sah_builder.h:27-40), defaults 1 / 8 */
    int enable_pruning;                        /* default 1 */
    double pruning_area_ratio;                 /* default 0.01 */
    size_t parallel_threshold;                 /* default 1024 */
    size_t log2_grid_dim;                      /* default 4 */
    size_t log_cluster_size;                   /* SplitHeuristic (split_heuristic.h:17-23), defaults 0 ... */
    double cost_ratio;                         /* ... and 1 */
};
BVH_AMD_API struct bvh3f* bvh3f_build_minitree_device(const float* d_bboxes, const float* d_centers, size_t prim_count,
    const struct bvh_amd_minitree_config* config, void* stream);
BVH_AMD_API struct bvh3d* bvh3d_build_minitree_device(const double* d_bboxes, const double* d_centers, size_t prim_count,
    const struct bvh_amd_minitree_config* config, void* stream);

/* Additive: wrap an existing reference-layout BVH (28/56-byte nodes, node.h:31-37) and upload it. */
BVH_AMD_API struct bvh3f* bvh3f_from_nodes(const void* nodes, size_t node_count, const size_t* prim_ids, size_t prim_count);
BVH_AMD_API struct bvh3d* bvh3d_from_nodes(const void* nodes, size_t node_count, const size_t* prim_ids, size_t prim_count);

/* Additive: Bvh::extract_bvh(root_id) (src/bvh/v2/bvh.h:92-122) on the device: the subtree under `root_id` as its own BVH,
 * node order and re-packed prim ids exactly as the reference lays them out. NULL + bvh_amd_last_error() on failure. */
BVH_AMD_API struct bvh3f* bvh3f_extract(struct bvh3f* bvh, size_t root_id);
BVH_AMD_API struct bvh3d* bvh3d_extract(struct bvh3d* bvh, size_t root_id);

BVH_AMD_API void bvh3f_destroy(struct bvh3f*);                                   /* c_api/bvh.h:130 */
BVH_AMD_API void bvh3d_destroy(struct bvh3d*);                                   /* c_api/bvh.h:132 */

/* ---- optimization (c_api/bvh.h:226-229): ReinsertionOptimizer::optimize on the device, in place. The pool
 * argument is accepted for signature compatibility (the result does not depend on it in the reference either).
 * On failure the BVH is left unchanged and bvh_amd_last_error() is set. */
BVH_AMD_API void bvh3f_optimize(struct bvh_thread_pool*, struct bvh3f*);
BVH_AMD_API void bvh3d_optimize(struct bvh_thread_pool*, struct bvh3d*);
/* Additive: ReinsertionOptimizer::Config (src/bvh/v2/reinsertion_optimizer.h:18-24), which the reference's C API does not
 * expose; NULL = its defaults {0.05, 3}. Returns an error code (the void functions above only set bvh_amd_last_error). */
struct bvh_amd_optimize_config {
    double batch_size_ratio;                   /* fraction of the nodes re-inserted per iteration, default 0.05 */
    size_t max_iter_count;                     /* default 3 */
};
BVH_AMD_API int bvh3f_optimize_config(struct bvh3f*, const struct bvh_amd_optimize_config*);
BVH_AMD_API int bvh3d_optimize_config(struct bvh3d*, const struct bvh_amd_optimize_config*);

/* ---- refit and node editing (c_api/bvh.h:170-229). The setters, append and remove act on the host mirror exactly
 * like the reference (node pointers alias the mirror and are invalidated by append). `bvhXX_refit` pushes the mirror
 * to the device, recomputes every inner box bottom-up there (Bvh::refit, bvh.h:211-218) and refreshes both copies.
 * After editing WITHOUT refit/optimize, call bvhXX_sync_device before tracing (additive; 0 on success). */
BVH_AMD_API void bvh3f_refit(struct bvh3f*);
BVH_AMD_API void bvh3d_refit(struct bvh3d*);
/* The void functions above (c_api/bvh.h:218-229) cannot report a failure: on one (HIP error, reinsertion search-stack overflow)
 * they print the reason and abort rather than leave a half-updated tree behind. Callers that want to handle it use
 * bvhXX_optimize_config (NULL config = the reference's defaults) and bvhXX_refit_status: 0 or a negative code + bvh_amd_last_error(). */
BVH_AMD_API int bvh3f_refit_status(struct bvh3f*);
BVH_AMD_API int bvh3d_refit_status(struct bvh3d*);

/* ---- refit from moved primitives, entirely on the device (additive) ------------------------------------------------------
 * The resident form of the reference's Bvh::refit(leaf_fn) (bvh.h:211-218): moved primitives in HBM in, a tree ready to trace out,
 * on the caller's stream, no host copy. For EVERY leaf of the node array (reachable or not, like traverse_bottom_up)
 *     box = BBox::make_empty()                                            (+max, -max; bbox.h:40-44)
 *     for i in [first_id, first_id + prim_count): box.extend(bboxes[prim_ids[i]])      in this order (bbox.h:23-27)
 * with extend = robust_min / robust_max (utils.h:41-43: `a < b ? a : b` / `a > b ? a : b` with the accumulated value as a). Order and
 * the direction of the comparison are part of the contract: whenever `a < b` is false the OTHER value is taken, so of +0 and -0 the
 * one met last stays, and a NaN component replaces the accumulated value and is itself replaced by the next primitive's (a NaN in
 * the leaf's last primitive stays in the box) — exactly what the loop a user of the reference writes inside refit(leaf_fn) does. Every inner box is then left.extend(right), children before parents. 2D trees keep z = (+0, +0).
 *
 * refit_boxes: d_bboxes has the layout of the build input (bvhXX_build_device: n x {min, max}; 2D: n x {min.x, min.y, max.x, max.y})
 *   and is indexed by ORIGINAL primitive id, i.e. by the values of prim_ids.
 * refit_tris (3D): d_tris9 = n x {p0, p1, p2} in original order; bboxes[j] = Tri::get_bbox() = BBox(p0).extend(p1).extend(p2)
 *   (tri.h:24, bit-identical to bvh_amd_tri_bounds3X). If d_tris12_out is not NULL it receives PrecomputedTri(tris[prim_ids[i]]) for
 *   every BVH-order slot i, byte-identical to bvh_amd_precompute_tris3X(d_tris9, bvhXX_device_prim_ids(bvh), prim_count, out): one
 *   call per frame takes deformed vertices to a traceable (tree, primitives) pair. It may be the array earlier launches read: the
 *   call is ordered on `stream` like any other work.
 *
 * Both calls
 *   - are asynchronous on `stream` (NULL = the default stream) from the second call on a tree: no synchronisation, no copy of node
 *     arrays, no allocation (scratch comes from the per-stream block cache). The first call pays one read-back (the largest prim id);
 *   - update in place both device representations: the reference-layout nodes (serialize_device, extract, optimize, broadcast keep
 *     working) and the traversal records (same allocation). Index words are never written;
 *   - keep what depends on the topology only: the tree depth, the measured launch plan (a plan affects speed, never results), the
 *     device prim ids. The root box the ray / query reordering scales its keys by is refreshed behind an event the next launch waits
 *     for; the expected-visits figure of the plan predictor is left as it was (bvh3X_traversal_cost recomputes it);
 *   - mark the host mirror stale instead of copying it back; the next accessor refills it. Node pointers obtained from
 *     bvhXX_get_node BEFORE the call still point at valid memory (they are invalidated by append only), but what is written through
 *     them after the call and before the next accessor is discarded by that refill: fetch node pointers again after a refit_* call.
 *     If the mirror is valid when the call arrives (an accessor ran since the last device operation, or the tree came from
 *     from_nodes / load / deserialize), it is pushed, validated and the records are rebuilt first, exactly as bvhXX_refit does on
 *     every call — leaf boxes and inner boxes set through the mirror do not survive the refit, index edits do. A one-off, not a
 *     per-frame cost, as long as the frame loop does not touch the mirror;
 *   - validate before touching anything: bvh and pointers non-NULL, n_boxes / n_tris larger than the largest value in prim_ids.
 *     On failure: a negative code, bvh_amd_last_error(), tree unchanged;
 *   - are NOT re-entrant (they write the tree): launches that read the tree (bvhXX_intersect_rays_*, bvhXX_closest_points_*,
 *     serialize_device, ...) must be ordered before / after the refit by the caller (same stream, or events). */
BVH_AMD_API int bvh3f_refit_boxes(struct bvh3f*, const float* d_bboxes, size_t n_boxes, void* stream);
BVH_AMD_API int bvh3d_refit_boxes(struct bvh3d*, const double* d_bboxes, size_t n_boxes, void* stream);
BVH_AMD_API int bvh3f_refit_tris(struct bvh3f*, const float* d_tris9, size_t n_tris, float* d_tris12_out, void* stream);
BVH_AMD_API int bvh3d_refit_tris(struct bvh3d*, const double* d_tris9, size_t n_tris, double* d_tris12_out, void* stream);
/* The figure to watch to decide "refit again or rebuild" (it grows as a refitted tree degrades): the number of traversal records a
 * random line through the scene is expected to fetch = the sum over the inner nodes OTHER THAN THE ROOT (the terms are taken per
 * inner child of a record, and the root is nobody's child) of half_area(node) / half_area(root), half_area = xy + yz + zx, computed
 * from the CURRENT records, each term truncated to units of 2^-16 (an integer sum: the result does not depend on the order of the
 * atomics). Synchronous on `stream` (one read-back). 3D trees only. */
BVH_AMD_API int bvh3f_traversal_cost(struct bvh3f*, double* cost_out, void* stream);
BVH_AMD_API int bvh3d_traversal_cost(struct bvh3d*, double* cost_out, void* stream);
BVH_AMD_API int bvh3f_sync_device(struct bvh3f*);
BVH_AMD_API int bvh3d_sync_device(struct bvh3d*);
BVH_AMD_API void bvh3f_append_node(struct bvh3f*);
BVH_AMD_API void bvh3d_append_node(struct bvh3d*);
BVH_AMD_API void bvh3f_remove_last_node(struct bvh3f*);
BVH_AMD_API void bvh3d_remove_last_node(struct bvh3d*);
BVH_AMD_API void bvh_node3f_set_prim_count(struct bvh_node3f*, size_t);
BVH_AMD_API void bvh_node3d_set_prim_count(struct bvh_node3d*, size_t);
BVH_AMD_API void bvh_node3f_set_first_id(struct bvh_node3f*, size_t);
BVH_AMD_API void bvh_node3d_set_first_id(struct bvh_node3d*, size_t);
BVH_AMD_API void bvh_node3f_set_bbox(struct bvh_node3f*, const struct bvh_bbox3f*);
BVH_AMD_API void bvh_node3d_set_bbox(struct bvh_node3d*, const struct bvh_bbox3d*);

/* ---- serialization (c_api/bvh.h:136-144; byte format of Bvh::serialize, bvh.h:221-229) -------- */
BVH_AMD_API void bvh3f_save(const struct bvh3f*, FILE*);
BVH_AMD_API void bvh3d_save(const struct bvh3d*, FILE*);
BVH_AMD_API struct bvh3f* bvh3f_load(FILE*);
BVH_AMD_API struct bvh3d* bvh3d_load(FILE*);
/* Additive: the same byte stream to/from memory (it is the RCCL broadcast payload). Returns the
 * stream size; writes only if cap is large enough. */
BVH_AMD_API size_t bvh3f_serialize(const struct bvh3f*, void* out, size_t cap);
BVH_AMD_API size_t bvh3d_serialize(const struct bvh3d*, void* out, size_t cap);
BVH_AMD_API struct bvh3f* bvh3f_deserialize(const void* bytes, size_t size);
BVH_AMD_API struct bvh3d* bvh3d_deserialize(const void* bytes, size_t size);
/* The same stream in DEVICE memory (bvh.h:221-243, node.h:90-102): written from / turned into the resident nodes by kernels and
 * device-to-device copies, so the RCCL broadcast of a scene moves no payload byte through the host (deserialize reads the
 * 16-byte header and the root node only). d_out / d_bytes must be aligned to the index type (4 bytes float, 8 double).
 * serialize: returns the stream size, writes (asynchronously on `stream`) only if cap suffices, 0 on error.
 * deserialize: validates the structure the traversal relies on (children adjacent at an odd index, leaf ranges inside prim_ids);
 * the buffer may be released when the call returns. */
BVH_AMD_API size_t bvh3f_serialize_device(struct bvh3f*, void* d_out, size_t cap, void* stream);
BVH_AMD_API size_t bvh3d_serialize_device(struct bvh3d*, void* d_out, size_t cap, void* stream);
BVH_AMD_API struct bvh3f* bvh3f_deserialize_device(const void* d_bytes, size_t size, void* stream);
BVH_AMD_API struct bvh3d* bvh3d_deserialize_device(const void* d_bytes, size_t size, void* stream);

/* ---- accessors (c_api/bvh.h:148-203), on the host mirror -------------------------------------- */
BVH_AMD_API struct bvh_node3f* bvh3f_get_node(struct bvh3f*, size_t);
BVH_AMD_API struct bvh_node3d* bvh3d_get_node(struct bvh3d*, size_t);
BVH_AMD_API size_t bvh3f_get_prim_id(const struct bvh3f*, size_t);
BVH_AMD_API size_t bvh3d_get_prim_id(const struct bvh3d*, size_t);
BVH_AMD_API size_t bvh3f_get_prim_count(const struct bvh3f*);
BVH_AMD_API size_t bvh3d_get_prim_count(const struct bvh3d*);
BVH_AMD_API size_t bvh3f_get_node_count(const struct bvh3f*);
BVH_AMD_API size_t bvh3d_get_node_count(const struct bvh3d*);
BVH_AMD_API bool bvh_node3f_is_leaf(const struct bvh_node3f*);
BVH_AMD_API bool bvh_node3d_is_leaf(const struct bvh_node3d*);
BVH_AMD_API size_t bvh_node3f_get_prim_count(const struct bvh_node3f*);
BVH_AMD_API size_t bvh_node3d_get_prim_count(const struct bvh_node3d*);
BVH_AMD_API size_t bvh_node3f_get_first_id(const struct bvh_node3f*);
BVH_AMD_API size_t bvh_node3d_get_first_id(const struct bvh_node3d*);
BVH_AMD_API struct bvh_bbox3f bvh_node3f_get_bbox(const struct bvh_node3f*);
BVH_AMD_API struct bvh_bbox3d bvh_node3d_get_bbox(const struct bvh_node3d*);
/* Additive bulk accessors: copy all nodes (reference layout) / prim ids out of the host mirror. */
BVH_AMD_API void bvh3f_copy_nodes(const struct bvh3f*, void* out_nodes28);
BVH_AMD_API void bvh3d_copy_nodes(const struct bvh3d*, void* out_nodes56);
BVH_AMD_API void bvh3f_copy_prim_ids(const struct bvh3f*, size_t* out);
BVH_AMD_API void bvh3d_copy_prim_ids(const struct bvh3d*, size_t* out);
/* Device-resident prim ids (uint32, BVH order) for device-side permutation of primitives. */
BVH_AMD_API const uint32_t* bvh3f_device_prim_ids(const struct bvh3f*);
BVH_AMD_API const uint32_t* bvh3d_device_prim_ids(const struct bvh3d*);

/* ---- primitive preparation on the device (caller-side loops of test/benchmark.cpp:205-225) ---- */
/* tris9: n x {p0,p1,p2}. Writes Tri::get_bbox / Tri::get_center (tri.h:24-25). */
BVH_AMD_API int bvh_amd_tri_bounds3f(const float* d_tris9, size_t n, float* d_bboxes, float* d_centers, void* stream);
BVH_AMD_API int bvh_amd_tri_bounds3d(const double* d_tris9, size_t n, double* d_bboxes, double* d_centers, void* stream);
/* out[i] = PrecomputedTri(tris[perm ? perm[i] : i]) (tri.h:35-37): n x {p0,e1,e2,n}. */
BVH_AMD_API int bvh_amd_precompute_tris3f(const float* d_tris9, const uint32_t* d_perm, size_t n, float* d_tris12, void* stream);
BVH_AMD_API int bvh_amd_precompute_tris3d(const double* d_tris9, const uint32_t* d_perm, size_t n, double* d_tris12, void* stream);
/* spheres4: n x {center, radius}. Sphere::get_bbox / get_center (sphere.h:24-27). */
BVH_AMD_API int bvh_amd_sphere_bounds3f(const float* d_sph4, size_t n, float* d_bboxes, float* d_centers, void* stream);
BVH_AMD_API int bvh_amd_sphere_bounds3d(const double* d_sph4, size_t n, double* d_bboxes, double* d_centers, void* stream);
/* out[i] = in[perm[i]] for records of `stride` bytes (multiple of 4). */
BVH_AMD_API int bvh_amd_gather(const void* d_in, const uint32_t* d_perm, size_t n, size_t stride, void* d_out, void* stream);

/* The renderer of the reference's benchmark (test/benchmark.cpp:340-371) around the batch traversal: primary rays of its
 * pinhole camera, row-major (y, x): Ray(eye, normalize(dir) + u * right + v * up), u = 2x/w - 1, v = 2y/h - 1 (:343-359);
 * eye/dir/up are HOST float[3]. */
BVH_AMD_API int bvh_amd_pinhole_rays3f(const float eye[3], const float dir[3], const float up[3], size_t width, size_t height,
    struct bvh_ray3f* d_rays, void* stream);
BVH_AMD_API int bvh_amd_pinhole_rays3d(const double eye[3], const double dir[3], const double up[3], size_t width, size_t height,
    struct bvh_ray3d* d_rays, void* stream);
/* ... and its eyelight shading (:363-371): rgb[3i..3i+2] = clamp(int(|dot(normalize(tri.n), ray.dir)| * 256), 0, 255), 0 for a
 * miss. d_tris12 = the BVH-ordered PrecomputedTri array the rays were traced against. */
BVH_AMD_API int bvh_amd_shade_eyelight3f(const float* d_tris12, const struct bvh_ray3f* d_rays, const struct bvh_hit3f* d_hits, size_t n,
    uint8_t* d_rgb, void* stream);
BVH_AMD_API int bvh_amd_shade_eyelight3d(const double* d_tris12, const struct bvh_ray3d* d_rays, const struct bvh_hit3d* d_hits, size_t n,
    uint8_t* d_rgb, void* stream);

/* ---- batched traversal: Bvh::intersect<IsAnyHit, IsRobust> (bvh.h:160-182) for n rays ---------- */
/* d_prims are in BVH order (prims[i] belongs to prim_ids[i]), like the reference's permuted
 * primitives (test/simple_example.cpp:57-65). d_counters may be NULL. Re-entrant like Bvh::intersect on a const Bvh: launches
 * of one BVH may be issued concurrently from several host threads and on several streams (up to 64 in flight per BVH).
 * (bvhXX_refit_boxes / bvh3X_refit_tris WRITE the tree and are not re-entrant: order them against these launches.) */
BVH_AMD_API int bvh3f_intersect_rays_tri(const struct bvh3f*, const float* d_tris12, const struct bvh_ray3f* d_rays,
    size_t n, unsigned flags, struct bvh_hit3f* d_hits, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3d_intersect_rays_tri(const struct bvh3d*, const double* d_tris12, const struct bvh_ray3d* d_rays,
    size_t n, unsigned flags, struct bvh_hit3d* d_hits, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3f_intersect_rays_sphere(const struct bvh3f*, const float* d_sph4, const struct bvh_ray3f* d_rays,
    size_t n, unsigned flags, struct bvh_hit3f* d_hits, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3d_intersect_rays_sphere(const struct bvh3d*, const double* d_sph4, const struct bvh_ray3d* d_rays,
    size_t n, unsigned flags, struct bvh_hit3d* d_hits, struct bvh_amd_counters* d_counters, void* stream);

/* ---- batched closest-point queries: for each point, the nearest primitive and its distance ------------------------------- */
/* d_queries4 holds n x {x, y, z, max_distance} of the tree's scalar type (16 B per query for 3f, 32 B for 3d); d_prims are the
 * BVH-order PrecomputedTri (tri) or Sphere<T, 3> {c, r} (sphere) arrays that bvhXX_intersect_rays_* take. One record per query:
 *   hit:  prim = the BVH-order index (bvh.prim_ids[i] with BVH_AMD_RAY_ORIGINAL_IDS) of the primitive at the smallest squared
 *         distance <= max_distance^2 among the primitives the walk tests, ties among those to the lowest index; t = sqrt(d^2). A
 *         subtree is skipped when its box's computed squared distance exceeds the best so far, so a primitive whose computed distance
 *         rounds below its box's can hide one at an equal or one-ulp-nearer distance: the record is the brute force's argmin by
 *         (d2, index) exactly when the distances are computed exactly, and its distance is within rounding of it otherwise. Triangles: distance to the solid triangle, (u, v) the
 *         barycentrics of its closest point, point = p0 + u (p1 - p0) + v (p2 - p0). Spheres: max(|q - c| - r, 0), u = v = 0.
 *   miss: prim = BVH_AMD_INVALID, t = max_distance, u = v = 0 (also for a NaN coordinate and a negative or NaN max_distance;
 *         +inf = unbounded).
 * flags: BVH_AMD_RAY_ORIGINAL_IDS, BVH_AMD_RAY_SORTED / BVH_AMD_RAY_UNSORTED (reorder the batch by the Hilbert cell of each point in the
 * root box, or never; with neither the library reorders batches of >= 1M queries). Any other bit: BVH_AMD_ERR_ARG. A record depends
 * only on the tree, the primitives and its query (not on batch size, position or order). n == 0 is a no-op. Device pointers must be
 * 16-byte aligned; d_counters (optional) receives {pair records fetched, primitives tested, leaves visited}. 3D trees only.
 * Re-entrant on a const tree, like bvhXX_intersect_rays_*. */
BVH_AMD_API int bvh3f_closest_points_tri(const struct bvh3f*, const float* d_tris12, const float* d_queries4, size_t n, unsigned flags,
    struct bvh_hit3f* d_out, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3d_closest_points_tri(const struct bvh3d*, const double* d_tris12, const double* d_queries4, size_t n, unsigned flags,
    struct bvh_hit3d* d_out, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3f_closest_points_sphere(const struct bvh3f*, const float* d_sph4, const float* d_queries4, size_t n, unsigned flags,
    struct bvh_hit3f* d_out, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3d_closest_points_sphere(const struct bvh3d*, const double* d_sph4, const double* d_queries4, size_t n, unsigned flags,
    struct bvh_hit3d* d_out, struct bvh_amd_counters* d_counters, void* stream);

/* ---- batched radius queries: for each point, every primitive within a distance -------------------------------------------------- */
/* Queries and primitives as for bvhXX_closest_points_* (n x {x, y, z, max_distance}; BVH-order PrecomputedTri or Sphere<T, 3>). With
 * r2 = max_distance * max_distance, the result of a query is the LIST of BVH-order indices i with d2(i) <= r2, d2 being the squared
 * distance bvhXX_closest_points_* measures (solid triangle; max(|q - c| - r, 0)^2 for a sphere). A subtree is entered iff the
 * squared distance of its box to the point is <= r2.
 *   order:   fixed by the tree. The walk is depth-first, a node's left child (first_id) before its right (first_id + 1), ascending
 *            index inside a leaf; there is no near-first ordering.
 *   invalid: a NaN coordinate and a negative or NaN max_distance give an empty list; +inf gives every reachable primitive; 0 gives the
 *            primitives at distance exactly 0.
 *   output:  d_counts[q] (n entries, or NULL) = the number of primitives within the radius, NEVER truncated. d_offsets (n + 1 entries,
 *            or NULL = count pass, no list written): query q owns [d_offsets[q], d_offsets[q + 1]) of d_list_prims (required iff
 *            d_offsets) and d_list_dist (optional, sqrt(d2) correctly rounded, parallel to d_list_prims). The first min(count, segment
 *            length) entries of its list are written there in walk order; the rest of the segment is padded with BVH_AMD_INVALID and
 *            distance = the query's max_distance (the miss record of closest_points). Nothing outside a query's segment is written;
 *            a segment whose end does not exceed its begin is empty. At least one of d_counts and d_offsets must be given. Hence:
 *            count, bvh_amd_offsets_from_counts, fill = exact compressed-sparse-row lists; d_offsets = k * {0, 1, ..., n} = k slots
 *            per query in one pass, d_counts telling which lists overflowed; d_counts alone = count only.
 *   flags:   BVH_AMD_RAY_ORIGINAL_IDS lists bvh.prim_ids[i] instead of i (the order stays the walk's); BVH_AMD_RAY_SORTED /
 *            BVH_AMD_RAY_UNSORTED as for closest_points (with neither, batches of >= 1M queries are reordered internally). Any other
 *            bit: BVH_AMD_ERR_ARG. n == 0 is a no-op.
 * A query's count and list depend only on the tree, the primitives and the query: not on batch size, position or order, the
 * reordering flags, the stream or the thread. d_counters (optional) receives {pair records fetched, primitives tested, leaves
 * visited}. Alignment: d_prims and d_queries4 16 bytes, d_offsets and d_counters 8, d_counts, d_list_prims and a float d_list_dist 4,
 * a double d_list_dist 8. 3D trees only; a 2D tree, a NULL or misaligned pointer and a tree without a device copy are refused with
 * BVH_AMD_ERR_ARG. Re-entrant on a const tree (no work slot of the tree is claimed). */
BVH_AMD_API int bvh3f_radius_search_tri(const struct bvh3f*, const float* d_tris12, const float* d_queries4, size_t n, unsigned flags,
    uint32_t* d_counts, const uint64_t* d_offsets, uint32_t* d_list_prims, float* d_list_dist, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3d_radius_search_tri(const struct bvh3d*, const double* d_tris12, const double* d_queries4, size_t n, unsigned flags,
    uint32_t* d_counts, const uint64_t* d_offsets, uint32_t* d_list_prims, double* d_list_dist, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3f_radius_search_sphere(const struct bvh3f*, const float* d_sph4, const float* d_queries4, size_t n, unsigned flags,
    uint32_t* d_counts, const uint64_t* d_offsets, uint32_t* d_list_prims, float* d_list_dist, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3d_radius_search_sphere(const struct bvh3d*, const double* d_sph4, const double* d_queries4, size_t n, unsigned flags,
    uint32_t* d_counts, const uint64_t* d_offsets, uint32_t* d_list_prims, double* d_list_dist, struct bvh_amd_counters* d_counters, void* stream);
/* d_offsets[0..n] = {0, c0, c0 + c1, ...} of d_counts[0..n): 64-bit sums, asynchronous on `stream` (no host read-back). n == 0
 * writes d_offsets[0] = 0. */
BVH_AMD_API int bvh_amd_offsets_from_counts(const uint32_t* d_counts, size_t n, uint64_t* d_offsets, void* stream);

/* ---- batched k-nearest queries: for each point, the k nearest primitives in ascending distance ----------------------------------- */
/* Queries and primitives as for bvhXX_closest_points_* (n x {x, y, z, max_distance}; BVH-order PrecomputedTri or Sphere<T, 3>); k in
 * [1, BVH_AMD_KNN_MAX_K]. With r2 = max_distance * max_distance (rounded in the scalar type), the result of a query is the k smallest
 * pairs (d2, i), in lexicographic order, among the BVH-order indices i with d2(i) <= r2; d2 is the squared distance
 * bvhXX_closest_points_* measures. The pairs are listed in ascending (d2, i) order: equal squared distances by ascending BVH-order
 * index (also when BVH_AMD_RAY_ORIGINAL_IDS maps the reported ids). k = 1 is closest_points' {prim, t}. As there, "smallest" is among
 * the primitives the walk tests: that is the whole scene, and the row the brute force's, when the distances are computed exactly; with
 * rounded distances a primitive computed nearer than its own box can hide an equal or one-ulp-nearer one in a skipped subtree, and
 * the row's distances differ from the brute force's by rounding only.
 *   output:  d_out_prims (n x k, row-major, caller order, required): BVH-order indices (bvh.prim_ids[i] with
 *            BVH_AMD_RAY_ORIGINAL_IDS). d_out_dist (n x k, or NULL): sqrt(d2), correctly rounded. d_counts (n, or NULL): the valid
 *            entries of each row, <= k. The unused slots of a row hold {BVH_AMD_INVALID, max_distance} (the miss record of
 *            closest_points, the padding of radius_search). Nothing outside [0, n * k) of the output arrays is written.
 *   invalid: a NaN coordinate and a negative or NaN max_distance give count 0 and a fully padded row whose distances carry the query's
 *            own max_distance bits; +inf is unbounded; 0 yields the primitives at distance exactly 0.
 *   walk:    that of closest_points, pruned against the worst candidate: a subtree is entered iff the squared distance of its box is
 *            <= r2 while fewer than k candidates are held, <= the k-th smallest d2 held afterwards.
 *   flags:   BVH_AMD_RAY_ORIGINAL_IDS, BVH_AMD_RAY_SORTED / BVH_AMD_RAY_UNSORTED as for closest_points (with neither, batches of >= 1M
 *            queries are reordered internally). Any other bit: BVH_AMD_ERR_ARG. n == 0 is a no-op.
 * A row depends only on the tree, the primitives and its query: not on batch size, position or order, the flags, the stream or the
 * thread. d_counters (optional) receives {pair records fetched, primitives tested, leaves visited}. Alignment: d_prims and d_queries4
 * 16 bytes, d_counters and a double d_out_dist 8, the rest 4. 3D trees only; k == 0 or k > BVH_AMD_KNN_MAX_K, a 2D tree, a NULL handle,
 * NULL prims, queries or d_out_prims, a misaligned pointer and a tree without a device copy are refused with BVH_AMD_ERR_ARG.
 * Re-entrant on a const tree (no work slot of the tree is claimed). */
#define BVH_AMD_KNN_MAX_K 64
BVH_AMD_API int bvh3f_knn_tri(const struct bvh3f*, const float* d_tris12, const float* d_queries4, size_t n, unsigned k, unsigned flags,
    uint32_t* d_out_prims, float* d_out_dist, uint32_t* d_counts, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3d_knn_tri(const struct bvh3d*, const double* d_tris12, const double* d_queries4, size_t n, unsigned k, unsigned flags,
    uint32_t* d_out_prims, double* d_out_dist, uint32_t* d_counts, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3f_knn_sphere(const struct bvh3f*, const float* d_sph4, const float* d_queries4, size_t n, unsigned k, unsigned flags,
    uint32_t* d_out_prims, float* d_out_dist, uint32_t* d_counts, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3d_knn_sphere(const struct bvh3d*, const double* d_sph4, const double* d_queries4, size_t n, unsigned k, unsigned flags,
    uint32_t* d_out_prims, double* d_out_dist, uint32_t* d_counts, struct bvh_amd_counters* d_counters, void* stream);

/* ---- batched winding numbers: is a point inside the mesh? (and, with closest_points, signed distance) ------------------------------ */
/* The generalized winding number of the triangle mesh at each query point, evaluated hierarchically (Barill et al., "Fast Winding
 * Numbers for Soups and Clouds", 2018; first order): for a closed mesh whose ab x ac = (p1 - p0) x (p2 - p0) point outward it is 1
 * inside and 0 outside; it is 0 in the cavity of a shell (an inner surface facing the cavity), 2 inside a doubled surface, and degrades
 * to fractional values near the holes of an open or defective mesh instead of flipping as crossing parity does. (d_tris12 holds
 * n = cross(p0 - p1, p2 - p0) = -(ab x ac); the area vector of a triangle is A = (ab x ac) / 2 = -n / 2.)
 *
 * bvh3X_winding_prepare writes the per-node moments into the CALLER's buffer d_moments: moments_rows >= node_count + 1 rows of 8
 * scalars of the tree's type (32 B / 64 B a row). Node c is row c + 1, row 0 is zero, so the two children of a pair record share one
 * aligned 16-scalar line. A row is {cx, cy, cz, r2, Nx, Ny, Nz, area}: N = the sum of the area vectors below the node, area = the sum
 * of their lengths, c = the area-weighted mean of the triangles' centroids (the centre of the node's box when area is 0), r2 = the
 * squared distance from c to the farthest corner of the node's box. A leaf sums its triangles in ascending BVH-order index, an inner
 * node is always left + right: the bytes depend on the tree and the triangles only. r2 bounds the triangles as long as the tree's
 * boxes do (after a build or bvh3X_refit_tris). Asynchronous on `stream`; reads the tree (its traversal records) and writes only
 * d_moments: re-entrant on a const tree. The moments are STALE after bvh3X_refit_tris and after bvhXX_optimize: prepare them again.
 *
 * bvh3X_winding_numbers: d_queries4 is the array bvhXX_closest_points_* take, n x {x, y, z, ignored} (the max_distance slot is not
 * read). Per query, depth-first from the root, the left child before the right, nothing pruned against what was found: a node with
 * |c - q|^2 > beta^2 r2 adds N . (c - q) / |c - q|^3; otherwise a leaf adds, for each of its triangles in ascending index, the solid
 * angle 2 atan2(det(a, b, c), |a||b||c| + (a.b)|c| + (a.c)|b| + (b.c)|a|) (a, b, c = the vertices minus q; a zero determinant adds 0),
 * and an inner node is opened. d_w[q] = sum / 4 pi, accumulated in the tree's type in that order.
 *   beta:    the accuracy knob, >= 1; 2 is the default of the other layers, +inf never takes the far branch and gives the exact sum.
 *            beta < 1 or NaN: BVH_AMD_ERR_ARG.
 *   special: a NaN or infinite query coordinate gives w = NaN and leaves the query's hit record alone. Finite input never yields NaN or inf as long as
 *            the product of three distances from a query to the mesh is representable: with d the largest such distance, 8 d^3 must
 *            not overflow (float: d below about 3e12; double: 8e101) and d^2 must not underflow. ON the surface the value lies between the two sides' values and is
 *            otherwise unspecified.
 *   d_hits:  optional, the records bvh3X_closest_points_tri wrote for the same queries: t is negated where w >= 1/2, nothing else is
 *            touched. That is the whole of signed distance (negative inside).
 *   flags:   BVH_AMD_RAY_SORTED / BVH_AMD_RAY_UNSORTED as for closest_points (with neither, batches of >= 1M queries are reordered
 *            internally). BVH_AMD_RAY_ORIGINAL_IDS is refused (there is nothing to map), like any other bit. n == 0 is a no-op.
 * A value depends only on the tree, the triangles, the moments, beta and its query: not on batch size, position or order, the flags,
 * the stream or the thread. d_counters (optional) receives {pair records opened, triangles summed exactly, far terms added}.
 * Alignment: d_tris12, d_moments, d_queries4 and d_hits 16 bytes, d_counters 8, d_w its element. 3D trees only; a 2D tree, a NULL
 * handle, NULL tris, moments, queries or d_w, a misaligned pointer, moments_rows < node_count + 1 and a tree without a device copy
 * are refused with BVH_AMD_ERR_ARG and nothing is written. Re-entrant on a const tree (no work slot of the tree is claimed). */
BVH_AMD_API int bvh3f_winding_prepare(const struct bvh3f*, const float* d_tris12, float* d_moments, size_t moments_rows, void* stream);
BVH_AMD_API int bvh3d_winding_prepare(const struct bvh3d*, const double* d_tris12, double* d_moments, size_t moments_rows, void* stream);
BVH_AMD_API int bvh3f_winding_numbers(const struct bvh3f*, const float* d_tris12, const float* d_moments, size_t moments_rows,
    const float* d_queries4, size_t n, double beta, unsigned flags, float* d_w, struct bvh_hit3f* d_hits, struct bvh_amd_counters* d_counters,
    void* stream);
BVH_AMD_API int bvh3d_winding_numbers(const struct bvh3d*, const double* d_tris12, const double* d_moments, size_t moments_rows,
    const double* d_queries4, size_t n, double beta, unsigned flags, double* d_w, struct bvh_hit3d* d_hits, struct bvh_amd_counters* d_counters,
    void* stream);

/* ---- batched box-overlap queries and self-overlap pairs (broad phase) ------------------------------------------------------------ */
/* d_bboxes is the array bvhXX_build_device and bvhXX_refit_boxes take: n_boxes x {min.xyz, max.xyz}, indexed by ORIGINAL primitive
 * id; the box of BVH-order primitive i is d_bboxes[prim_ids[i]], so the kind of primitive the tree was built over does not matter.
 * n_boxes must exceed the largest prim id. d_queries6 is n x {min.xyz, max.xyz} in the same layout.
 *   test:    closed intervals: boxes a and b overlap iff on every axis a.min <= b.max && b.min <= a.max. Touching boxes overlap, -0
 *            equals +0, a zero-extent box is a point and overlaps what contains it. A NaN component, or min > max, in the query or in
 *            a primitive's box makes every comparison that involves it false: an empty list, or a primitive that is never listed.
 *            The same expression decides whether a child is entered (its box against the query) and whether a primitive is listed.
 *   result:  every BVH-order index i whose box overlaps the query and all of whose ancestors' boxes overlap it. For a tree fitted to
 *            these boxes (built from them, or bvhXX_refit_boxes with them: every ancestor box is the min / max union of the boxes
 *            below it) that is EXACTLY the brute-force set. For boxes the tree was not fitted to it is the walk's set.
 *   order:   that of bvhXX_radius_search_*: depth-first, left child before right, ascending index inside a leaf; nothing is pruned.
 *   output:  that of bvhXX_radius_search_* without distances: d_counts[q] is never truncated; query q owns [d_offsets[q],
 *            d_offsets[q + 1]) of d_list_prims (required iff d_offsets); the first min(count, segment length) entries are written, the
 *            rest of the segment is padded with BVH_AMD_INVALID, nothing outside a segment is written and a non-ascending segment is
 *            empty. At least one of d_counts and d_offsets must be given. Count pass, bvh_amd_offsets_from_counts, fill pass = exact
 *            CSR lists; k fixed slots per query take one pass.
 *   self:    bvh3X_overlap_self takes no queries: n = bvhXX_get_prim_count, query q IS BVH-order primitive q with the box
 *            d_bboxes[prim_ids[q]], and its list holds only i > q (compared in BVH order): every unordered overlapping pair appears
 *            exactly once and no primitive pairs with itself. The CSR (offsets, list) is the pair list; row q stands for primitive q,
 *            or prim_ids[q] for a caller who uses original ids. Self mode never reorders (BVH order is the tree's spatial order):
 *            BVH_AMD_RAY_SORTED and BVH_AMD_RAY_UNSORTED are refused there.
 *   flags:   BVH_AMD_RAY_ORIGINAL_IDS lists prim_ids[i] (the order and the i > q filter stay BVH-order). For bvh3X_overlap_boxes,
 *            BVH_AMD_RAY_SORTED / BVH_AMD_RAY_UNSORTED: the reordering key is the Hilbert cell of the query box's centre in the root
 *            box (with neither, batches of >= 1M queries are reordered). Any other bit: BVH_AMD_ERR_ARG. n == 0 is a no-op.
 * Outputs are in caller order. A query's result does not depend on batch size, position, order, flags, stream or thread. d_counters
 * (optional) receives {pair records fetched, primitive boxes tested, leaves visited}. Alignment: d_bboxes and d_queries6 to their
 * scalar, d_offsets and d_counters 8 bytes, d_counts and d_list_prims 4. Refused with BVH_AMD_ERR_ARG: a 2D tree, a NULL handle, a NULL
 * or misaligned pointer, the forbidden output combinations, a tree without a device copy or without device prim ids, n_boxes at or
 * below the largest prim id. Re-entrant on a const tree (no work slot is claimed); like every reader of the tree, the caller orders
 * it after a bvhXX_refit_*. Not offered: the 2D families, exact primitive-against-box tests (sphere against box: that narrow phase
 * is the caller's; for triangles against triangles see bvh3X_intersect_tris below), a dual-tree (tree against tree) traversal, a
 * fused single-walk list variant. */
BVH_AMD_API int bvh3f_overlap_boxes(const struct bvh3f*, const float* d_bboxes, size_t n_boxes, const float* d_queries6, size_t n, unsigned flags,
    uint32_t* d_counts, const uint64_t* d_offsets, uint32_t* d_list_prims, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3d_overlap_boxes(const struct bvh3d*, const double* d_bboxes, size_t n_boxes, const double* d_queries6, size_t n, unsigned flags,
    uint32_t* d_counts, const uint64_t* d_offsets, uint32_t* d_list_prims, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3f_overlap_self(const struct bvh3f*, const float* d_bboxes, size_t n_boxes, unsigned flags,
    uint32_t* d_counts, const uint64_t* d_offsets, uint32_t* d_list_prims, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3d_overlap_self(const struct bvh3d*, const double* d_bboxes, size_t n_boxes, unsigned flags,
    uint32_t* d_counts, const uint64_t* d_offsets, uint32_t* d_list_prims, struct bvh_amd_counters* d_counters, void* stream);

/* ---- batched triangle-intersection queries and mesh self-intersections (narrow phase) ---------------------------------------------- */
/* d_tris9 is the array bvh3X_refit_tris takes: n_tris x {p0.xyz, p1.xyz, p2.xyz}, indexed by ORIGINAL primitive id; the triangle of
 * BVH-order primitive i is d_tris9[prim_ids[i]]. n_tris must exceed the largest prim id. d_queries9 is n x 9 scalars in the same layout.
 *   test:    two triangles intersect iff they share a point as CLOSED sets: touching at a vertex or along an edge counts, and so does
 *            coplanar containment. The decision is taken from SIGNS of determinants of coordinate differences only: the side of a
 *            vertex against the other triangle's plane ((v - p0) . n, n = (p1 - p0) x (p2 - p0)), 3 x 3 determinants of differences
 *            that order the two triangles' intervals on the line their planes share, and for coplanar triangles 2 x 2 orientations in
 *            the projection along the largest component of the query's normal. No division, no square root, no epsilon, no product
 *            of two determinants: whenever every determinant is computed without rounding (small integers, say) the answer is the
 *            exact one; otherwise it is the one these roundings give (one rounding per operation, no contraction), the same on the
 *            device and in a host build of the same source. Before the signs, the boxes of the two triangles are compared (closed
 *            intervals): boxes apart, no intersection.
 *   invalid: a triangle whose computed normal is (0, 0, 0) (no area), or has a NaN or infinite component (a NaN or infinite
 *            coordinate ends there), intersects nothing: as a query it has an empty list, as a primitive it is never listed. -0 = +0.
 *   result:  every BVH-order index i whose triangle intersects the query's and all of whose ancestors' boxes overlap the box of the
 *            query triangle (the node test of bvh3X_overlap_boxes, closed intervals). For a tree fitted to these triangles (built from
 *            bvh_amd_tri_bounds3X of them, or bvh3X_refit_tris with them) that is EXACTLY the brute-force set of the pair test. For
 *            triangles the tree was not fitted to it is the walk's set.
 *   order, output: those of bvh3X_overlap_boxes: depth-first, left child before right, ascending index inside a leaf; d_counts[q] is
 *            never truncated; query q owns [d_offsets[q], d_offsets[q + 1]) of d_list_prims (required iff d_offsets), the rest of a
 *            segment is padded with BVH_AMD_INVALID, nothing outside a segment is written, a non-ascending segment is empty. At least
 *            one of d_counts and d_offsets must be given.
 *   self:    bvh3X_intersect_tris_self takes no queries: n = bvhXX_get_prim_count, query q IS BVH-order primitive q with the triangle
 *            d_tris9[prim_ids[q]], and its list holds only i > q (compared in BVH order): every unordered intersecting pair appears
 *            exactly once and no triangle pairs with itself. Self mode never reorders: BVH_AMD_RAY_SORTED and BVH_AMD_RAY_UNSORTED are
 *            refused there.
 *   flags:   BVH_AMD_RAY_ORIGINAL_IDS lists prim_ids[i] (the order and the i > q filter stay BVH-order). BVH_AMD_TRI_SKIP_SHARED (both
 *            entry points): a pair in which some vertex of one triangle equals some vertex of the other on all three coordinates
 *            (==: -0 equals +0, a NaN equals nothing) is not listed; without it the neighbours of a mesh's triangle fill its self
 *            list. For bvh3X_intersect_tris, BVH_AMD_RAY_SORTED / BVH_AMD_RAY_UNSORTED: the reordering key is the Hilbert cell of the
 *            centre of the query triangle's box in the root box (with neither, batches of >= 1M queries are reordered). Any other bit:
 *            BVH_AMD_ERR_ARG. n == 0 is a no-op.
 * Outputs are in caller order. A query's result does not depend on batch size, position, order, flags, stream or thread. d_counters
 * (optional) receives {pair records fetched, triangles fetched (in self mode after the i > q filter; before any box or shared-vertex
 * early-out), leaves visited}. Alignment: d_tris9 and d_queries9 to their scalar, d_offsets and d_counters 8 bytes, d_counts and
 * d_list_prims 4. Refused with BVH_AMD_ERR_ARG: a 2D tree, a NULL handle, a NULL or misaligned pointer, the forbidden output
 * combinations, a tree without a device copy or without device prim ids, n_tris at or below the largest prim id. Re-entrant on a const
 * tree (no work slot is claimed); like every reader of the tree, the caller orders it after a bvhXX_refit_*. Not offered: the segment
 * two triangles share, spheres, the 2D families, a dual-tree traversal, exact arithmetic beyond what the inputs make exact. */
BVH_AMD_API int bvh3f_intersect_tris(const struct bvh3f*, const float* d_tris9, size_t n_tris, const float* d_queries9, size_t n, unsigned flags,
    uint32_t* d_counts, const uint64_t* d_offsets, uint32_t* d_list_prims, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3d_intersect_tris(const struct bvh3d*, const double* d_tris9, size_t n_tris, const double* d_queries9, size_t n, unsigned flags,
    uint32_t* d_counts, const uint64_t* d_offsets, uint32_t* d_list_prims, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3f_intersect_tris_self(const struct bvh3f*, const float* d_tris9, size_t n_tris, unsigned flags,
    uint32_t* d_counts, const uint64_t* d_offsets, uint32_t* d_list_prims, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3d_intersect_tris_self(const struct bvh3d*, const double* d_tris9, size_t n_tris, unsigned flags,
    uint32_t* d_counts, const uint64_t* d_offsets, uint32_t* d_list_prims, struct bvh_amd_counters* d_counters, void* stream);

/* ---- batched triangle-distance queries: the nearest mesh triangle to a triangle ---------------------------------------------------- */
/* d_tris9 as for bvh3X_intersect_tris (n_tris x {p0.xyz, p1.xyz, p2.xyz} by ORIGINAL primitive id, n_tris above the largest prim id);
 * d_queries9 is n x 9 scalars in the same layout. A query also has a max_distance: d_max_distances[q] (n scalars, caller order) or,
 * with d_max_distances == NULL, `max_distance` for the whole batch (INFINITY: unbounded). Triangles are closed sets; collinear or
 * coincident vertices are legal on both sides and stand for the segment or point they are.
 *   answer:  the tree triangle nearest to the query triangle within max_distance, as one record {prim, t, u, v}: t = the distance,
 *            (u, v) = the barycentrics of the closest point on the TREE triangle in the convention of bvh3X_closest_points_*
 *            (point = p0 + u (p1 - p0) + v (p2 - p0)). d_query_uv (optional, n x 2 scalars) receives the barycentrics of the closest
 *            point on the QUERY triangle in the same convention: the two points give the separation vector and the contact normal.
 *   t == 0:  for every pair bvh3X_intersect_tris' pair test accepts (run first, on the same vertices: the two queries cannot
 *            disagree). The barycentrics then name a common point up to rounding: where an edge of one triangle crosses or touches
 *            the other's face, or two edges cross. A segment that passes through a triangle also comes out at t ~ 0 (within the
 *            tolerance), although the pair test, which wants area on both sides, does not see it.
 *   else:    the smallest over the 9 edge / edge and the 6 vertex / face pairs, each computed as the distance of two points rebuilt
 *            from clamped parameters: never the distance to a point outside a triangle; within the residual of INTEGRATION.md 3m.
 *   miss:    {BVH_AMD_INVALID, max_distance, 0, 0} and query barycentrics 0: nothing within max_distance, a NaN query coordinate, a NaN
 *            or negative max_distance.
 *   ties:    among the triangles the walk tests, equal squared distances go to the lowest BVH-order index (also under
 *            BVH_AMD_RAY_ORIGINAL_IDS, which maps the reported prim only). The walk enters a child iff the squared distance between
 *            its box and the query triangle's box is <= the best squared distance so far, nearer first, and does not stop at 0. A
 *            subtree whose box is computed to lie beyond the best distance is skipped, so, as for bvh3X_closest_points_*, the
 *            record is the brute force's argmin by (distance^2, index) exactly when the arithmetic is exact, otherwise its distance
 *            is within the stated residual of it.
 *   flags:   BVH_AMD_RAY_ORIGINAL_IDS, BVH_AMD_RAY_SORTED / BVH_AMD_RAY_UNSORTED (bvh3X_intersect_tris' reordering key; with neither,
 *            batches of >= 1M queries are reordered). Any other bit: BVH_AMD_ERR_ARG. n == 0 is a no-op.
 * Outputs are in caller order. A query's record depends only on the tree, the triangles, the query, its max_distance and
 * ORIGINAL_IDS: not on batch size, position or order, the reordering flags, the stream or the thread. d_counters (optional) receives
 * {pair records fetched, leaf triangles fetched (before their box test), leaves visited}. Alignment: d_tris9, d_queries9,
 * d_max_distances and d_query_uv to their scalar, d_hits 16 bytes, d_counters 8. Refused with BVH_AMD_ERR_ARG: a 2D tree, a NULL handle,
 * a NULL d_tris9, d_queries9 or d_hits, a misaligned pointer, a tree without a device copy or without device prim ids, n_tris at or
 * below the largest prim id. Re-entrant on a const tree (no work slot is claimed); like every reader of the tree, the caller orders
 * it after a bvhXX_refit_*. Not offered: spheres, the 2D families, self-proximity with adjacency filtering, the k nearest triangles,
 * all pairs within a distance, a dual-tree traversal. */
BVH_AMD_API int bvh3f_tri_distance(const struct bvh3f*, const float* d_tris9, size_t n_tris, const float* d_queries9, size_t n, float max_distance,
    const float* d_max_distances, unsigned flags, struct bvh_hit3f* d_hits, float* d_query_uv, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3d_tri_distance(const struct bvh3d*, const double* d_tris9, size_t n_tris, const double* d_queries9, size_t n, double max_distance,
    const double* d_max_distances, unsigned flags, struct bvh_hit3d* d_hits, double* d_query_uv, struct bvh_amd_counters* d_counters, void* stream);

/* ---- batched convex-region queries: the primitives inside a set of planes ---------------------------------------------------------- */
/* A query is m planes {nx, ny, nz, d}, 1 <= m <= 8, m one number for the whole batch: d_planes is n x m x 4 scalars of the tree's type.
 * d_tris9 as for bvh3X_intersect_tris (n_prims x {p0.xyz, p1.xyz, p2.xyz} by ORIGINAL primitive id); d_sph4 is n_prims x {centre.xyz,
 * radius} by original id. n_prims must exceed the largest prim id.
 *   value:   of plane p at a point x: ((nx*x0 + ny*x1) + nz*x2) + d, evaluated in exactly this order with one rounding per operation
 *            and no contraction.
 *   region:  x is inside plane p iff value <= 0 (a NaN value is not inside); the region is the set of points inside all m planes:
 *            closed, possibly unbounded, possibly empty. Normals point OUT of the region and need not have unit length. A plane with
 *            a zero normal and d <= 0 holds everywhere (that is how a caller pads to m), one with d > 0 nowhere. -0 equals +0. A query
 *            with a NaN or infinite plane component has an empty list.
 *   CULL:    (triangles, the default) a triangle is rejected iff some plane has none of its three vertices inside. Conservative: a
 *            superset of the triangles that meet the region (a triangle beside an edge or corner of the region can pass every plane
 *            on its own); exact for one plane, for parallel planes and for triangles with a vertex in the region.
 *   EXACT:   (triangles, BVH_AMD_REGION_EXACT) a triangle matches iff triangle and region share a point as CLOSED sets, decided by
 *            SIGNS of 3 x 3 determinants only. With D[p][i] the value of plane p at vertex i, plane p is, in the triangle's (u, v)
 *            parameters, the constraint L_p = (D[p][1] - D[p][0], D[p][2] - D[p][0], D[p][0]), read a*u + b*v + c <= 0; the triangle
 *            adds (-1, 0, 0), (0, -1, 0) and (1, 1, -1). The m + 3 half-planes share a point iff for some pair i < j,
 *            w = cross(L_i, L_j).z != 0 and every other k has sign(w) * dot(L_k, cross(L_i, L_j)) <= 0 (a nonempty bounded polygon
 *            has a vertex). No division, no epsilon, no product of two determinants: where every determinant is computed without
 *            rounding the answer is the exact one, otherwise it is the one these roundings give, the same on the device and in a
 *            host build of the same source. A triangle without area needs no special case. A triangle with a NaN or infinite
 *            coefficient in some L_p (a NaN vertex, an overflow) is not listed. EXACT runs only on triangles that pass CULL: its list
 *            is a subset of CULL's.
 *   spheres: per plane len = sqrt((nx*nx + ny*ny) + nz*nz), s = the value at the centre; the sphere is outside plane p iff
 *            !(s <= r*len) and is listed iff it is outside no plane; it is wholly inside iff s <= -(r*len) for every plane. The
 *            plane-by-plane test only: BVH_AMD_REGION_EXACT is refused for spheres.
 *   result:  every BVH-order index i whose primitive passes its test and all of whose ancestors' boxes pass the node test: for every
 *            plane, the value at the box corner lowest along the normal (max on an axis where the normal's component is < 0, min
 *            otherwise; the same expression as a vertex's value; per axis the kernel takes the smaller of n*min and n*max, which for
 *            finite bounds is that product) is <= 0. Rounding is monotone, so that value is <= the value at
 *            every finite point of the box: for a tree fitted to finite triangles (built from bvh_amd_tri_bounds3X of them, or
 *            bvh3X_refit_tris with them) the result is EXACTLY the brute-force set of the triangle test. A sphere's box is c +- r
 *            after rounding and the sphere test has r*len where the box has r*|n|_1: a sphere within rounding of tangent from outside
 *            can be dropped by the node test. The walk never drops a sphere whose margin r*len - s, evaluated in float64, exceeds
 *            16 u M, u = the unit roundoff of the tree's type, M = |nx|(|cx| + r) + |ny|(|cy| + r) + |nz|(|cz| + r) + |d|
 *            (DESIGN.md has the argument). For primitives the tree was not fitted to the result is the walk's set.
 *   order, output: those of bvh3X_overlap_boxes: depth-first, left child before right, ascending index inside a leaf; d_counts[q] is
 *            never truncated; query q owns [d_offsets[q], d_offsets[q + 1]) of d_list_prims (required iff d_offsets), the rest of a
 *            segment is padded with BVH_AMD_INVALID, nothing outside a segment is written, a non-ascending segment is empty. At least
 *            one of d_counts and d_offsets must be given. d_list_inside (optional, only with d_offsets) is parallel to d_list_prims:
 *            1 = wholly inside the region (all three vertices inside all planes, or the sphere rule above), 0 = crossing; padding 0.
 *   flags:   BVH_AMD_RAY_ORIGINAL_IDS lists prim_ids[i]; BVH_AMD_REGION_EXACT (triangles). The batch is NEVER reordered: an unbounded
 *            region has no cell, so BVH_AMD_RAY_SORTED and BVH_AMD_RAY_UNSORTED are refused; callers get coherence by submitting
 *            tiles in screen order. Any other bit: BVH_AMD_ERR_ARG. n == 0 is a no-op.
 * Outputs are in caller order. A query's result does not depend on batch size, position, stream or thread. d_counters (optional)
 * receives {pair records fetched, primitives tested, leaves visited}. Alignment: d_prims and d_planes to their scalar, d_offsets and
 * d_counters 8 bytes, d_counts and d_list_prims 4. Refused with BVH_AMD_ERR_ARG: a 2D tree, a NULL handle, a NULL or misaligned
 * pointer, the forbidden output combinations, d_list_inside without d_offsets, a tree without a device copy or without device prim
 * ids, n_prims at or below the largest prim id, m outside 1..8, BVH_AMD_REGION_EXACT on spheres. Re-entrant on a const tree (no work
 * slot is claimed); like every reader of the tree, the caller orders it after a bvhXX_refit_*. One lane walks one region and lists
 * its whole output serially: the mapping is for many regions. Not offered: the 2D families, exact sphere-against-polytope tests,
 * boxes as primitives, more than 8 planes, plane masking down the tree, a wave-per-query walk for a single huge region. */
BVH_AMD_API int bvh3f_region_tris(const struct bvh3f*, const float* d_tris9, size_t n_prims, const float* d_planes, size_t m, size_t n, unsigned flags,
    uint32_t* d_counts, const uint64_t* d_offsets, uint32_t* d_list_prims, uint8_t* d_list_inside, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3d_region_tris(const struct bvh3d*, const double* d_tris9, size_t n_prims, const double* d_planes, size_t m, size_t n, unsigned flags,
    uint32_t* d_counts, const uint64_t* d_offsets, uint32_t* d_list_prims, uint8_t* d_list_inside, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3f_region_spheres(const struct bvh3f*, const float* d_sph4, size_t n_prims, const float* d_planes, size_t m, size_t n, unsigned flags,
    uint32_t* d_counts, const uint64_t* d_offsets, uint32_t* d_list_prims, uint8_t* d_list_inside, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3d_region_spheres(const struct bvh3d*, const double* d_sph4, size_t n_prims, const double* d_planes, size_t m, size_t n, unsigned flags,
    uint32_t* d_counts, const uint64_t* d_offsets, uint32_t* d_list_prims, uint8_t* d_list_inside, struct bvh_amd_counters* d_counters, void* stream);

/* ---- batched all-hits ray queries: for each ray, every primitive it crosses --------------------------------------------------------- */
/* Rays and primitives as for bvh3X_intersect_rays_* (n x {org, dir, tmin, tmax}; BVH-order PrecomputedTri or Sphere<T, 3>).
 *   result:  every BVH-order index i that (1) passes the leaf test of bvh3X_intersect_rays_* (tri.h:56-74 / sphere.h:32-49) against
 *            the UNSHORTENED ray: tmax is never updated between tests, and (2) all of whose ancestors' boxes pass the node test
 *            (bvh.h:177-180) against the unshortened [tmin, tmax]; a root that is a leaf is tested without a box test. That is the
 *            set the reference's intersect<false, IsRobust> reports to a leaf_fn that records a hit and never shortens the ray.
 *            Each hit is the record bvh3X_intersect_rays_* writes, with the same (t, u, v) bits: {prim, t, u, v} for a triangle,
 *            {prim, t0, t1, 0} for a sphere. Whenever closest-hit bvh3X_intersect_rays_* with the same ROBUST flag hits, the ray's
 *            list holds that record byte for byte (every test that passes with a shortened tmax passes with the original one);
 *            whenever it misses, the count is 0. For a sphere "that record" is its prim and t0: t1 = min(exit, tmax), and
 *            closest-hit clips it to the tmax it has shortened so far, while the list holds the unclipped one.
 *   order:   that of bvhXX_radius_search_*: depth-first, a node's left child (first_id) before its right, ascending index inside a
 *            leaf. NOT sorted by t and without near / far reordering; equal t are all kept. A caller who wants hits along the ray
 *            sorts each segment by (t, prim).
 *   output:  that of bvhXX_radius_search_*, with one array of hit records in place of its two list arrays: d_counts[r] (n entries,
 *            or NULL) is NEVER truncated. d_offsets (n + 1 entries, or NULL = count pass, no record written): ray r owns
 *            [d_offsets[r], d_offsets[r + 1]) of d_list_hits (required iff d_offsets); the first min(count, segment length) hits are
 *            written there in walk order, the rest of the segment is padded with the miss record of bvh3X_intersect_rays_*,
 *            {BVH_AMD_INVALID, the ray's tmax bits, 0, 0}; nothing outside a segment is written and a segment whose offsets do not
 *            ascend is empty. At least one of d_counts and d_offsets must be given. Count pass, bvh_amd_offsets_from_counts, fill
 *            pass = exact compressed-sparse-row lists; d_offsets = k * {0, 1, ..., n} = k slots per ray in one pass, d_counts
 *            telling which lists overflowed.
 *   invalid: a ray whose tmin or tmax is NaN has count 0 and a fully padded segment. Every other ray is walked, including one with
 *            tmin > tmax, a zero direction or NaN components: it gets whatever the two tests produce, as in the reference.
 *   flags:   BVH_AMD_RAY_ROBUST selects the robust node test (the default is the fast one), as for bvh3X_intersect_rays_*;
 *            BVH_AMD_RAY_ORIGINAL_IDS stores prim_ids[i] in the records (the order stays the walk's); BVH_AMD_RAY_SORTED /
 *            BVH_AMD_RAY_UNSORTED force / forbid reading the batch in the order of the rays' origin cells and direction octants (with
 *            neither, batches of >= 1M rays are reordered). BVH_AMD_RAY_ANY_HIT and any other bit: BVH_AMD_ERR_ARG. n == 0 is a no-op.
 * A ray's count and list depend only on the tree, the primitives, the ray and ROBUST / ORIGINAL_IDS: not on batch size, position or
 * order, the reordering flags, the stream or the thread. d_counters (optional) receives {pair records fetched, primitives tested,
 * leaves visited}. Alignment: d_prims and d_rays 16 bytes, d_offsets and d_counters 8, d_counts 4, d_list_hits to the size of its
 * record (16 / 32). 3D trees only; a 2D tree, a NULL handle, a NULL or misaligned pointer, the forbidden output combinations and a
 * tree without a device copy are refused with BVH_AMD_ERR_ARG. Re-entrant on a const tree (no work slot of the tree is claimed).
 * Not offered: the 2D families, hits sorted by t (the first k of them are bvh3X_intersect_rays_nearest_*, below), instanced
 * (two-level) scenes. */
BVH_AMD_API int bvh3f_intersect_rays_all_tri(const struct bvh3f*, const float* d_tris12, const struct bvh_ray3f* d_rays, size_t n, unsigned flags,
    uint32_t* d_counts, const uint64_t* d_offsets, struct bvh_hit3f* d_list_hits, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3d_intersect_rays_all_tri(const struct bvh3d*, const double* d_tris12, const struct bvh_ray3d* d_rays, size_t n, unsigned flags,
    uint32_t* d_counts, const uint64_t* d_offsets, struct bvh_hit3d* d_list_hits, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3f_intersect_rays_all_sphere(const struct bvh3f*, const float* d_sph4, const struct bvh_ray3f* d_rays, size_t n, unsigned flags,
    uint32_t* d_counts, const uint64_t* d_offsets, struct bvh_hit3f* d_list_hits, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3d_intersect_rays_all_sphere(const struct bvh3d*, const double* d_sph4, const struct bvh_ray3d* d_rays, size_t n, unsigned flags,
    uint32_t* d_counts, const uint64_t* d_offsets, struct bvh_hit3d* d_list_hits, struct bvh_amd_counters* d_counters, void* stream);

/* ---- batched nearest-hits ray queries: for each ray, the first k primitives it crosses, front to back ------------------------------- */
/* Rays, primitives and records as for bvh3X_intersect_rays_all_*. k is in [1, BVH_AMD_RAY_NEAREST_MAX_K]; longer rows are the
 * all-hits query's.
 *   candidate: a BVH-order index i that the walk tests and that passes the leaf test of bvh3X_intersect_rays_* against the UNSHORTENED
 *            ray. Its record is exactly the all-hits record: {prim, t, u, v} for a triangle, {prim, t0, t1 = min(exit, the ray's own
 *            tmax), 0} for a sphere; the tmax the walk has shortened never enters a record.
 *   row:     d_out_hits[r * k .. r * k + k) holds the k smallest (t, i) in lexicographic order among the candidates, ascending; equal
 *            t sort by ascending BVH-order index (also under BVH_AMD_RAY_ORIGINAL_IDS, which maps the reported prim only). Unused
 *            slots hold the miss record of bvh3X_intersect_rays_*, {BVH_AMD_INVALID, the ray's tmax bits, 0, 0}. d_counts[r] (n
 *            entries, or NULL) = the valid records of row r, <= k. Nothing outside [0, n * k) records is written.
 *   walk:    that of bvh3X_intersect_rays_*: depth-first, of two children the ray meets the one it enters first (l0 > r0 takes the
 *            right one), the other stacked with its entry t. Both node tests (bvh.h:177-180) run against [tmin, worst]: worst is the
 *            ray's tmax while fewer than k candidates are held, afterwards the t of the largest (t, i) held. A stacked entry is
 *            dropped iff its entry t > worst. A leaf tests ascending i; while fewer than k are held every candidate is accepted,
 *            afterwards a candidate is accepted iff (t, i) < (worst, worst's index), and it replaces the worst.
 *   relation: k = 1: hit or miss and the t bits are those of closest-hit bvh3X_intersect_rays_* with the same ROBUST flag, and so is
 *            prim unless two tested primitives tie at that t (closest-hit keeps the last one tested there, this query the lowest
 *            index). k >= the ray's all-hits count: the row is the ray's bvh3X_intersect_rays_all_* list sorted by (t, prim), byte for
 *            byte (nothing is pruned while fewer than k are held). In between, "smallest" is among the primitives the walk tests,
 *            as for bvhXX_knn_*: the sorted all-hits prefix unless a box is computed to start behind a primitive it contains.
 *   invalid: a ray whose tmin or tmax is NaN has count 0 and a fully padded row. Every other ray is walked, as for the all-hits query.
 *   flags:   BVH_AMD_RAY_ROBUST, BVH_AMD_RAY_ORIGINAL_IDS, BVH_AMD_RAY_SORTED / BVH_AMD_RAY_UNSORTED as for the all-hits query (the
 *            same reordering key; with neither, batches of >= 1M rays are reordered). BVH_AMD_RAY_ANY_HIT and any other bit:
 *            BVH_AMD_ERR_ARG. n == 0 is a no-op.
 * A ray's row and count depend only on the tree, the primitives, the ray, k and ROBUST / ORIGINAL_IDS: not on batch size, position or
 * order, the reordering flags, the stream or the thread. d_counters (optional) receives {pair records fetched, primitives tested
 * (the write-out's repeated tests not counted), leaves visited}. Alignment: d_prims and d_rays 16 bytes, d_out_hits to the size of
 * its record (16 / 32), d_counters 8, d_counts 4. 3D trees only; k == 0 or k > BVH_AMD_RAY_NEAREST_MAX_K, a 2D tree, a NULL handle, a
 * NULL d_prims, d_rays or d_out_hits, a misaligned pointer and a tree without a device copy are refused with BVH_AMD_ERR_ARG.
 * Re-entrant on a const tree (no work slot of the tree is claimed). Not offered: the 2D families, instanced (two-level) scenes. */
#define BVH_AMD_RAY_NEAREST_MAX_K 64
BVH_AMD_API int bvh3f_intersect_rays_nearest_tri(const struct bvh3f*, const float* d_tris12, const struct bvh_ray3f* d_rays, size_t n, unsigned k,
    unsigned flags, struct bvh_hit3f* d_out_hits, uint32_t* d_counts, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3d_intersect_rays_nearest_tri(const struct bvh3d*, const double* d_tris12, const struct bvh_ray3d* d_rays, size_t n, unsigned k,
    unsigned flags, struct bvh_hit3d* d_out_hits, uint32_t* d_counts, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3f_intersect_rays_nearest_sphere(const struct bvh3f*, const float* d_sph4, const struct bvh_ray3f* d_rays, size_t n, unsigned k,
    unsigned flags, struct bvh_hit3f* d_out_hits, uint32_t* d_counts, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3d_intersect_rays_nearest_sphere(const struct bvh3d*, const double* d_sph4, const struct bvh_ray3d* d_rays, size_t n, unsigned k,
    unsigned flags, struct bvh_hit3d* d_out_hits, uint32_t* d_counts, struct bvh_amd_counters* d_counters, void* stream);

/* ---- batched sphere-cast queries: the first contact of a ball swept along a segment --------------------------------------------- */
/* A query is a ray record {org, dir, tmin, tmax} and a radius r: d_radii[q] (n scalars, caller order) or, with d_radii == NULL,
 * `radius` for the whole batch. The ball's centre is c(t) = org + t * dir for t in [tmin, tmax]; dir need not be unit length, t is the
 * ray parameter and distances are Euclidean. A primitive is a SOLID triangle (BVH-order PrecomputedTri, 12 scalars) or a solid sphere
 * (4 scalars), as bvh3X_closest_points_* takes them.
 *   answer:  the smallest t in [tmin, tmax] with dist(c(t), primitive) <= r (closed), as one record {prim, t, u, v} per query.
 *            (u, v) are the barycentrics of the contact point on the triangle in the convention of bvh3X_closest_points_*:
 *            point = p0 - u * e1 + v * e2; the contact normal is (c(t) - point) / r. A sphere leaf writes u = v = 0.
 *   overlap: a ball that already touches a primitive at tmin reports t = tmin (an initial overlap: t == tmin tells).
 *   dir = 0: allowed; an overlap test at c(tmin). r = 0: allowed; a ray cast against the closed triangle in THIS function's
 *            arithmetic (not promised to match the bits of bvh3X_intersect_rays_*).
 *   miss:    {BVH_AMD_INVALID, the ray's tmax bits, 0, 0}: no contact, a NaN tmin or tmax, a NaN or negative radius.
 *   ties:    among the primitives the walk tests, equal t go to the lowest BVH-order index (also under BVH_AMD_RAY_ORIGINAL_IDS,
 *            which maps the reported prim only). The walk enters a child iff the ray meets its box grown by r on every side within
 *            [tmin, best t so far], nearer entry first; a subtree whose grown box is computed to start behind the best t is skipped,
 *            so, as for bvh3X_closest_points_*, the record is the brute force's argmin by (t, index) exactly when the arithmetic is
 *            exact, otherwise within the residual stated in INTEGRATION.md 3l.
 *   flags:   BVH_AMD_RAY_ROBUST (the robust box test), BVH_AMD_RAY_ORIGINAL_IDS, BVH_AMD_RAY_SORTED / BVH_AMD_RAY_UNSORTED (the
 *            reordering key of the all-hits query; with neither, batches of >= 1M queries are reordered). Any other bit:
 *            BVH_AMD_ERR_ARG. n == 0 is a no-op.
 *   t < 0:   with BVH_AMD_RAY_ROBUST no contact at t >= 0 is lost to the box test; below 0 (a negative tmin) a box thinner than the
 *            padding of the inverse direction, such as the box of an axis-aligned triangle under r = 0, can be skipped, because the
 *            padding moves a slab's exit outward only where t >= 0. What IS reported there is still a contact. Start the ray
 *            further back (tmin >= 0) where contacts behind the origin matter.
 * A query's record depends only on the tree, the primitives, the ray, its radius and ROBUST / ORIGINAL_IDS: not on batch size,
 * position or order, the reordering flags, the stream or the thread. d_counters (optional) receives {pair records fetched, primitives
 * tested, leaves visited}. Alignment: d_prims and d_rays 16 bytes, d_hits to the size of its record (16 / 32), d_counters 8, d_radii
 * to its scalar (4 / 8). 3D trees only; a 2D tree, a NULL handle, a NULL d_prims, d_rays or d_hits, a misaligned pointer and a tree
 * without a device copy are refused with BVH_AMD_ERR_ARG. Re-entrant on a const tree (no work slot of the tree is claimed).
 * Not offered: the 2D families, instanced scenes, swept capsules or boxes, a top-k variant. */
BVH_AMD_API int bvh3f_sphere_cast_tri(const struct bvh3f*, const float* d_tris12, const struct bvh_ray3f* d_rays, size_t n, float radius,
    const float* d_radii, unsigned flags, struct bvh_hit3f* d_hits, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3d_sphere_cast_tri(const struct bvh3d*, const double* d_tris12, const struct bvh_ray3d* d_rays, size_t n, double radius,
    const double* d_radii, unsigned flags, struct bvh_hit3d* d_hits, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3f_sphere_cast_sphere(const struct bvh3f*, const float* d_sph4, const struct bvh_ray3f* d_rays, size_t n, float radius,
    const float* d_radii, unsigned flags, struct bvh_hit3f* d_hits, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3d_sphere_cast_sphere(const struct bvh3d*, const double* d_sph4, const struct bvh_ray3d* d_rays, size_t n, double radius,
    const double* d_radii, unsigned flags, struct bvh_hit3d* d_hits, struct bvh_amd_counters* d_counters, void* stream);

/* ---- batched instanced ray queries: a two-level scene with transforms ---------------------------------------------------------- */
/* A scene is a table of geometries {tree, its BVH-order PrecomputedTri, as bvh3X_intersect_rays_tri takes them}, n_instances
 * instances {object-to-world matrix, geometry index}, and a top tree: an ordinary bvh3X built over the instances' world boxes,
 * whose prim ids are instance indices. Matrices are row-major 3 x 4 (12 scalars): x_world = M x_object + t, t in column 3.
 * d_geometry holds one uint32 per instance, or is NULL: every instance uses geometry 0.
 *
 * bvh3X_instance_prepare, one launch: per instance the world-to-object matrix (adjugate / determinant; a zero determinant or
 * anything non-finite DISABLES the instance: twelve NaNs), the world box of its geometry's root box {min.xyz, max.xyz}, widened so
 * that it is conservative under rounding (by at most 12 eps (sum_j |m_ij| max(|lo_j|, |hi_j|) + |t_i|) per axis), and that box's
 * centre — the arrays bvhXX_build_device and bvhXX_refit_boxes take. A disabled instance, or one whose geometry index is outside the
 * table, gets the zero-extent box at its translation (at the origin when that is not finite). The root boxes are read from the
 * geometries' resident nodes on the stream: a geometry refitted on it before the call is seen. Rigid motion therefore needs no
 * geometry rebuild: new matrices -> bvh3X_instance_prepare -> bvh3X_refit_boxes on the top tree -> trace.
 *
 * bvh3X_intersect_rays_instanced: per ray exactly the nesting of the single-level query. The top tree is walked as
 * Bvh::intersect<IsAnyHit, IsRobust> walks; at a top leaf its slots are taken in order; an instance that is enabled and whose
 * geometry index is inside the table gets the ray in its object space (org' = W org + w, dir' = W dir, tmin and the current tmax
 * unchanged; the direction is not normalised, so t means the same in both spaces; a -0 component may come out +0) and its tree is
 * walked from its root with the same rules and the triangle test of bvh3X_intersect_rays_tri. An accepted hit shortens tmax for
 * everything after it, in both levels; any-hit ends at the first geometry leaf that leaves a hit. d_hits[r] = {prim = BVH-order
 * index in the hit geometry's tree (its prim_ids[...] with BVH_AMD_RAY_ORIGINAL_IDS), t, u, v}, d_hit_instances[r] = the instance; a
 * miss is {BVH_AMD_INVALID, the ray's tmax, 0, 0} and instance BVH_AMD_INVALID. A ray whose tmin or tmax is NaN is a miss and counts
 * nothing. d_counters (optional) sums both levels: pair records fetched, triangles tested, leaves visited (a top leaf once).
 * flags: BVH_AMD_RAY_ANY_HIT, BVH_AMD_RAY_ROBUST, BVH_AMD_RAY_ORIGINAL_IDS, BVH_AMD_RAY_UNSORTED (what happens anyway: the batch is
 * never reordered); BVH_AMD_RAY_SORTED and any other bit: BVH_AMD_ERR_ARG. n_rays == 0 is a no-op. n_instances must exceed the
 * top tree's largest prim id (checked once per layout). Re-entrant on const trees (no work slot is claimed); the call synchronises
 * nothing (the first call on a layout measures the trees' depths). Not offered: spheres, the 2D families, more than two levels,
 * mixed scalar types, reordering of the batch.
 *
 * What "exactly the nesting of the single-level query" covers (tests/test_instanced_fuzz_host.py, tests/test_gpu_instanced_fuzz.py):
 * it holds bit for bit, counters included, where the order of the instances is fixed and no box of the top tree is tested (a top
 * tree of one leaf). Under a built top tree the order depends on the ray, and: with BVH_AMD_RAY_ROBUST every hit of the box-free
 * composition is kept, with its t byte for byte, on mirrored, squashed (kappa 1e3), 1e-4 / 1e4-scaled, far (+1e4), coincident and
 * disabled instances and on rays grazing the geometries' root boxes from 30 and 3000 units; without it (fast mode) the walk can only
 * LOSE hits to box culling, never invent or alter one. The loss is inherited: a direction component of magnitude <= eps gets the
 * inverse copysign(max, d), -inv * org then overflows for |org| > 1 and every top box fails: of 1021 axis-aligned rays on 12
 * instances that hit 870 times, 209 hits are left (all 870 under a one-leaf top tree); across the tests' scenes 7 to 18 % of all hits,
 * nearly all of them on axis-aligned rays. Use ROBUST for such rays. Against a float64 brute force over the world-space triangles
 * the robust walk agrees on hit or miss, instance and primitive wherever float rounding cannot decide (margin 1e-3). Its t is held
 * to 4 times the worst relative error that the reference's own single-level composition shows against that brute force on the same
 * rays, which measured 6.14e-6 (float) / 4.90e-14 (double), mirrored 2.92e-5 / 5.24e-14, at +1e4 3.89e-3 / 3.22e-11. The bvh_hit3d
 * record is stored whole, as bvh3d_intersect_rays_tri stores it: its padding word is written as 0. */
struct bvh_amd_geometry3f { const struct bvh3f* bvh; const float* d_tris12; };
struct bvh_amd_geometry3d { const struct bvh3d* bvh; const double* d_tris12; };
BVH_AMD_API int bvh3f_instance_prepare(const struct bvh_amd_geometry3f* geoms, size_t n_geoms, const float* d_obj2world12, const uint32_t* d_geometry,
    size_t n_instances, float* d_world2obj12, float* d_bboxes, float* d_centers, void* stream);
BVH_AMD_API int bvh3d_instance_prepare(const struct bvh_amd_geometry3d* geoms, size_t n_geoms, const double* d_obj2world12, const uint32_t* d_geometry,
    size_t n_instances, double* d_world2obj12, double* d_bboxes, double* d_centers, void* stream);
BVH_AMD_API int bvh3f_intersect_rays_instanced(const struct bvh3f* top, const struct bvh_amd_geometry3f* geoms, size_t n_geoms,
    const float* d_world2obj12, const uint32_t* d_geometry, size_t n_instances, const struct bvh_ray3f* d_rays, size_t n_rays, unsigned flags,
    struct bvh_hit3f* d_hits, uint32_t* d_hit_instances, struct bvh_amd_counters* d_counters, void* stream);
BVH_AMD_API int bvh3d_intersect_rays_instanced(const struct bvh3d* top, const struct bvh_amd_geometry3d* geoms, size_t n_geoms,
    const double* d_world2obj12, const uint32_t* d_geometry, size_t n_instances, const struct bvh_ray3d* d_rays, size_t n_rays, unsigned flags,
    struct bvh_hit3d* d_hits, uint32_t* d_hit_instances, struct bvh_amd_counters* d_counters, void* stream);

/* Optional, additive: pays NOW what the first large batch through a fresh tree would pay inside its own call — the tree's depth /
 * expected-visits pass (one read-back) and the first allocation of the ray-reordering scratch for batches of `n_rays_hint` rays (kept
 * in the library's block cache for that stream). A single Bvh::intersect on a fresh Bvh is the reference's normal use (bvh.h:160-182);
 * a batch that comes unprepared does the same work itself. */
BVH_AMD_API int bvh3f_prepare_trace(const struct bvh3f*, size_t n_rays_hint, void* stream);
BVH_AMD_API int bvh3d_prepare_trace(const struct bvh3d*, size_t n_rays_hint, void* stream);

/* ---- building blocks exposed for unit tests (order-defining sorts) ----------------------- */
/* d_ids_out[0..n) = the permutation libstdc++ 11's std::sort(iota, [&](i,j){ return keys[i] < keys[j]; }) produces,
 * including the arrangement of equal keys (sweep_sah_builder.h:57-63 depends on it). */
BVH_AMD_API int bvh_amd_std_sort_ids3f(const float* d_keys, size_t n, uint32_t* d_ids_out, void* stream);
BVH_AMD_API int bvh_amd_std_sort_ids3d(const double* d_keys, size_t n, uint32_t* d_ids_out, void* stream);
/* stable LSD radix sort of (key, value) pairs by the low `bits` bits of the key, in place */
BVH_AMD_API int bvh_amd_radix_sort_pairs_u32(uint32_t* d_keys, uint32_t* d_vals, size_t n, int bits, void* stream);
/* d_order_out[0..n) = the stable order of n < 2^31 keys by their low `bits` bits (1..32), through exactly what a reordered ray or
 * query batch runs: the first histogram by the key kernel, positions as values, keys narrowed between passes and dropped. */
BVH_AMD_API int bvh_amd_radix_order_u32(const uint32_t* d_keys, size_t n, int bits, uint32_t* d_order_out, void* stream);

/* Name and average duration source for profiling: the kernel symbol the last intersect call used. */
BVH_AMD_API const char* bvh_amd_last_kernel_name(void);
/* 1 when the calling thread's latest 3D batch traversal reordered its rays internally (BVH_AMD_RAY_SORTED, or the default rule). */
BVH_AMD_API int bvh_amd_last_launch_reordered(void);
/* The number of walk-kernel launches the calling thread's latest point, box or instanced ray query made: 1, or one per slice of a
 * batch over a tree deeper than 64 levels that was cut to bound the stack spill. 0 before the first such query. A call that is
 * refused by its argument checks or has an empty batch leaves the value as it was; a call that fails after them (an allocation, a
 * launch) leaves the number of launches it made before it failed, 0 if none. */
BVH_AMD_API int bvh_amd_last_query_launches(void);
/* Measurement aid: with timing on, every batch traversal launched by the calling thread records a pair of events on its stream
 * around the traversal kernel alone (not the optional ray reordering in front of it). bvh_amd_kernel_times waits for and returns
 * the durations (ms) of the latest min(capacity, 256) launches since timing was switched on, oldest first. */
BVH_AMD_API void bvh_amd_kernel_timing(int on);
BVH_AMD_API int bvh_amd_kernel_times(float* ms_out, size_t capacity, size_t* count_out);
/* The same launches: milliseconds from the start of the call on its stream to the start of the traversal kernel = ray keys +
 * radix sort of the optional reordering (0 for a batch traced as given). */
BVH_AMD_API int bvh_amd_reorder_times(float* ms_out, size_t capacity, size_t* count_out);
/* Developer knob for A/B runs inside one process: overrides, for the calling thread's following batch launches, the refill /
 * leaf-parking thresholds of the persistent waves (lanes idle before a wave draws new rays / lanes waiting at a leaf before the
 * leaf code runs), the record fetch of the float 3D kernels (0 per lane, 1 quad-cooperative) and the number of ticket ranges a launch
 * is cut into (1..256; default one per XCD). < 0 restores the default. Results never depend on any of them. */
BVH_AMD_API void bvh_amd_tuning(int refill_threshold, int leaf_threshold, int coop_fetch, int ticket_ranges);
/* Developer experiments of the calling thread, for A/B runs inside one process (tools/r04_experiments.py); results never change.
 * name: "grid_blocks" (cap of the persistent grid), "stream_hints" (1: rays / order / hit records loaded and stored non-temporally),
 * "tri_stride" (floats between PrecomputedTri records of the caller's array: 12, or 16 = padded to a 64-byte line), "key_curve"
 * (0 Morton, 1 Hilbert order of the reordering key), "key_bits" (bits per axis of its grid, 1..8), "step_events" (events the device
 * logs per launch of the per-ray callback walk: a short log makes the tests continue a walk from the device's stack); value < 0 = the default;
 * "one_shot" (1 / 0: force / forbid the one-shot grid of batches of up to 2^18 rays), "stagger" (tickets per eighth of the persistent grid
 * of the staggered drain; 0 = off), "key_class_bits" / "key_class_scale" (chord classes of the reordering key: long rays first),
 * "key_tail" / "key_tail_permille" (0 / 1: the tail class of the one-bit key, and its threshold in 1/1000 diagonals of the root box; 0 =
 * only rays with no chord through it), "range_align" (0: the ticket ranges of a reordered launch are equal slices, not one key prefix each);
 * "reset" clears all of them. Returns BVH_AMD_ERR_ARG for an unknown name.                                                       */
BVH_AMD_API int bvh_amd_experiment(const char* name, int value);
/* Developer library only (libbvh_amd_dev.so; the release library returns BVH_AMD_ERR_ARG and its kernels carry no such code): after
 * bvh_amd_experiment("wave_times", 1), every batch launch of the calling thread records, per wavefront of the persistent grid, six
 * 64-bit words {begin, last ticket draw, end} in s_memrealtime ticks (100 MHz), {XCC id << 32 | rays traced}, {ticks spent inside
 * refills (ticket atomic -> order -> ray loads arrived), number of refills}; this copies the latest
 * launch's records out (it waits for the device). The drain-tail study of profiles/r05_tail_timeline_before.txt / _after.txt (tools/tail_timeline.py). */
BVH_AMD_API int bvh_amd_wave_times(unsigned long long* out, size_t capacity_waves, size_t* n_waves);
/* How the calling thread's latest batch launch was traced: out = {0 as given / 1 reordered / 2 reordered with the long rays first,
 * record fetch 0 per lane / 1 quad-cooperative, refill threshold, leaf threshold}. For 3D trees whose traversal records exceed the
 * 32 MB of L2 and batches of >= 2^20 rays the library MEASURES this once per tree and kind of ray (closest / any-hit): the first such
 * batch is traced with the plan a static predictor gives the tree, the following ones with the other candidate plans — {as given,
 * reordered} x {per-lane, cooperative fetch} and, closest-hit, reordered with the long rays first — one WHOLE batch each, timed by
 * events on the launch stream (csrc/traverse.hip: launch_traverse); a candidate that loses clearly is not traced again, survivors are
 * measured twice (3 to 8 batches in all), and the fastest is kept until the tree is re-laid out. Smaller trees and batches use the
 * predictor. BVH_AMD_CALIBRATE=0 in the environment keeps the predictor everywhere. */
BVH_AMD_API void bvh_amd_last_launch_plan(int out[4]);
/* The table of the latest plan search the calling thread FINISHED (the call that settled a tree's plan): nanoseconds per ray of the five
 * candidates {0 as given + per lane, 1 as given + cooperative, 2 reordered + per lane (any-hit: as given + cooperative, heavy thresholds),
 * 3 reordered + cooperative, 4 reordered + cooperative + long rays first (closest-hit only)} — the better of a candidate's measurements,
 * the keys + sort of a reordering candidate charged at their measured rate —, how often each was measured (0: pruned before its turn)
 * and the mask of candidates dropped as clear losers. Measurement aid: bench.py quotes it in `roofline.launch_plan.search`. */
BVH_AMD_API void bvh_amd_last_plan_search(float ns_per_ray[5], int measurements[5], unsigned* dropped_mask);
/* ReinsertionOptimizer iterations run so far in this process: out[0] = through the heap-free fast path, out[1] = through the
 * exact replay of the reference's candidate heap + std::sort (taken when ties make their layout matter).
 * Both produce the reference's result bit for bit; BVH_AMD_REINSERT=exact in the environment forces the replay. */
BVH_AMD_API void bvh_amd_reinsertion_stats(unsigned out[2]);
/* The calling thread's latest ReinsertionOptimizer run (bvhXX_optimize*, or the optimize step of a Quality::High build;
 * reinsertion_optimizer.h:237-267): iterations run, how many of them had to replay the libstdc++ candidate heap of
 * find_candidates exactly (:88-105) instead of the heap-free fast path, the pop_heap + push_heap replacements those replays
 * made, and the GPU time of the heap kernels. */
struct bvh_amd_optimize_profile { unsigned iterations, replayed; unsigned long long replacements; float heap_ms; };
BVH_AMD_API void bvh_amd_last_optimize_profile(struct bvh_amd_optimize_profile* out);


/* ---- one ray, leaves intersected by a HOST callback (c_api/bvh.h:277-295; bvh_impl.h:235-250) --------------------------------
 * Bvh::intersect<IsAnyHit, IsRobust>(ray, root, SmallStack<Index, 64>, leaf_fn): the walk runs on the device and logs the
 * leaves it reaches; the callback is invoked on the calling thread, in the reference's order, with &ray.tmax. Whenever
 * the callback changes tmax the walk restarts from that leaf with the shortened ray, so culling is the reference's.
 * Re-entrant (per-thread stream and buffers). Cost: one or more kernel launches per ray; use the *_intersect_rays_* family for
 * throughput. These return void like the reference's; a device failure aborts with a message instead of reporting "no hit". */
BVH_AMD_API void bvh3f_intersect_ray(const struct bvh3f*, const struct bvh_ray3f*, const struct bvh_intersect_callbackf*);
BVH_AMD_API void bvh3d_intersect_ray(const struct bvh3d*, const struct bvh_ray3d*, const struct bvh_intersect_callbackd*);
BVH_AMD_API void bvh3f_intersect_ray_any(const struct bvh3f*, const struct bvh_ray3f*, const struct bvh_intersect_callbackf*);
BVH_AMD_API void bvh3d_intersect_ray_any(const struct bvh3d*, const struct bvh_ray3d*, const struct bvh_intersect_callbackd*);
BVH_AMD_API void bvh3f_intersect_ray_robust(const struct bvh3f*, const struct bvh_ray3f*, const struct bvh_intersect_callbackf*);
BVH_AMD_API void bvh3d_intersect_ray_robust(const struct bvh3d*, const struct bvh_ray3d*, const struct bvh_intersect_callbackd*);
BVH_AMD_API void bvh3f_intersect_ray_any_robust(const struct bvh3f*, const struct bvh_ray3f*, const struct bvh_intersect_callbackf*);
BVH_AMD_API void bvh3d_intersect_ray_any_robust(const struct bvh3d*, const struct bvh_ray3d*, const struct bvh_intersect_callbackd*);
/* Additive: start at any node (`start_index` = the packed index word of Bvh::intersect's `start`, i.e. first_id << 4 |
 * prim_count; BVH_AMD_START_AT_ROOT = the root's), optional inner callback, error code instead of abort. */
#define BVH_AMD_START_AT_ROOT SIZE_MAX
BVH_AMD_API int bvh3f_intersect_ray_visit(const struct bvh3f*, const struct bvh_ray3f*, size_t start_index, unsigned flags,
    const struct bvh_amd_ray_visitorf*);
BVH_AMD_API int bvh3d_intersect_ray_visit(const struct bvh3d*, const struct bvh_ray3d*, size_t start_index, unsigned flags,
    const struct bvh_amd_ray_visitord*);

/* ---- the 2D families `2f` / `2d` (c_api/bvh.cpp:7-10: Bvh<Node<T, 2>>) ---------------------------------------------------
 * Same contracts as the 3D functions above with bvh_bbox2X / bvh_vec2X / bvh_ray2X and 20/40-byte nodes
 * ({minx,maxx,miny,maxy}, index). Builders: serial DefaultBuilder (Low = binned SAH, Medium = sweep SAH, High = sweep +
 * reinsertion), bit-identical with the reference; with a thread pool the reference runs the serial builder below
 * parallel_threshold (default_builder.h:38-39) and so does this library, while AT OR ABOVE the threshold its mini-tree
 * builder reads the third component of 2D points (mini_tree_builder.h:183: undefined behaviour), which is refused here
 * (NULL + bvh_amd_last_error()). Leaf primitive of the batch traversal: circles = Sphere<T, 2> {center.x, center.y, radius}
 * (sphere.h:15-50; tri.h has no 2D intersector). */
BVH_AMD_API struct bvh2f* bvh2f_build(struct bvh_thread_pool*, const struct bvh_bbox2f* bboxes,
    const struct bvh_vec2f* centers, size_t prim_count, const struct bvh_build_config* config);   /* c_api/bvh.h:99-125 */
BVH_AMD_API struct bvh2f* bvh2f_build_device(const float* d_bboxes4, const float* d_centers2, size_t prim_count,
    const struct bvh_build_config* config, enum bvh_amd_builder builder, void* stream);
BVH_AMD_API struct bvh2f* bvh2f_build_sah(struct bvh_thread_pool*, const struct bvh_bbox2f* bboxes, const struct bvh_vec2f* centers,
    size_t prim_count, const struct bvh_build_config* config, const struct bvh_amd_sah_config* sah);
BVH_AMD_API struct bvh2f* bvh2f_build_device_sah(const float* d_bboxes4, const float* d_centers2, size_t prim_count,
    const struct bvh_build_config* config, enum bvh_amd_builder builder, const struct bvh_amd_sah_config* sah, void* stream);
BVH_AMD_API struct bvh2f* bvh2f_build_device_binned(const float* d_bboxes4, const float* d_centers2, size_t prim_count,
    const struct bvh_build_config* config, const struct bvh_amd_sah_config* sah, size_t bin_count, void* stream);
BVH_AMD_API struct bvh2f* bvh2f_from_nodes(const void* nodes, size_t node_count, const size_t* prim_ids, size_t prim_count);
BVH_AMD_API struct bvh2f* bvh2f_extract(struct bvh2f* bvh, size_t root_id);
BVH_AMD_API void bvh2f_destroy(struct bvh2f*);
BVH_AMD_API void bvh2f_optimize(struct bvh_thread_pool*, struct bvh2f*);
BVH_AMD_API int bvh2f_optimize_config(struct bvh2f*, const struct bvh_amd_optimize_config*);
BVH_AMD_API void bvh2f_refit(struct bvh2f*);
BVH_AMD_API int bvh2f_refit_status(struct bvh2f*);
BVH_AMD_API int bvh2f_refit_boxes(struct bvh2f*, const float* d_bboxes4, size_t n_boxes, void* stream);     /* see bvh3f_refit_boxes */
BVH_AMD_API int bvh2f_sync_device(struct bvh2f*);
BVH_AMD_API void bvh2f_append_node(struct bvh2f*);
BVH_AMD_API void bvh2f_remove_last_node(struct bvh2f*);
BVH_AMD_API void bvh_node2f_set_prim_count(struct bvh_node2f*, size_t);
BVH_AMD_API void bvh_node2f_set_first_id(struct bvh_node2f*, size_t);
BVH_AMD_API void bvh_node2f_set_bbox(struct bvh_node2f*, const struct bvh_bbox2f*);
BVH_AMD_API void bvh2f_save(const struct bvh2f*, FILE*);
BVH_AMD_API struct bvh2f* bvh2f_load(FILE*);
BVH_AMD_API size_t bvh2f_serialize(const struct bvh2f*, void* out, size_t capacity);
BVH_AMD_API struct bvh2f* bvh2f_deserialize(const void* bytes, size_t size);
BVH_AMD_API size_t bvh2f_serialize_device(struct bvh2f*, void* d_out, size_t cap, void* stream);
BVH_AMD_API struct bvh2f* bvh2f_deserialize_device(const void* d_bytes, size_t size, void* stream);
BVH_AMD_API struct bvh_node2f* bvh2f_get_node(struct bvh2f*, size_t);
BVH_AMD_API size_t bvh2f_get_prim_id(const struct bvh2f*, size_t);
BVH_AMD_API size_t bvh2f_get_prim_count(const struct bvh2f*);
BVH_AMD_API size_t bvh2f_get_node_count(const struct bvh2f*);
BVH_AMD_API bool bvh_node2f_is_leaf(const struct bvh_node2f*);
BVH_AMD_API size_t bvh_node2f_get_prim_count(const struct bvh_node2f*);
BVH_AMD_API size_t bvh_node2f_get_first_id(const struct bvh_node2f*);
BVH_AMD_API struct bvh_bbox2f bvh_node2f_get_bbox(const struct bvh_node2f*);
BVH_AMD_API void bvh2f_copy_nodes(const struct bvh2f*, void* out);
BVH_AMD_API void bvh2f_copy_prim_ids(const struct bvh2f*, size_t* out);
BVH_AMD_API const uint32_t* bvh2f_device_prim_ids(const struct bvh2f*);
/* circles3: n x {center.x, center.y, radius} -> bboxes n x {min.x,min.y,max.x,max.y}, centers n x 2 (sphere.h:24-27) */
BVH_AMD_API int bvh_amd_sphere_bounds2f(const float* d_circles3, size_t n, float* d_bboxes4, float* d_centers2, void* stream);
/* d_circles3 in BVH order; hit = {prim, t0, t1, 0} like the 3D sphere traversal */
BVH_AMD_API int bvh2f_intersect_rays_sphere(const struct bvh2f* bvh, const float* d_circles3, const struct bvh_ray2f* d_rays,
    size_t n, unsigned flags, struct bvh_hit3f* d_hits, struct bvh_amd_counters* d_counters, void* stream);

BVH_AMD_API struct bvh2d* bvh2d_build(struct bvh_thread_pool*, const struct bvh_bbox2d* bboxes,
    const struct bvh_vec2d* centers, size_t prim_count, const struct bvh_build_config* config);   /* c_api/bvh.h:99-125 */
BVH_AMD_API struct bvh2d* bvh2d_build_device(const double* d_bboxes4, const double* d_centers2, size_t prim_count,
    const struct bvh_build_config* config, enum bvh_amd_builder builder, void* stream);
BVH_AMD_API struct bvh2d* bvh2d_build_sah(struct bvh_thread_pool*, const struct bvh_bbox2d* bboxes, const struct bvh_vec2d* centers,
    size_t prim_count, const struct bvh_build_config* config, const struct bvh_amd_sah_config* sah);
BVH_AMD_API struct bvh2d* bvh2d_build_device_sah(const double* d_bboxes4, const double* d_centers2, size_t prim_count,
    const struct bvh_build_config* config, enum bvh_amd_builder builder, const struct bvh_amd_sah_config* sah, void* stream);
BVH_AMD_API struct bvh2d* bvh2d_build_device_binned(const double* d_bboxes4, const double* d_centers2, size_t prim_count,
    const struct bvh_build_config* config, const struct bvh_amd_sah_config* sah, size_t bin_count, void* stream);
BVH_AMD_API struct bvh2d* bvh2d_from_nodes(const void* nodes, size_t node_count, const size_t* prim_ids, size_t prim_count);
BVH_AMD_API struct bvh2d* bvh2d_extract(struct bvh2d* bvh, size_t root_id);
BVH_AMD_API void bvh2d_destroy(struct bvh2d*);
BVH_AMD_API void bvh2d_optimize(struct bvh_thread_pool*, struct bvh2d*);
BVH_AMD_API int bvh2d_optimize_config(struct bvh2d*, const struct bvh_amd_optimize_config*);
BVH_AMD_API void bvh2d_refit(struct bvh2d*);
BVH_AMD_API int bvh2d_refit_status(struct bvh2d*);
BVH_AMD_API int bvh2d_refit_boxes(struct bvh2d*, const double* d_bboxes4, size_t n_boxes, void* stream);
BVH_AMD_API int bvh2d_sync_device(struct bvh2d*);
BVH_AMD_API void bvh2d_append_node(struct bvh2d*);
BVH_AMD_API void bvh2d_remove_last_node(struct bvh2d*);
BVH_AMD_API void bvh_node2d_set_prim_count(struct bvh_node2d*, size_t);
BVH_AMD_API void bvh_node2d_set_first_id(struct bvh_node2d*, size_t);
BVH_AMD_API void bvh_node2d_set_bbox(struct bvh_node2d*, const struct bvh_bbox2d*);
BVH_AMD_API void bvh2d_save(const struct bvh2d*, FILE*);
BVH_AMD_API struct bvh2d* bvh2d_load(FILE*);
BVH_AMD_API size_t bvh2d_serialize(const struct bvh2d*, void* out, size_t capacity);
BVH_AMD_API struct bvh2d* bvh2d_deserialize(const void* bytes, size_t size);
BVH_AMD_API size_t bvh2d_serialize_device(struct bvh2d*, void* d_out, size_t cap, void* stream);
BVH_AMD_API struct bvh2d* bvh2d_deserialize_device(const void* d_bytes, size_t size, void* stream);
BVH_AMD_API struct bvh_node2d* bvh2d_get_node(struct bvh2d*, size_t);
BVH_AMD_API size_t bvh2d_get_prim_id(const struct bvh2d*, size_t);
BVH_AMD_API size_t bvh2d_get_prim_count(const struct bvh2d*);
BVH_AMD_API size_t bvh2d_get_node_count(const struct bvh2d*);
BVH_AMD_API bool bvh_node2d_is_leaf(const struct bvh_node2d*);
BVH_AMD_API size_t bvh_node2d_get_prim_count(const struct bvh_node2d*);
BVH_AMD_API size_t bvh_node2d_get_first_id(const struct bvh_node2d*);
BVH_AMD_API struct bvh_bbox2d bvh_node2d_get_bbox(const struct bvh_node2d*);
BVH_AMD_API void bvh2d_copy_nodes(const struct bvh2d*, void* out);
BVH_AMD_API void bvh2d_copy_prim_ids(const struct bvh2d*, size_t* out);
BVH_AMD_API const uint32_t* bvh2d_device_prim_ids(const struct bvh2d*);
/* circles3: n x {center.x, center.y, radius} -> bboxes n x {min.x,min.y,max.x,max.y}, centers n x 2 (sphere.h:24-27) */
BVH_AMD_API int bvh_amd_sphere_bounds2d(const double* d_circles3, size_t n, double* d_bboxes4, double* d_centers2, void* stream);
/* d_circles3 in BVH order; hit = {prim, t0, t1, 0} like the 3D sphere traversal */
BVH_AMD_API int bvh2d_intersect_rays_sphere(const struct bvh2d* bvh, const double* d_circles3, const struct bvh_ray2d* d_rays,
    size_t n, unsigned flags, struct bvh_hit3d* d_hits, struct bvh_amd_counters* d_counters, void* stream);

/* c_api/bvh.h:277-295, 2D */
BVH_AMD_API void bvh2f_intersect_ray(const struct bvh2f*, const struct bvh_ray2f*, const struct bvh_intersect_callbackf*);
BVH_AMD_API void bvh2d_intersect_ray(const struct bvh2d*, const struct bvh_ray2d*, const struct bvh_intersect_callbackd*);
BVH_AMD_API void bvh2f_intersect_ray_any(const struct bvh2f*, const struct bvh_ray2f*, const struct bvh_intersect_callbackf*);
BVH_AMD_API void bvh2d_intersect_ray_any(const struct bvh2d*, const struct bvh_ray2d*, const struct bvh_intersect_callbackd*);
BVH_AMD_API void bvh2f_intersect_ray_robust(const struct bvh2f*, const struct bvh_ray2f*, const struct bvh_intersect_callbackf*);
BVH_AMD_API void bvh2d_intersect_ray_robust(const struct bvh2d*, const struct bvh_ray2d*, const struct bvh_intersect_callbackd*);
BVH_AMD_API void bvh2f_intersect_ray_any_robust(const struct bvh2f*, const struct bvh_ray2f*, const struct bvh_intersect_callbackf*);
BVH_AMD_API void bvh2d_intersect_ray_any_robust(const struct bvh2d*, const struct bvh_ray2d*, const struct bvh_intersect_callbackd*);
BVH_AMD_API int bvh2f_intersect_ray_visit(const struct bvh2f*, const struct bvh_ray2f*, size_t start_index, unsigned flags,
    const struct bvh_amd_ray_visitorf*);
BVH_AMD_API int bvh2d_intersect_ray_visit(const struct bvh2d*, const struct bvh_ray2d*, size_t start_index, unsigned flags,
    const struct bvh_amd_ray_visitord*);
/* multi-GPU for the 2D families: see bvh3f_broadcast / bvh3f_replicate */
BVH_AMD_API struct bvh2f* bvh2f_broadcast(struct bvh_amd_comm*, int root, struct bvh2f* bvh, const void* d_prims, size_t prim_bytes,
                                          void** d_prims_out, size_t* prim_bytes_out, void* stream);
BVH_AMD_API struct bvh2d* bvh2d_broadcast(struct bvh_amd_comm*, int root, struct bvh2d* bvh, const void* d_prims, size_t prim_bytes,
                                          void** d_prims_out, size_t* prim_bytes_out, void* stream);
BVH_AMD_API int bvh2f_replicate(struct bvh2f* bvh, const void* d_prims, size_t prim_bytes, int n_devices, const int* devices,
                                struct bvh2f** bvhs_out, void** d_prims_out);
BVH_AMD_API int bvh2d_replicate(struct bvh2d* bvh, const void* d_prims, size_t prim_bytes, int n_devices, const int* devices,
                                struct bvh2d** bvhs_out, void** d_prims_out);

#ifdef __cplusplus
}
#endif

#endif
