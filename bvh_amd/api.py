"""Host-side mirror of the reference interface (bvh::v2) over the C-ABI. torch = device memory + streams."""
from __future__ import annotations

import ctypes as C
import enum
from dataclasses import dataclass, field

import numpy as np

from . import _lib

INVALID = 0xFFFFFFFF
HITF = np.dtype([("prim", "<u4"), ("t", "<f4"), ("u", "<f4"), ("v", "<f4")])
HITD = np.dtype([("prim", "<u4"), ("pad", "<u4"), ("t", "<f8"), ("u", "<f8"), ("v", "<f8")])
NODEF = np.dtype([("bounds", "<f4", (6,)), ("index", "<u4")])     # reference node.h:31-37
NODED = np.dtype([("bounds", "<f8", (6,)), ("index", "<u8")])
NODE2F = np.dtype([("bounds", "<f4", (4,)), ("index", "<u4")])    # Node<float, 2>: {minx,maxx,miny,maxy}, index
NODE2D = np.dtype([("bounds", "<f8", (4,)), ("index", "<u8")])
_NODE_DTYPES = {"3f": NODEF, "3d": NODED, "2f": NODE2F, "2d": NODE2D}


class Quality(enum.IntEnum):          # default_builder.h:21
    Low = 0
    Medium = 1
    High = 2


class RayFlags(enum.IntFlag):
    ANY_HIT = 1
    ROBUST = 2
    SORTED = 4
    UNSORTED = 16


class _Builder(enum.IntEnum):
    DEFAULT_SERIAL = 0
    DEFAULT_PARALLEL = 1
    BINNED = 2
    SWEEP = 3


@dataclass
class SplitHeuristic:                 # split_heuristic.h:17-23: SplitHeuristic(log_cluster_size = 0, cost_ratio = 1)
    log_cluster_size: int = 0
    cost_ratio: float = 1.0

    def _c(self):
        return _lib.SahConfig(int(self.log_cluster_size), float(self.cost_ratio))


@dataclass
class Config:                         # default_builder.h:23-30 + top_down_sah_builder.h:27-40
    quality: Quality = Quality.High
    min_leaf_size: int = 1
    max_leaf_size: int = 8
    parallel_threshold: int = 1024
    sah: SplitHeuristic = field(default_factory=SplitHeuristic)

    def _c(self):
        return _lib.BuildConfig(int(self.quality), self.min_leaf_size, self.max_leaf_size, self.parallel_threshold)


class ThreadPool:
    """bvh::v2::ThreadPool stand-in (thread_pool.h:13-46). The GPU grid replaces the pool; passing one
    selects the reference's parallel (mini-tree) builder semantics exactly like the reference API."""

    def __init__(self, thread_count: int = 0):
        self.thread_count = thread_count


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise _lib.BvhAmdError("no HIP device visible to torch: bvh_amd has no CPU path")
    return torch


def _suffix(dtype, dim: int = 3) -> str:
    import torch
    if dim not in (2, 3):
        raise ValueError("BVHs are 2- or 3-dimensional")
    if dtype in (torch.float32, np.float32, np.dtype(np.float32)):
        return f"{dim}f"
    if dtype in (torch.float64, np.float64, np.dtype(np.float64)):
        return f"{dim}d"
    raise TypeError(f"unsupported scalar type {dtype}")


def _dev(x, cols=None):
    """numpy / torch (any device) -> contiguous torch tensor on the current HIP device."""
    torch = _torch()
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not x.is_cuda:
        x = x.cuda()
    x = x.contiguous()
    if cols is not None:
        x = x.reshape(-1, cols)
    return x


def _stream():
    return C.c_void_p(_torch().cuda.current_stream().cuda_stream)


class Bvh:
    """bvh::v2::Bvh<Node<T,3>> or Bvh<Node<T,2>> (bvh.h:17-89): host mirror in the reference layout + device-resident copy."""

    def __init__(self, handle, suffix: str):
        if not handle:
            raise _lib.BvhAmdError(_lib.last_error())
        self._h, self._s = handle, suffix
        self._lib = _lib.load()

    def __del__(self):
        if getattr(self, "_h", None):
            getattr(self._lib, f"bvh{self._s}_destroy")(self._h)
            self._h = None

    def _f(self, name):
        return getattr(self._lib, name.format(S=self._s))

    @property
    def dtype(self):
        return np.float32 if self._s[1] == "f" else np.float64

    @property
    def dim(self) -> int:
        return int(self._s[0])

    @property
    def node_count(self) -> int:
        return self._f("bvh{S}_get_node_count")(self._h)

    @property
    def prim_count(self) -> int:
        return self._f("bvh{S}_get_prim_count")(self._h)

    @property
    def nodes(self) -> np.ndarray:
        out = np.empty(self.node_count, dtype=_NODE_DTYPES[self._s])
        self._f("bvh{S}_copy_nodes")(self._h, out.ctypes.data_as(C.c_void_p))
        return out

    @property
    def prim_ids(self) -> np.ndarray:
        out = np.empty(self.prim_count, dtype=np.uint64)
        self._f("bvh{S}_copy_prim_ids")(self._h, out.ctypes.data_as(C.c_void_p))
        return out

    def device_prim_ids(self):
        """uint32 prim ids resident in HBM, as a torch tensor view (no copy)."""
        torch = _torch()
        ptr = self._f("bvh{S}_device_prim_ids")(self._h)
        n = self.prim_count

        class _Holder:
            __cuda_array_interface__ = {"shape": (n,), "typestr": "<i4", "data": (ptr, False), "version": 2}
        t = torch.as_tensor(_Holder(), device="cuda")
        t._bvh_keepalive = self
        return t

    def optimize(self, thread_pool=None, batch_size_ratio=None, max_iter_count=None):
        """ReinsertionOptimizer::optimize (reinsertion_optimizer.h:27-35), in place on the device; the two keyword arguments are
        its Config (:18-24, defaults 0.05 and 3)."""
        _torch()
        if batch_size_ratio is not None or max_iter_count is not None:
            cfg = _lib.OptimizeConfig(0.05 if batch_size_ratio is None else float(batch_size_ratio),
                                      3 if max_iter_count is None else int(max_iter_count))
            _lib.check(self._f("bvh{S}_optimize_config")(self._h, C.byref(cfg)), "optimize")
            return
        _lib.check(self._f("bvh{S}_optimize_config")(self._h, None), "optimize")      # NULL config = the reference's defaults

    def refit(self):
        """Bvh::refit (bvh.h:211-218) on the device; pushes host-side node edits first."""
        _torch()
        _lib.check(self._f("bvh{S}_refit_status")(self._h), "refit")

    def _prims_in(self, x, cols, what):
        torch = _torch()
        if not hasattr(x, "dtype"):
            x = np.asarray(x)
        dt = x.dtype
        want = torch.float32 if self._s[1] == "f" else torch.float64
        if dt not in (want, np.dtype(self.dtype), self.dtype):
            raise TypeError(f"{what}: the tree is {np.dtype(self.dtype).name}, the array is {dt}")
        return _dev(x, cols)

    def refit_boxes(self, bboxes):
        """Leaf boxes from `bboxes` ((n, 2 dim) {min, max}, indexed by ORIGINAL primitive id, numpy or torch), inner boxes bottom-up;
        nodes and traversal records updated in place on the current torch stream, no host copy (bvhXX_refit_boxes)."""
        bb = self._prims_in(bboxes, 2 * self.dim, "refit_boxes")
        _lib.check(self._f("bvh{S}_refit_boxes")(self._h, bb.data_ptr(), bb.shape[0], _stream()), "refit_boxes")

    def refit_tris(self, tris9, out=None):
        """refit_boxes with Tri::get_bbox of (n, 9) triangles in original order, and the BVH-order PrecomputedTri array ((prim_count, 12),
        written into `out` if given) that intersect / closest_points take: deformed vertices to a traceable pair in one call."""
        torch = _torch()
        if self.dim != 3:
            raise TypeError("refit_tris: triangles are 3D (tri.h)")
        t = self._prims_in(tris9, 9, "refit_tris")
        if out is None:
            out = torch.empty((self.prim_count, 12), dtype=t.dtype, device=t.device)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.is_contiguous() and out.dtype == t.dtype and out.numel() == 12 * self.prim_count):
            raise TypeError("refit_tris: `out` must be a contiguous (prim_count, 12) device tensor of the tree's scalar type")
        _lib.check(self._f("bvh{S}_refit_tris")(self._h, t.data_ptr(), t.shape[0], out.data_ptr(), _stream()), "refit_tris")
        return out.reshape(-1, 12)

    def traversal_cost(self) -> float:
        """Traversal records a random line through the scene is expected to fetch, from the current boxes (bvh3X_traversal_cost): grows
        as a refitted tree degrades. Synchronises the current stream."""
        _torch()
        if self.dim != 3:
            raise TypeError("traversal_cost: 3D trees only")
        cost = C.c_double(0.0)
        _lib.check(self._f("bvh{S}_traversal_cost")(self._h, C.byref(cost), _stream()), "traversal_cost")
        return float(cost.value)

    def set_node_bbox(self, node_id: int, lo, hi):
        """bvh_nodeXX_set_bbox on the host mirror (takes effect on the device at the next refit()/sync_device())."""
        node = self._f("bvh{S}_get_node")(self._h, node_id)
        ct = C.c_float if self._s[1] == "f" else C.c_double
        bb = (ct * (2 * self.dim))(*[float(v) for v in list(lo) + list(hi)])
        self._f("bvh_node{S}_set_bbox")(node, bb)

    def sync_device(self):
        _lib.check(self._f("bvh{S}_sync_device")(self._h), "sync_device")

    def sync_host(self):
        """Fills the host mirror (reference-layout nodes + prim ids) from the device now instead of at the first accessor: the
        device-to-host copy that turns a device-resident build into the reference's host `Bvh` (what bvhXX_get_node does first)."""
        if not self._f("bvh{S}_get_node")(self._h, 0):
            raise _lib.BvhAmdError(_lib.last_error())

    def get_root(self):
        return self.nodes[0]

    def serialize(self) -> bytes:                     # bvh.h:221-229
        n = self._f("bvh{S}_serialize")(self._h, None, 0)
        buf = C.create_string_buffer(n)
        self._f("bvh{S}_serialize")(self._h, buf, n)
        return buf.raw

    @staticmethod
    def deserialize(data: bytes, dtype=np.float32, dim: int = 3) -> "Bvh":   # bvh.h:231-243
        s = _suffix(np.dtype(dtype), dim)
        lib = _lib.load()
        _torch()
        return Bvh(getattr(lib, f"bvh{s}_deserialize")(data, len(data)), s)

    def serialize_device(self):
        """Bvh::serialize (bvh.h:221-229) into HBM: a uint8 torch tensor holding the reference's byte stream, written from the
        resident nodes on the current stream (no host copy). This is the RCCL broadcast payload."""
        torch = _torch()
        n = self._f("bvh{S}_serialize_device")(self._h, None, 0, _stream())
        buf = torch.empty(n, dtype=torch.uint8, device="cuda")
        if self._f("bvh{S}_serialize_device")(self._h, buf.data_ptr(), n, _stream()) != n:
            raise _lib.BvhAmdError(_lib.last_error())
        return buf

    @staticmethod
    def deserialize_device(buf, dtype=np.float32, dim: int = 3) -> "Bvh":
        """Bvh::deserialize (bvh.h:231-243) of a byte stream resident in HBM (uint8 torch tensor): kernels and device-to-device
        copies only; the stream's structure is validated on the device."""
        torch = _torch()
        s = _suffix(np.dtype(dtype), dim)
        if not (buf.is_cuda and buf.dtype == torch.uint8 and buf.is_contiguous()):
            raise TypeError("deserialize_device takes a contiguous uint8 tensor resident on the GPU")
        return Bvh(getattr(_lib.load(), f"bvh{s}_deserialize_device")(buf.data_ptr(), buf.numel(), _stream()), s)

    def intersect_ray(self, ray, leaf_fn, any_hit: bool = False, robust: bool = False, inner_fn=None, start=None):
        """Bvh::intersect<IsAnyHit, IsRobust>(ray, start, stack, leaf_fn, inner_fn) (bvh.h:72-73) for ONE ray with host
        callbacks, over bvhXX_intersect_ray_visit: leaf_fn(tmax, begin, end) -> (was_hit, new_tmax) receives a BVH-order
        primitive range and the ray's current tmax and returns the possibly shortened tmax; inner_fn(first_child_id), if
        given, is called per visited pair. `ray` = {org, dir, tmin, tmax}; `start` = packed index word (default: the root's).
        The walk runs on the device (several kernel launches per ray): for throughput use bvh_amd.intersect."""
        lib = _lib.load()
        dt = np.float32 if self._s[1] == "f" else np.float64
        r = np.ascontiguousarray(ray, dtype=dt).reshape(2 * self.dim + 2)
        Visitor, leaf_t, inner_t = _lib.ray_visitor_types(self._s)
        failure = []

        def on_leaf(_user, t, begin, end):
            try:
                hit, new_t = leaf_fn(dt(t[0]), int(begin), int(end))
                t[0] = new_t
                return bool(hit)
            except BaseException as exc:                      # an exception cannot cross the C frames: end the walk, re-raise after
                failure.append(exc)
                t[0] = float("-inf")
                return True

        def on_inner(_user, first):
            try:
                if not failure:
                    inner_fn(int(first))
            except BaseException as exc:
                failure.append(exc)

        v = Visitor(None, leaf_t(on_leaf), inner_t(on_inner) if inner_fn is not None else inner_t())
        if start is None:
            start = (1 << 64) - 1                             # BVH_AMD_START_AT_ROOT
        rc = getattr(lib, f"bvh{self._s}_intersect_ray_visit")(self._h, r.ctypes.data, int(start), (RayFlags.ANY_HIT if any_hit else 0) | (RayFlags.ROBUST if robust else 0), C.byref(v))
        if failure:
            raise failure[0]
        _lib.check(rc, "intersect_ray_visit")

    def extract_bvh(self, root_id: int) -> "Bvh":
        """Bvh::extract_bvh (bvh.h:92-122): the subtree under node `root_id` as its own BVH (device op)."""
        h = getattr(_lib.load(), f"bvh{self._s}_extract")(self._h, int(root_id))
        return Bvh(h, self._s)

    @staticmethod
    def from_nodes(nodes: np.ndarray, prim_ids: np.ndarray) -> "Bvh":
        s = {28: "3f", 56: "3d", 20: "2f", 40: "2d"}[nodes.dtype.itemsize]
        lib = _lib.load()
        _torch()
        nodes = np.ascontiguousarray(nodes)
        ids = np.ascontiguousarray(prim_ids, dtype=np.uint64)
        return Bvh(getattr(lib, f"bvh{s}_from_nodes")(nodes.ctypes.data_as(C.c_void_p), len(nodes),
                                                      ids.ctypes.data_as(C.c_void_p), len(ids)), s)


def _build(bboxes, centers, config: Config, builder: _Builder, bin_count: int | None = None) -> Bvh:
    lib = _lib.load()
    dim = int(np.shape(centers)[-1])                          # (n,6) + (n,3), or (n,4) {min.x,min.y,max.x,max.y} + (n,2)
    bb = _dev(bboxes, 2 * dim)
    cc = _dev(centers, dim)
    if bb.dtype != cc.dtype or bb.shape[0] != cc.shape[0]:
        raise ValueError("bboxes (n, 2 dim) and centers (n, dim) must agree in dtype and length")
    s = _suffix(bb.dtype, dim)
    cfg = config._c()
    sah = config.sah._c()
    if bin_count is not None:                                 # BinnedSahBuilder<Node, BinCount> with a BinCount of its own
        h = getattr(lib, f"bvh{s}_build_device_binned")(bb.data_ptr(), cc.data_ptr(), bb.shape[0], C.byref(cfg), C.byref(sah), int(bin_count), _stream())
    else:
        h = getattr(lib, f"bvh{s}_build_device_sah")(bb.data_ptr(), cc.data_ptr(), bb.shape[0], C.byref(cfg), int(builder), C.byref(sah), _stream())
    return Bvh(h, s)


class DefaultBuilder:
    """bvh::v2::DefaultBuilder<Node>::build (default_builder.h:33-62)."""

    Config = Config
    Quality = Quality

    @staticmethod
    def build(bboxes, centers, config: Config | None = None, thread_pool: ThreadPool | None = None) -> Bvh:
        return _build(bboxes, centers, config or Config(),
                      _Builder.DEFAULT_PARALLEL if thread_pool is not None else _Builder.DEFAULT_SERIAL)


class BinnedSahBuilder:
    """bvh::v2::BinnedSahBuilder<Node, BinCount>::build (binned_sah_builder.h:18, :32-38); bin_count = the BinCount template
    argument (4, 8 = the reference's default, 16 or 32)."""

    @staticmethod
    def build(bboxes, centers, config: Config | None = None, bin_count: int = 8) -> Bvh:
        return _build(bboxes, centers, config or Config(), _Builder.BINNED, None if bin_count == 8 else bin_count)


class SweepSahBuilder:
    """bvh::v2::SweepSahBuilder<Node>::build (sweep_sah_builder.h:30-36)."""

    @staticmethod
    def build(bboxes, centers, config: Config | None = None) -> Bvh:
        return _build(bboxes, centers, config or Config(), _Builder.SWEEP)


class MiniTreeBuilder:
    """bvh::v2::MiniTreeBuilder<Node>::build(thread_pool, bboxes, centers, config) (mini_tree_builder.h:29-58), 3D."""

    @dataclass
    class Config:
        min_leaf_size: int = 1
        max_leaf_size: int = 8
        enable_pruning: bool = True
        pruning_area_ratio: float = 0.01
        parallel_threshold: int = 1024
        log2_grid_dim: int = 4
        sah: SplitHeuristic = field(default_factory=SplitHeuristic)

    @staticmethod
    def build(bboxes, centers, config: "MiniTreeBuilder.Config | None" = None, thread_pool: ThreadPool | None = None) -> Bvh:
        c = config or MiniTreeBuilder.Config()
        bb, cc = _dev(bboxes, 6), _dev(centers, 3)
        if bb.dtype != cc.dtype or bb.shape[0] != cc.shape[0]:
            raise ValueError("bboxes (n,6) and centers (n,3) must agree in dtype and length")
        s = _suffix(bb.dtype)
        cfg = _lib.MiniTreeConfig(c.min_leaf_size, c.max_leaf_size, int(c.enable_pruning), float(c.pruning_area_ratio), c.parallel_threshold,
                                  c.log2_grid_dim, int(c.sah.log_cluster_size), float(c.sah.cost_ratio))
        return Bvh(getattr(_lib.load(), f"bvh{s}_build_minitree_device")(bb.data_ptr(), cc.data_ptr(), bb.shape[0], C.byref(cfg), _stream()), s)


def tri_bounds(tris9):
    """Tri::get_bbox / Tri::get_center (tri.h:24-25) for n triangles -> (bboxes (n,6), centers (n,3)) in HBM."""
    torch = _torch()
    t = _dev(tris9, 9)
    s = _suffix(t.dtype)
    bb = torch.empty((t.shape[0], 6), dtype=t.dtype, device=t.device)
    cc = torch.empty((t.shape[0], 3), dtype=t.dtype, device=t.device)
    _lib.check(getattr(_lib.load(), f"bvh_amd_tri_bounds{s}")(t.data_ptr(), t.shape[0], bb.data_ptr(), cc.data_ptr(), _stream()),
               "tri_bounds")
    return bb, cc


def precompute_tris(tris9, perm=None):
    """PrecomputedTri (tri.h:35-37) of tris[perm[i]] -> (n,12) {p0,e1,e2,n} in HBM."""
    torch = _torch()
    t = _dev(tris9, 9)
    s = _suffix(t.dtype)
    if perm is not None:
        perm = _dev(perm) if not isinstance(perm, np.ndarray) else _dev(perm.astype(np.int32))
        perm = perm.to(torch.int32)
        n = perm.shape[0]
    else:
        n = t.shape[0]
    out = torch.empty((n, 12), dtype=t.dtype, device=t.device)
    _lib.check(getattr(_lib.load(), f"bvh_amd_precompute_tris{s}")(t.data_ptr(), perm.data_ptr() if perm is not None else None,
                                                                    n, out.data_ptr(), _stream()), "precompute_tris")
    return out


def sphere_bounds(sph4):
    """Sphere::get_bbox / get_center (sphere.h:24-27): (n,4) spheres {center, radius} -> (n,6), (n,3); (n,3) circles
    {center.x, center.y, radius} -> (n,4) {min.x,min.y,max.x,max.y}, (n,2)."""
    torch = _torch()
    dim = int(np.shape(sph4)[-1]) - 1
    t = _dev(sph4, dim + 1)
    s = _suffix(t.dtype, dim)
    bb = torch.empty((t.shape[0], 2 * dim), dtype=t.dtype, device=t.device)
    cc = torch.empty((t.shape[0], dim), dtype=t.dtype, device=t.device)
    _lib.check(getattr(_lib.load(), f"bvh_amd_sphere_bounds{s}")(t.data_ptr(), t.shape[0], bb.data_ptr(), cc.data_ptr(), _stream()),
               "sphere_bounds")
    return bb, cc


def pinhole_rays(width: int, height: int, eye, direction, up, dtype=np.float32):
    """Primary rays of the reference's benchmark camera (test/benchmark.cpp:343-359), generated on the device: (h*w, 8)."""
    torch = _torch()
    dt = np.dtype(dtype)
    s = _suffix(torch.float32 if dt == np.float32 else torch.float64)
    arr = [np.ascontiguousarray(np.asarray(v, dtype=dt).reshape(3)) for v in (eye, direction, up)]
    out = torch.empty((width * height, 8), dtype=torch.float32 if dt == np.float32 else torch.float64, device="cuda")
    _lib.check(getattr(_lib.load(), f"bvh_amd_pinhole_rays{s}")(arr[0].ctypes.data_as(C.c_void_p), arr[1].ctypes.data_as(C.c_void_p),
                                                              arr[2].ctypes.data_as(C.c_void_p), width, height, out.data_ptr(), _stream()),
               "pinhole_rays")
    return out


def shade_eyelight(prims12, rays, hits):
    """Eyelight shading of test/benchmark.cpp:363-371 on the device -> (n, 3) uint8."""
    torch = _torch()
    p, r = _dev(prims12, 12), _dev(rays, 8)
    s = _suffix(p.dtype)
    out = torch.empty((r.shape[0], 3), dtype=torch.uint8, device=p.device)
    _lib.check(getattr(_lib.load(), f"bvh_amd_shade_eyelight{s}")(p.data_ptr(), r.data_ptr(), hits.data_ptr(), r.shape[0], out.data_ptr(), _stream()),
               "shade_eyelight")
    return out


def gather(records, perm):
    """out[i] = records[perm[i]] on the device (prim permutation, test/benchmark.cpp:221-225)."""
    torch = _torch()
    r = _dev(records)
    p = _dev(perm).to(torch.int32)
    out = torch.empty((p.shape[0],) + tuple(r.shape[1:]), dtype=r.dtype, device=r.device)
    stride = r.element_size() * int(np.prod(r.shape[1:]))
    _lib.check(_lib.load().bvh_amd_gather(r.data_ptr(), p.data_ptr(), p.shape[0], stride, out.data_ptr(), _stream()), "gather")
    return out


def prepare_trace(bvh: Bvh, n_rays_hint: int = 0):
    """bvhXX_prepare_trace: the per-tree one-offs of the first large batch (depth pass, first reordering scratch for batches of
    `n_rays_hint` rays) paid now, on the current stream. Optional; 3D families."""
    if bvh.dim != 3:
        return
    _lib.check(getattr(_lib.load(), f"bvh{bvh._s}_prepare_trace")(bvh._h, int(n_rays_hint), _stream()), "prepare_trace")


def intersect(bvh: Bvh, prims, rays, any_hit: bool = False, robust: bool = False, leaf: str = "tri",
              counters: bool = False, out=None, sort_rays=None, original_ids: bool = False):
    """Batched Bvh::intersect<IsAnyHit, IsRobust> (bvh.h:160-182) with the closest/any-hit leaf loop of
    test/benchmark.cpp:281-291. prims are in BVH order. Returns a torch tensor of hit records
    ((n,4) of the BVH scalar type; view with hits_to_numpy) and, optionally, (pairs, tests, leaves). original_ids: report
    the original primitive id (bvh.prim_ids[i]) instead of the BVH-order index i the reference's leaf callback sees."""
    torch = _torch()
    lib = _lib.load()
    s = bvh._s
    dt = torch.float32 if s[1] == "f" else torch.float64
    r = _dev(rays, 2 * bvh.dim + 2)                           # {org, dir, tmin, tmax}
    p = _dev(prims)
    if bvh.dim == 2:
        leaf = "sphere"                                       # circles {center.x, center.y, radius}: the only 2D leaf (sphere.h)
    if r.dtype != dt or p.dtype != dt:
        raise TypeError("prims/rays dtype must match the BVH scalar type")
    n = r.shape[0]
    out = _records_out(out, n, dt, r.device)
    cnt = _counters(counters, r.device)
    flags = (RayFlags.ANY_HIT if any_hit else 0) | (RayFlags.ROBUST if robust else 0) | (0 if sort_rays is None else RayFlags.SORTED if sort_rays else RayFlags.UNSORTED) | \
            (8 if original_ids else 0)                        # BVH_AMD_RAY_ORIGINAL_IDS: hit.prim = bvh.prim_ids[BVH-order index]
    fn = getattr(lib, f"bvh{s}_intersect_rays_{'tri' if leaf == 'tri' else 'sphere'}")
    _lib.check(fn(bvh._h, p.data_ptr(), r.data_ptr(), n, int(flags), out.data_ptr(),
                  cnt.data_ptr() if counters else None, _stream()), "intersect_rays")
    if counters:
        return out, cnt
    return out


def closest_points(bvh: Bvh, prims, points, max_distance: float = float("inf"), leaf: str = "tri", counters: bool = False, out=None,
                   sort_queries=None, original_ids: bool = False):
    """For each point, the nearest primitive within max_distance and its distance (bvhXX_closest_points_*): among the primitives the
    walk tests, the lowest BVH-order index of those at the smallest computed distance. A subtree whose box is computed farther than the
    best so far is skipped, so this is the brute force's argmin by (distance, index) exactly when distances are computed exactly, and
    within rounding of its distance otherwise. prims are in BVH order
    ((n, 12) PrecomputedTri or (n, 4) spheres, as for intersect). points: (n, 3) with the scalar max_distance, or (n, 4) with a
    per-query radius in column 3 (max_distance left at its default). Returns the (n, 4) tensor of hit records (hits_to_numpy views
    it): prim = BVH-order index (bvh.prim_ids[i] with original_ids) or INVALID, t = distance (max_distance on a miss), (u, v) the
    barycentrics of the closest point of a triangle (point = p0 + u (p1 - p0) + v (p2 - p0); 0 for spheres); with counters also
    (pairs, tests, leaves). sort_queries: True / False force / forbid reordering the batch internally (None: the library decides)."""
    q, p, dt = _point_query_args(bvh, prims, points, max_distance, leaf, "closest_points", "max_distance", float("inf"))
    n = q.shape[0]
    out = _records_out(out, n, dt, q.device)
    cnt = _counters(counters, q.device)
    fn = getattr(_lib.load(), f"bvh{bvh._s}_closest_points_{leaf}")
    _lib.check(fn(bvh._h, p.data_ptr(), q.data_ptr(), n, int(_sort_flags(sort_queries, original_ids)), out.data_ptr(), cnt.data_ptr() if counters else None, _stream()),
               "closest_points")
    if counters:
        return out, cnt
    return out


def _point_query_args(bvh: Bvh, prims, points, radius, leaf: str, who: str, name: str = "radius", unset=None):
    """The checks and the (n, 4) query tensor of the point queries: (queries, prims, scalar dtype). `radius` is the argument called
    `name`, `unset` its default: (n, 4) points carry a radius per query and want it left there; (n, 3) points take the scalar, which
    must be given when the default is None."""
    torch = _torch()
    if bvh.dim != 3:
        raise TypeError(f"{who}: 3D trees only")
    if leaf not in ("tri", "sphere"):
        raise ValueError("leaf is 'tri' or 'sphere'")
    dt = torch.float32 if bvh._s[1] == "f" else torch.float64
    pts = _dev(points)
    if pts.dim() != 2 or pts.shape[1] not in (3, 4):
        raise ValueError("points must be (n, 3) or (n, 4)")
    if pts.dtype != dt:
        raise TypeError("points dtype must match the BVH scalar type")
    if pts.shape[1] == 3:
        if unset is None and radius is None:
            raise ValueError("(n, 3) points need a radius")
        q = torch.empty((pts.shape[0], 4), dtype=dt, device=pts.device)
        q[:, :3] = pts
        q[:, 3] = float(radius)
    else:
        if (radius is not None) if unset is None else (radius != unset):
            raise ValueError(f"(n, 4) points carry their own radius: leave {name} at its default")
        q = pts
    p = _dev(prims)
    if p.dtype != dt:
        raise TypeError("prims dtype must match the BVH scalar type")
    return q, p, dt


def _sort_flags(sort_queries, original_ids=False):
    return (0 if sort_queries is None else RayFlags.SORTED if sort_queries else RayFlags.UNSORTED) | (8 if original_ids else 0)


def _counters(counters: bool, dev):
    """The (pairs, tests, leaves) tensor a query fills when asked for counters, else None."""
    torch = _torch()
    return torch.zeros(3, dtype=torch.int64, device=dev) if counters else None


def _records_out(out, n: int, dt, dev, who=None):
    """`out` as given, or allocated: the contiguous (n, 4) tensor of hit records of the tree's scalar type. `who` names the function
    that checks a given `out` (intersect and closest_points take it as it comes)."""
    if out is None:
        return _torch().empty((n, 4), dtype=dt, device=dev)
    if who is not None and (out.dtype != dt or not out.is_contiguous() or out.numel() < n * 4):
        raise TypeError(f"{who}: out must be a contiguous (n, 4) tensor of the BVH scalar type")
    return out


def _per_query_value(value, n: int, dt, who: str, name: str, one: str):
    """A float for the batch, or one value per query: (scalar, None) or (0.0, the (n,) device tensor). `name` is the argument, `one`
    what it holds ("radius per ray")."""
    if isinstance(value, (int, float)):
        return float(value), None
    values = _dev(value)
    if values.dtype != dt:
        raise TypeError(f"{name} dtype must match the BVH scalar type")
    if values.dim() != 1 or values.shape[0] != n:
        raise ValueError(f"{who}: {name} must be a float or hold one {one} ({n}), got shape {tuple(values.shape)}")
    return 0.0, values


def winding_prepare(bvh: Bvh, prims, out=None):
    """The per-node moments the winding-number queries read (bvh3X_winding_prepare): a (node_count + 1, 8) tensor of the tree's scalar
    type, node c in row c + 1 as {cx, cy, cz, r2, Nx, Ny, Nz, area}, written into `out` if given. prims: the BVH-order (n, 12)
    PrecomputedTri. The tree is only read. The moments are stale after Bvh.refit_tris and Bvh.optimize: prepare them again."""
    torch = _torch()
    if bvh.dim != 3:
        raise TypeError("winding_prepare: 3D trees only")
    dt = torch.float32 if bvh._s[1] == "f" else torch.float64
    p = _dev(prims, 12)
    if p.dtype != dt:
        raise TypeError("prims dtype must match the BVH scalar type")
    rows = bvh.node_count + 1
    if out is None:
        out = torch.empty((rows, 8), dtype=dt, device=p.device)
    elif out.dtype != dt or not out.is_contiguous() or out.numel() < rows * 8:
        raise TypeError("winding_prepare: out must be a contiguous (node_count + 1, 8) tensor of the BVH scalar type")
    _lib.check(getattr(_lib.load(), f"bvh{bvh._s}_winding_prepare")(bvh._h, p.data_ptr(), out.data_ptr(), out.numel() // 8, _stream()), "winding_prepare")
    return out


def _winding_call(bvh: Bvh, p, moments, q, beta, sort_queries, counters: bool, out, hits, who: str):
    torch = _torch()
    m = _dev(moments)
    if m.dtype != q.dtype:
        raise TypeError("moments dtype must match the BVH scalar type")
    n = q.shape[0]
    if out is None:
        out = torch.empty(n, dtype=q.dtype, device=q.device)
    cnt = _counters(counters, q.device)
    fn = getattr(_lib.load(), f"bvh{bvh._s}_winding_numbers")
    _lib.check(fn(bvh._h, p.data_ptr(), m.data_ptr(), m.numel() // 8, q.data_ptr(), n, float(beta), int(_sort_flags(sort_queries)), out.data_ptr(),
                  hits.data_ptr() if hits is not None else None, cnt.data_ptr() if counters else None, _stream()), who)
    return out, cnt


def winding_numbers(bvh: Bvh, prims, moments, points, beta: float = 2.0, sort_queries=None, counters: bool = False, out=None):
    """For each point, the generalized winding number of the triangle mesh (bvh3X_winding_numbers): 1 inside and 0 outside a closed mesh
    whose (p1 - p0) x (p2 - p0) point outward, 0 in the cavity of a shell, 2 inside a doubled surface, fractional near the holes of an
    open or defective mesh. prims: the BVH-order (n, 12) PrecomputedTri; moments: winding_prepare's tensor for the same tree and
    triangles. points: (n, 3), or (n, 4) as closest_points takes them (column 3 is not read). beta >= 1 trades speed for accuracy: a
    node farther than beta radii is replaced by one dipole; inf gives the exact sum. Returns the (n,) tensor of the tree's scalar type
    (NaN for a point with a NaN or infinite coordinate); with counters also (pair records opened, triangles summed, far terms added).
    sort_queries: True / False force / forbid reordering the batch internally (None: the library decides); values never change."""
    q, p, _ = _point_query_args(bvh, prims, points, 0.0, "tri", "winding_numbers", "max_distance", 0.0)
    w, cnt = _winding_call(bvh, p, moments, q, beta, sort_queries, counters, out, None, "winding_numbers")
    return (w, cnt) if counters else w


def signed_distance(bvh: Bvh, prims, moments, points, beta: float = 2.0, max_distance: float = float("inf"), sort_queries=None, out=None):
    """closest_points' (n, 4) hit records with a signed t: negative where the winding number is at least 1/2 (bvh3X_closest_points_tri,
    then bvh3X_winding_numbers on the same queries with the records as d_hits). Every other field is closest_points'; a miss keeps
    prim = INVALID and carries +-max_distance."""
    q, p, dt = _point_query_args(bvh, prims, points, max_distance, "tri", "signed_distance", "max_distance", float("inf"))
    hits = closest_points(bvh, p, q, sort_queries=sort_queries, out=out)
    _winding_call(bvh, p, moments, q, beta, sort_queries, False, None, hits, "signed_distance")
    return hits


def occupancy(bvh: Bvh, prims, moments, points, beta: float = 2.0, sort_queries=None):
    """For each point, whether it is inside the mesh: winding_numbers(...) >= 0.5 as an (n,) bool tensor (False for a NaN point)."""
    return winding_numbers(bvh, prims, moments, points, beta=beta, sort_queries=sort_queries) >= 0.5


def offsets_from_counts(counts):
    """(n + 1,) int64 offsets {0, c0, c0 + c1, ...} of an (n,) int32 tensor of counts, on the device and without a read-back
    (bvh_amd_offsets_from_counts)."""
    torch = _torch()
    c = _dev(counts)
    if c.dtype != torch.int32 or c.dim() != 1:
        raise TypeError("counts must be a 1-D int32 tensor")
    out = torch.empty(c.shape[0] + 1, dtype=torch.int64, device=c.device)
    _lib.check(_lib.load().bvh_amd_offsets_from_counts(c.data_ptr() if c.shape[0] else None, c.shape[0], out.data_ptr(), _stream()), "offsets_from_counts")
    return out


def radius_count(bvh: Bvh, prims, points, radius=None, leaf: str = "tri", sort_queries=None, counters: bool = False):
    """For each point, how many primitives lie within the radius (bvhXX_radius_search_* without lists): an int32 (n,) tensor; with
    counters also (pairs, tests, leaves). points: (n, 3) with the scalar radius, or (n, 4) with a per-query radius in column 3."""
    q, p, _ = _point_query_args(bvh, prims, points, radius, leaf, "radius_count")
    n = q.shape[0]
    fn = getattr(_lib.load(), f"bvh{bvh._s}_radius_search_{leaf}")
    flags = int(_sort_flags(sort_queries))
    call = lambda counts, offsets, ids, dist, cnt: fn(bvh._h, p.data_ptr(), q.data_ptr(), n, flags, counts, offsets, ids, dist, cnt, _stream())
    return _count_only("radius_count", call, n, q.device, counters)


def radius_search(bvh: Bvh, prims, points, radius=None, leaf: str = "tri", max_per_query=None, distances: bool = True,
                  original_ids: bool = False, sort_queries=None, counters: bool = False):
    """For each point, the primitives within the radius (bvhXX_radius_search_*), in the order the tree fixes (depth-first, left child
    first, ascending index inside a leaf). prims are in BVH order, as for closest_points; points: (n, 3) with the scalar radius, or
    (n, 4) with a per-query radius in column 3. Returns (offsets, ids, dist): offsets int64 (n + 1,), query q owns
    ids[offsets[q]:offsets[q + 1]] (int32 BVH-order indices, or bvh.prim_ids[i] with original_ids) and the distances beside them
    (None without `distances`).
      max_per_query=None: exact lists — a count pass, the offsets on the device, one read of offsets[-1] to size the lists, a fill pass.
      max_per_query=k: one pass, k slots per query (offsets = k * arange(n + 1)): the first k of each list, the unused slots holding
        -1 (INVALID) and the query's radius; returns (offsets, ids, dist, counts), counts (int32, untruncated) telling which lists
        overflowed.
    With counters, (pairs, tests, leaves) of the pass that wrote the lists is appended to the result."""
    q, p, dt = _point_query_args(bvh, prims, points, radius, leaf, "radius_search")
    n = q.shape[0]
    fn = getattr(_lib.load(), f"bvh{bvh._s}_radius_search_{leaf}")
    flags = int(_sort_flags(sort_queries, original_ids))
    call = lambda counts, offsets, ids, dist, cnt: fn(bvh._h, p.data_ptr(), q.data_ptr(), n, flags, counts, offsets, ids, dist, cnt, _stream())
    return _two_pass_lists("radius_search", call, n, q.device, max_per_query, counters, dt if distances else None)


def _two_pass_lists(who: str, call, n: int, dev, max_per_query, counters: bool, dist_dtype=None, record_dtype=None):
    """Count pass, offsets, fill pass (or one pass into max_per_query slots) of call(counts, offsets, ids, dist, counters), the list
    output of radius_search, the overlap queries and ray_hits: (offsets, ids, dist[, counts][, counters]); dist (None without
    dist_dtype) is written beside ids. With record_dtype the list is ONE array of hit records, (total, 4) of that scalar type, in
    the place of ids."""
    torch = _torch()
    cnt = _counters(counters, dev)
    counts = torch.zeros(n, dtype=torch.int32, device=dev)
    if max_per_query is None:
        _lib.check(call(counts.data_ptr(), None, None, None, None), who)
        offsets = offsets_from_counts(counts)
        total = int(offsets[-1].item())
    else:
        k = int(max_per_query)
        if k < 0:
            raise ValueError("max_per_query must not be negative")
        offsets = torch.arange(n + 1, dtype=torch.int64, device=dev) * k
        total = n * k
    if record_dtype is not None:
        ids = torch.empty((max(total, 1), 4), dtype=record_dtype, device=dev)
    else:
        ids = torch.empty(max(total, 1), dtype=torch.int32, device=dev)           # (never a null pointer: an empty result is still a list)
    dist = torch.empty(max(total, 1), dtype=dist_dtype, device=dev) if dist_dtype is not None else None
    _lib.check(call(counts.data_ptr() if max_per_query is not None else None, offsets.data_ptr(), ids.data_ptr(),
                    dist.data_ptr() if dist is not None else None, cnt.data_ptr() if counters else None), who)
    ids, dist = ids[:total], dist[:total] if dist is not None else None
    out = (offsets, ids, dist) if max_per_query is None else (offsets, ids, dist, counts)
    return out + (cnt,) if counters else out


def _count_only(who: str, call, n: int, dev, counters: bool):
    """The count pass of call(counts, offsets, ids, dist, counters) alone, no lists: the int32 (n,) counts[, counters]."""
    torch = _torch()
    counts = torch.zeros(n, dtype=torch.int32, device=dev)
    cnt = _counters(counters, dev)
    _lib.check(call(counts.data_ptr(), None, None, None, cnt.data_ptr() if counters else None), who)
    return (counts, cnt) if counters else counts


def _ray_query_args(bvh: Bvh, prims, rays, leaf: str, who: str):
    """The checks of the all-hits ray queries: ((n, 8) rays, prims, scalar dtype)."""
    torch = _torch()
    if bvh.dim != 3:
        raise TypeError(f"{who}: 3D trees only")
    if leaf not in ("tri", "sphere"):
        raise ValueError("leaf is 'tri' or 'sphere'")
    dt = torch.float32 if bvh._s[1] == "f" else torch.float64
    r = _dev(rays, 8)                                         # {org, dir, tmin, tmax}
    p = _dev(prims)
    if r.dtype != dt or p.dtype != dt:
        raise TypeError("prims/rays dtype must match the BVH scalar type")
    return r, p, dt


def ray_hit_count(bvh: Bvh, prims, rays, leaf: str = "tri", robust: bool = False, sort_queries=None, counters: bool = False):
    """For each ray, how many primitives the unshortened ray crosses (bvh3X_intersect_rays_all_* without lists): an int32 (n,)
    tensor; with counters also (pairs, tests, leaves). prims and rays as for intersect."""
    r, p, _ = _ray_query_args(bvh, prims, rays, leaf, "ray_hit_count")
    n = r.shape[0]
    fn = getattr(_lib.load(), f"bvh{bvh._s}_intersect_rays_all_{leaf}")
    flags = int(_sort_flags(sort_queries)) | (int(RayFlags.ROBUST) if robust else 0)
    call = lambda counts, offsets, hits, _, cnt: fn(bvh._h, p.data_ptr(), r.data_ptr(), n, flags, counts, offsets, hits, cnt, _stream())
    return _count_only("ray_hit_count", call, n, r.device, counters)


def ray_hits(bvh: Bvh, prims, rays, leaf: str = "tri", robust: bool = False, max_per_ray=None, original_ids: bool = False, sort_queries=None,
             counters: bool = False):
    """For each ray, every primitive the unshortened ray {org, dir, tmin, tmax} crosses (bvh3X_intersect_rays_all_*): what the
    reference's intersect reports to a leaf_fn that records a hit and never shortens the ray. The hits of a ray come in the order the
    tree fixes (depth-first, left child first, ascending index inside a leaf), NOT sorted by t; equal t are all kept. prims are in BVH
    order, as for intersect. Returns (offsets, hits): offsets int64 (n + 1,), ray r owns hits[offsets[r]:offsets[r + 1]], an (m, 4)
    tensor of the records intersect writes (hits_to_numpy views it): {prim, t, u, v} for triangles, {prim, t0, t1, 0} for spheres;
    prim is the BVH-order index, or bvh.prim_ids[i] with original_ids.
      max_per_ray=None: exact lists - a count pass, the offsets on the device, one read of offsets[-1] to size the lists, a fill pass.
      max_per_ray=k: one pass, k slots per ray (offsets = k * arange(n + 1)): the first k of each list, the unused slots holding
        intersect's miss record {INVALID, the ray's tmax, 0, 0}; returns (offsets, hits, counts), counts (int32, untruncated) telling
        which lists overflowed.
    With counters, (pairs, tests, leaves) of the pass that wrote the lists is appended to the result."""
    r, p, dt = _ray_query_args(bvh, prims, rays, leaf, "ray_hits")
    n = r.shape[0]
    fn = getattr(_lib.load(), f"bvh{bvh._s}_intersect_rays_all_{leaf}")
    flags = int(_sort_flags(sort_queries, original_ids)) | (int(RayFlags.ROBUST) if robust else 0)
    call = lambda counts, offsets, hits, _, cnt: fn(bvh._h, p.data_ptr(), r.data_ptr(), n, flags, counts, offsets, hits, cnt, _stream())
    out = _two_pass_lists("ray_hits", call, n, r.device, max_per_ray, counters, record_dtype=dt)
    return out[:2] + out[3:]                                                        # (no distances beside the records)


RAY_NEAREST_MAX_K = 64                          # BVH_AMD_RAY_NEAREST_MAX_K


def ray_hits_nearest(bvh: Bvh, prims, rays, k: int, leaf: str = "tri", robust: bool = False, original_ids: bool = False, sort_queries=None,
                     counters: bool = False):
    """For each ray, the first k primitives it crosses, front to back (bvh3X_intersect_rays_nearest_*): the k smallest (t, BVH-order
    index) among the primitives the walk tests and the unshortened ray {org, dir, tmin, tmax} crosses, ascending; equal t sort by
    index. k = 1 is intersect's hit (the lowest index where primitives tie at its t); k >= a ray's ray_hits count gives that list
    sorted by (t, prim), byte for byte. prims are in BVH order, as for intersect. Returns (hits, counts): hits (n, k, 4), the
    records intersect writes (hits_to_numpy views them as n * k records): {prim, t, u, v} for triangles, {prim, t0, t1, 0} for spheres;
    prim is the BVH-order index, or bvh.prim_ids[i] with original_ids; the unused slots of a row hold intersect's miss record
    {INVALID, the ray's tmax, 0, 0}. counts int32 (n,): the valid records of each row. With counters, (pairs, tests, leaves) is
    appended to the result. sort_queries: True / False force / forbid reordering the batch internally (None: the library decides)."""
    torch = _torch()
    k = int(k)
    if not 1 <= k <= RAY_NEAREST_MAX_K:
        raise ValueError(f"k must be in [1, {RAY_NEAREST_MAX_K}]")
    r, p, dt = _ray_query_args(bvh, prims, rays, leaf, "ray_hits_nearest")
    n = r.shape[0]
    hits = torch.empty((n, k, 4), dtype=dt, device=r.device)
    counts = torch.zeros(n, dtype=torch.int32, device=r.device)
    cnt = _counters(counters, r.device)
    fn = getattr(_lib.load(), f"bvh{bvh._s}_intersect_rays_nearest_{leaf}")
    flags = int(_sort_flags(sort_queries, original_ids)) | (int(RayFlags.ROBUST) if robust else 0)
    _lib.check(fn(bvh._h, p.data_ptr(), r.data_ptr(), n, k, flags, hits.data_ptr(), counts.data_ptr(), cnt.data_ptr() if counters else None, _stream()),
               "ray_hits_nearest")
    return (hits, counts, cnt) if counters else (hits, counts)


def sphere_cast(bvh: Bvh, prims, rays, radius, leaf: str = "tri", robust: bool = False, original_ids: bool = False, sort_queries=None,
                counters: bool = False, out=None):
    """For each ray {org, dir, tmin, tmax}, the first contact of a ball of the given radius whose centre moves along org + t dir
    (bvh3X_sphere_cast_*): the smallest t in [tmin, tmax] at which the ball touches a solid triangle or solid sphere, ties to the
    lowest BVH-order index among the primitives the walk tests. radius: a float for the whole batch, or an array / tensor of n.
    prims are in BVH order, as for closest_points. Returns the (n, 4) tensor of hit records (hits_to_numpy views it), written into
    `out` if given: prim = BVH-order index (bvh.prim_ids[i] with original_ids) or INVALID, t = the contact's ray parameter (t == tmin:
    the ball overlaps at its start; tmax on a miss), (u, v) = the barycentrics of the contact point on a triangle in closest_points'
    convention (0 for spheres): the contact normal is (org + t dir - point) / radius. A NaN or negative radius, a NaN tmin or tmax:
    a miss. robust=True takes the robust box test: wanted for axis-parallel sweeps (a direction component of exactly 0), which the
    fast test loses as intersect's does. With counters also (pairs, tests, leaves). sort_queries: True / False force / forbid reordering the batch internally
    (None: the library decides); records never change."""
    r, p, dt = _ray_query_args(bvh, prims, rays, leaf, "sphere_cast")
    n = r.shape[0]
    scalar, radii = _per_query_value(radius, n, dt, "sphere_cast", "radius", "radius per ray")
    out = _records_out(out, n, dt, r.device, "sphere_cast")
    cnt = _counters(counters, r.device)
    fn = getattr(_lib.load(), f"bvh{bvh._s}_sphere_cast_{leaf}")
    flags = int(_sort_flags(sort_queries, original_ids)) | (int(RayFlags.ROBUST) if robust else 0)
    _lib.check(fn(bvh._h, p.data_ptr(), r.data_ptr(), n, scalar, radii.data_ptr() if radii is not None and n else None, flags, out.data_ptr(),
                  cnt.data_ptr() if counters else None, _stream()), "sphere_cast")
    return (out, cnt) if counters else out


def _overlap_args(bvh: Bvh, bboxes, query_boxes, who: str):
    """The checks of the box-overlap queries: ((n_boxes, 6) boxes by original id, (n, 6) query boxes or None)."""
    if bvh.dim != 3:
        raise TypeError(f"{who}: 3D trees only")
    bb = bvh._prims_in(bboxes, 6, who)
    q = None if query_boxes is None else bvh._prims_in(query_boxes, 6, who)
    return bb, q


def overlap_count(bvh: Bvh, bboxes, query_boxes, sort_queries=None, counters: bool = False):
    """For each query box, how many primitives' boxes overlap it (bvh3X_overlap_boxes without lists): an int32 (n,) tensor; with
    counters also (pairs, box tests, leaves). bboxes: (n_boxes, 6) {min, max} indexed by ORIGINAL primitive id, what the builders and
    refit_boxes take; query_boxes: (n, 6) in the same layout. Closed intervals: touching boxes overlap."""
    bb, q = _overlap_args(bvh, bboxes, query_boxes, "overlap_count")
    fn = getattr(_lib.load(), f"bvh{bvh._s}_overlap_boxes")
    flags = int(_sort_flags(sort_queries))
    n = q.shape[0]
    call = lambda counts, offsets, ids, _, cnt: fn(bvh._h, bb.data_ptr(), bb.shape[0], q.data_ptr(), n, flags, counts, offsets, ids, cnt, _stream())
    return _count_only("overlap_count", call, n, q.device, counters)


def overlap_search(bvh: Bvh, bboxes, query_boxes, max_per_query=None, original_ids: bool = False, sort_queries=None, counters: bool = False):
    """For each query box, the primitives whose boxes overlap it (bvh3X_overlap_boxes), in the order the tree fixes (depth-first, left
    child first, ascending index inside a leaf). For a tree built from or refitted to `bboxes` this is exactly the brute-force set.
    Returns (offsets, ids) as radius_search does without distances: offsets int64 (n + 1,), query q owns ids[offsets[q]:offsets[q + 1]]
    (int32 BVH-order indices, or bvh.prim_ids[i] with original_ids).
      max_per_query=None: exact lists - a count pass, the offsets on the device, one read of offsets[-1] to size the lists, a fill pass.
      max_per_query=k: one pass, k slots per query (offsets = k * arange(n + 1)), unused slots holding -1 (INVALID); returns
        (offsets, ids, counts), counts (int32, untruncated) telling which lists overflowed.
    With counters, (pairs, box tests, leaves) of the pass that wrote the lists is appended to the result."""
    bb, q = _overlap_args(bvh, bboxes, query_boxes, "overlap_search")
    fn = getattr(_lib.load(), f"bvh{bvh._s}_overlap_boxes")
    flags = int(_sort_flags(sort_queries, original_ids))
    n = q.shape[0]
    call = lambda counts, offsets, ids, _, cnt: fn(bvh._h, bb.data_ptr(), bb.shape[0], q.data_ptr(), n, flags, counts, offsets, ids, cnt, _stream())
    out = _two_pass_lists("overlap_search", call, n, q.device, max_per_query, counters)
    return out[:2] + out[3:]                                                        # (no distances)


def self_overlaps(bvh: Bvh, bboxes, original_ids: bool = True, counters: bool = False):
    """Every unordered pair of primitives whose boxes overlap, once (bvh3X_overlap_self): the broad phase of a self-collision test. An
    (m, 2) int64 device tensor; with original_ids both columns hold original primitive ids (rows of `bboxes`), otherwise BVH-order
    indices with first < second. The rows are expanded from the CSR offsets with torch. With counters, (pairs, box tests, leaves) of
    the fill pass is returned too."""
    torch = _torch()
    bb, _ = _overlap_args(bvh, bboxes, None, "self_overlaps")
    fn = getattr(_lib.load(), f"bvh{bvh._s}_overlap_self")
    n = bvh.prim_count
    call = lambda counts, offsets, ids, _, cnt: fn(bvh._h, bb.data_ptr(), bb.shape[0], 8 if original_ids else 0, counts, offsets, ids, cnt, _stream())
    out = _two_pass_lists("self_overlaps", call, n, bb.device, None, counters)
    offsets, ids = out[0], out[1]
    rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=bb.device), offsets[1:] - offsets[:-1])
    if original_ids:
        rows = bvh.device_prim_ids().long()[rows]
    pairs = torch.stack([rows, ids.long()], dim=1)
    return (pairs, out[3]) if counters else pairs


_TRI_SKIP_SHARED = 32                                         # BVH_AMD_TRI_SKIP_SHARED


def _tri_intersect_args(bvh: Bvh, tris9, query_tris, who: str):
    """The checks of the triangle-intersection queries: ((n_tris, 9) triangles by original id, (n, 9) query triangles or None)."""
    if bvh.dim != 3:
        raise TypeError(f"{who}: 3D trees only")
    t = bvh._prims_in(tris9, 9, who)
    q = None if query_tris is None else bvh._prims_in(query_tris, 9, who)
    return t, q


def tri_intersect_count(bvh: Bvh, tris9, query_tris, skip_shared: bool = False, sort_queries=None, counters: bool = False):
    """For each query triangle, how many of the tree's triangles intersect it (bvh3X_intersect_tris without lists): an int32 (n,)
    tensor; with counters also (pairs, triangles fetched, leaves). tris9: (n_tris, 9) {p0, p1, p2} indexed by ORIGINAL primitive id,
    what refit_tris takes; query_tris: (n, 9) in the same layout. Closed sets: touching triangles intersect; a triangle without area
    or with a NaN or infinite coordinate intersects nothing. skip_shared: pairs with a common vertex are not counted."""
    t, q = _tri_intersect_args(bvh, tris9, query_tris, "tri_intersect_count")
    fn = getattr(_lib.load(), f"bvh{bvh._s}_intersect_tris")
    flags = int(_sort_flags(sort_queries)) | (_TRI_SKIP_SHARED if skip_shared else 0)
    n = q.shape[0]
    call = lambda counts, offsets, ids, _, cnt: fn(bvh._h, t.data_ptr(), t.shape[0], q.data_ptr(), n, flags, counts, offsets, ids, cnt, _stream())
    return _count_only("tri_intersect_count", call, n, q.device, counters)


_REGION_EXACT = 64                                            # BVH_AMD_REGION_EXACT
REGION_MAX_PLANES = 8


def frustum_planes(eye, direction, up, fov_y, aspect, near, far, dtype=np.float32):
    """The six planes {nx, ny, nz, d} of a view frustum, normals pointing OUT of it (a point x is inside iff n . x + d <= 0 for all
    six), as a (6, 4) numpy array in the order near, far, left, right, bottom, top: what region_count / region_search take. The camera
    is pinhole_rays': looking along `direction`, right = normalize(direction x up), the image's up = right x direction; fov_y is the
    full vertical opening angle in radians and aspect = width / height of the opening (pinhole_rays' own frustum, whatever its
    resolution, is fov_y = pi / 2, aspect = 1). The side planes pass through the eye; near and far are distances along `direction`.
    Computed in float64 and rounded once to `dtype`."""
    e = np.asarray(eye, dtype=np.float64).reshape(3)
    d = np.asarray(direction, dtype=np.float64).reshape(3)
    d = d / np.linalg.norm(d)
    r = np.cross(d, np.asarray(up, dtype=np.float64).reshape(3))
    r = r / np.linalg.norm(r)
    u = np.cross(r, d)
    ty = float(np.tan(0.5 * float(fov_y)))
    tx = ty * float(aspect)
    normals = [-d, d, -r - tx * d, r - tx * d, -u - ty * d, u - ty * d]
    consts = [d @ e + float(near), -(d @ e) - float(far)] + [-(n @ e) for n in normals[2:]]
    return np.ascontiguousarray(np.concatenate([np.stack(normals), np.asarray(consts)[:, None]], axis=1).astype(dtype))


def _region_args(bvh: Bvh, prims, planes, leaf: str, exact: bool, who: str):
    """The checks of the convex-region queries: ((n_prims, 9 or 4) primitives by original id, (n, m, 4) planes flattened to (n, 4 m), m)."""
    torch = _torch()
    if bvh.dim != 3:
        raise TypeError(f"{who}: 3D trees only")
    if leaf not in ("tri", "sphere"):
        raise ValueError(f"{who}: leaf must be 'tri' or 'sphere'")
    if exact and leaf != "tri":
        raise ValueError(f"{who}: exact is a triangle test (spheres have the plane-by-plane test only)")
    p = bvh._prims_in(prims, 9 if leaf == "tri" else 4, who)
    if not hasattr(planes, "dtype"):
        planes = np.asarray(planes)
    if len(planes.shape) != 3 or planes.shape[2] != 4 or not 1 <= planes.shape[1] <= REGION_MAX_PLANES:
        raise ValueError(f"{who}: planes must be (n, m, 4) with 1 <= m <= {REGION_MAX_PLANES}")
    m = int(planes.shape[1])
    if isinstance(planes, np.ndarray):
        planes = torch.from_numpy(np.ascontiguousarray(planes))
    q = bvh._prims_in(planes.reshape(planes.shape[0], 4 * m), 4 * m, who)
    return p, q, m


def region_count(bvh: Bvh, prims, planes, leaf: str = "tri", exact: bool = False, counters: bool = False):
    """For each region (m planes {nx, ny, nz, d} with outward normals: the points with n . x + d <= 0 for all of them), how many of the
    tree's primitives meet it (bvh3X_region_tris / bvh3X_region_spheres without lists): an int32 (n,) tensor; with counters also
    (pairs, primitives tested, leaves). prims: (n_prims, 9) triangles {p0, p1, p2} (what refit_tris takes) or, with leaf="sphere",
    (n_prims, 4) {centre, radius}, indexed by ORIGINAL primitive id; planes: (n, m, 4), 1 <= m <= 8 (pad with {0, 0, 0, 0}).
    The default test rejects a primitive iff it lies wholly outside one plane, which also lists triangles beside an edge or corner of
    the region; exact=True (triangles) lists exactly the triangles that share a point with the region. The batch is never reordered:
    submit tiles in screen order."""
    p, q, m = _region_args(bvh, prims, planes, leaf, exact, "region_count")
    fn = getattr(_lib.load(), f"bvh{bvh._s}_region_{'tris' if leaf == 'tri' else 'spheres'}")
    flags = _REGION_EXACT if exact else 0
    n = q.shape[0]
    call = lambda counts, offsets, ids, ins, cnt: fn(bvh._h, p.data_ptr(), p.shape[0], q.data_ptr(), m, n, flags, counts, offsets, ids, ins, cnt, _stream())
    return _count_only("region_count", call, n, q.device, counters)


def region_search(bvh: Bvh, prims, planes, leaf: str = "tri", exact: bool = False, max_per_query=None, original_ids: bool = False,
                  inside: bool = False, counters: bool = False):
    """For each region, the primitives that meet it (bvh3X_region_tris / bvh3X_region_spheres), in the order the tree fixes (depth-first,
    left child first, ascending index inside a leaf); arguments as for region_count. Returns (offsets, ids) as overlap_search does:
    offsets int64 (n + 1,), region q owns ids[offsets[q]:offsets[q + 1]] (int32 BVH-order indices, or bvh.prim_ids[i] with
    original_ids). With inside=True a uint8 tensor parallel to ids follows: 1 = the primitive lies wholly inside the region, 0 = it
    crosses the boundary (or is a padding slot).
      max_per_query=None: exact lists - a count pass, the offsets on the device, one read of offsets[-1] to size the lists, a fill pass.
      max_per_query=k: one pass, k slots per query (offsets = k * arange(n + 1)), unused slots holding -1 (INVALID); counts (int32,
        untruncated) is appended, telling which lists overflowed.
    With counters, (pairs, primitives tested, leaves) of the pass that wrote the lists is appended last."""
    torch = _torch()
    p, q, m = _region_args(bvh, prims, planes, leaf, exact, "region_search")
    fn = getattr(_lib.load(), f"bvh{bvh._s}_region_{'tris' if leaf == 'tri' else 'spheres'}")
    flags = (8 if original_ids else 0) | (_REGION_EXACT if exact else 0)
    n = q.shape[0]
    # (the inside flags take the place of radius_search's distances: one more array beside ids, written by the fill pass only)
    call = lambda counts, offsets, ids, ins, cnt: fn(bvh._h, p.data_ptr(), p.shape[0], q.data_ptr(), m, n, flags, counts, offsets, ids, ins, cnt, _stream())
    out = _two_pass_lists("region_search", call, n, q.device, max_per_query, counters, torch.uint8 if inside else None)
    return out if inside else out[:2] + out[3:]


def tri_distance(bvh: Bvh, tris9, query_tris, max_distance=float("inf"), original_ids: bool = False, sort_queries=None, counters: bool = False,
                 out=None, query_uv: bool = False):
    """For each query triangle, the nearest triangle of the tree, how far it is and where the two come closest (bvh3X_tri_distance).
    tris9: (n_tris, 9) {p0, p1, p2} indexed by ORIGINAL primitive id, what refit_tris and tri_intersect_count take; query_tris: (n, 9)
    in the same layout; a triangle with collinear or coincident vertices is the segment or point it is (a capsule against a mesh: query
    the segment {a, b, b} and compare t with the radius). max_distance: a float for the whole batch, or an array / tensor of n.
    Returns the (n, 4) tensor of hit records (hits_to_numpy views it), written into `out` if given: prim = BVH-order index
    (bvh.prim_ids[i] with original_ids) or INVALID, t = the distance (0 for every pair tri_intersect_count counts; max_distance on a
    miss), (u, v) = the barycentrics of the closest point on the tree triangle in closest_points' convention. With query_uv also the
    (n, 2) barycentrics of the closest point on the query triangle (0 on a miss); with counters also (pairs, triangles fetched,
    leaves). A NaN query coordinate, a NaN or negative max_distance: a miss. sort_queries: True / False force / forbid reordering
    the batch internally (None: the library decides); records never change."""
    torch = _torch()
    t, q = _tri_intersect_args(bvh, tris9, query_tris, "tri_distance")
    dt = q.dtype
    n = q.shape[0]
    scalar, limits = _per_query_value(max_distance, n, dt, "tri_distance", "max_distance", "distance per query")
    out = _records_out(out, n, dt, q.device, "tri_distance")
    uv = torch.zeros((n, 2), dtype=dt, device=q.device) if query_uv else None
    cnt = _counters(counters, q.device)
    fn = getattr(_lib.load(), f"bvh{bvh._s}_tri_distance")
    _lib.check(fn(bvh._h, t.data_ptr(), t.shape[0], q.data_ptr(), n, scalar, limits.data_ptr() if limits is not None and n else None,
                  int(_sort_flags(sort_queries, original_ids)), out.data_ptr(), uv.data_ptr() if query_uv and n else None,
                  cnt.data_ptr() if counters else None, _stream()), "tri_distance")
    res = (out,) + ((uv,) if query_uv else ()) + ((cnt,) if counters else ())
    return res if len(res) > 1 else out


def tri_intersect_search(bvh: Bvh, tris9, query_tris, max_per_query=None, original_ids: bool = False, skip_shared: bool = False, sort_queries=None,
                         counters: bool = False):
    """For each query triangle, the tree's triangles that intersect it (bvh3X_intersect_tris), in the order the tree fixes (depth-first,
    left child first, ascending index inside a leaf). For a tree built from or refitted to `tris9` this is exactly the brute-force set
    of the pair test, which decides by signs of determinants only (exact wherever the determinants are, e.g. small integers).
    Returns (offsets, ids) as overlap_search does: offsets int64 (n + 1,), query q owns ids[offsets[q]:offsets[q + 1]] (int32
    BVH-order indices, or bvh.prim_ids[i] with original_ids).
      max_per_query=None: exact lists - a count pass, the offsets on the device, one read of offsets[-1] to size the lists, a fill pass.
      max_per_query=k: one pass, k slots per query (offsets = k * arange(n + 1)), unused slots holding -1 (INVALID); returns
        (offsets, ids, counts), counts (int32, untruncated) telling which lists overflowed.
    With counters, (pairs, triangles fetched, leaves) of the pass that wrote the lists is appended to the result."""
    t, q = _tri_intersect_args(bvh, tris9, query_tris, "tri_intersect_search")
    fn = getattr(_lib.load(), f"bvh{bvh._s}_intersect_tris")
    flags = int(_sort_flags(sort_queries, original_ids)) | (_TRI_SKIP_SHARED if skip_shared else 0)
    n = q.shape[0]
    call = lambda counts, offsets, ids, _, cnt: fn(bvh._h, t.data_ptr(), t.shape[0], q.data_ptr(), n, flags, counts, offsets, ids, cnt, _stream())
    out = _two_pass_lists("tri_intersect_search", call, n, q.device, max_per_query, counters)
    return out[:2] + out[3:]                                                        # (no distances)


def self_intersections(bvh: Bvh, tris9, original_ids: bool = True, skip_shared: bool = True, counters: bool = False):
    """Every unordered pair of the tree's triangles that intersect, once (bvh3X_intersect_tris_self): a mesh's self-intersections. An
    (m, 2) int64 device tensor shaped as self_overlaps returns it; with original_ids both columns hold original primitive ids (rows of
    `tris9`), otherwise BVH-order indices with first < second. skip_shared (the default): pairs with a common vertex, a mesh's own
    neighbours, are left out. With counters, (pairs, triangles fetched, leaves) of the fill pass is returned too."""
    torch = _torch()
    t, _ = _tri_intersect_args(bvh, tris9, None, "self_intersections")
    fn = getattr(_lib.load(), f"bvh{bvh._s}_intersect_tris_self")
    n = bvh.prim_count
    flags = (8 if original_ids else 0) | (_TRI_SKIP_SHARED if skip_shared else 0)
    call = lambda counts, offsets, ids, _, cnt: fn(bvh._h, t.data_ptr(), t.shape[0], flags, counts, offsets, ids, cnt, _stream())
    out = _two_pass_lists("self_intersections", call, n, t.device, None, counters)
    offsets, ids = out[0], out[1]
    rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=t.device), offsets[1:] - offsets[:-1])
    if original_ids:
        rows = bvh.device_prim_ids().long()[rows]
    pairs = torch.stack([rows, ids.long()], dim=1)
    return (pairs, out[3]) if counters else pairs


def _geometry_table(geometries, who: str):
    """(struct bvh_amd_geometry3X array, family suffix, torch dtype, what keeps the triangle tensors alive) of a list of (Bvh, prims12)."""
    torch = _torch()
    geometries = list(geometries)
    if not geometries:
        raise ValueError(f"{who}: at least one geometry is needed")
    s = geometries[0][0]._s
    dt = torch.float32 if s[1] == "f" else torch.float64
    table = (_lib.Geometry * len(geometries))()
    keep = []
    for k, (bvh, prims) in enumerate(geometries):
        if bvh._s != s or bvh.dim != 3:
            raise TypeError(f"{who}: geometry {k} belongs to another family than geometry 0 (3D trees of one scalar type only)")
        p = bvh._prims_in(prims, 12, who)
        keep.append(p)
        table[k].bvh, table[k].d_tris12 = bvh._h, p.data_ptr()
    return table, s, dt, keep


def _geometry_ids(geometry_ids, n: int, who: str):
    torch = _torch()
    if geometry_ids is None:
        return None
    g = _dev(geometry_ids).reshape(-1)
    if g.dtype not in (torch.int32, torch.int64, torch.uint8, torch.int16):
        raise TypeError(f"{who}: geometry_ids must be integers")
    if g.shape[0] != n:
        raise ValueError(f"{who}: one geometry id per instance")
    return g.to(torch.int32).contiguous()


def instance_prepare(geometries, transforms, geometry_ids=None):
    """The instances of a two-level scene, ready for a builder or Bvh.refit_boxes (bvh3X_instance_prepare). geometries: a list of
    (Bvh, prims12); transforms: (n, 12) or (n, 3, 4) row-major object-to-world matrices (x_world = M x_object + t); geometry_ids: (n,)
    indices into `geometries` (None: all 0). Returns (world2obj (n, 12), bboxes (n, 6), centers (n, 3)) device tensors: the inverse
    maps (NaN rows: a singular or non-finite transform, the instance is disabled), the conservative world boxes {min, max} of the
    geometries' root boxes, read from the trees as they are now on the current stream, and the boxes' centres."""
    torch = _torch()
    table, s, dt, keep = _geometry_table(geometries, "instance_prepare")
    m = geometries[0][0]._prims_in(transforms, 12, "instance_prepare")
    n = m.shape[0]
    gid = _geometry_ids(geometry_ids, n, "instance_prepare")
    w = torch.empty((n, 12), dtype=dt, device=m.device)
    bb = torch.empty((n, 6), dtype=dt, device=m.device)
    cc = torch.empty((n, 3), dtype=dt, device=m.device)
    fn = getattr(_lib.load(), f"bvh{s}_instance_prepare")
    _lib.check(fn(table, len(table), m.data_ptr(), gid.data_ptr() if gid is not None else None, n, w.data_ptr(), bb.data_ptr(), cc.data_ptr(), _stream()),
               "instance_prepare")
    del keep
    return w, bb, cc


def intersect_instanced(top: Bvh, geometries, world2obj, rays, geometry_ids=None, any_hit: bool = False, robust: bool = False,
                        counters: bool = False, original_ids: bool = False, out=None):
    """Batched rays through a two-level scene (bvh3X_intersect_rays_instanced): `top` is a Bvh built over instance_prepare's boxes (its
    prim ids are instance indices), geometries the list of (Bvh, prims12) and world2obj / geometry_ids what instance_prepare took and
    returned. Per ray the nesting of `intersect`: the top tree is walked, an instance's geometry is walked with the ray carried into
    its object space, every accepted hit shortens the ray for what follows. Returns (hits, instances): the (n, 4) hit records of
    `intersect` (prim = BVH-order index in the hit geometry's tree, or its original id with original_ids) and an int32 (n,) tensor of
    instance indices (-1 = INVALID on a miss); with counters also (pairs, tests, leaves) summed over both levels."""
    torch = _torch()
    table, s, dt, keep = _geometry_table(geometries, "intersect_instanced")
    if top._s != s:
        raise TypeError("intersect_instanced: the top tree and the geometries must belong to one 3D family")
    w = top._prims_in(world2obj, 12, "intersect_instanced")
    r = top._prims_in(rays, 8, "intersect_instanced")
    n, n_inst = r.shape[0], w.shape[0]
    gid = _geometry_ids(geometry_ids, n_inst, "intersect_instanced")
    if out is None:
        out = torch.empty((n, 4), dtype=dt, device=r.device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.is_contiguous() and out.dtype == dt and out.numel() == 4 * n):
        raise TypeError("intersect_instanced: `out` must be a contiguous (n, 4) device tensor of the trees' scalar type")
    inst = torch.empty(n, dtype=torch.int32, device=r.device)
    cnt = _counters(counters, r.device)
    flags = (RayFlags.ANY_HIT if any_hit else 0) | (RayFlags.ROBUST if robust else 0) | (8 if original_ids else 0)
    fn = getattr(_lib.load(), f"bvh{s}_intersect_rays_instanced")
    _lib.check(fn(top._h, table, len(table), w.data_ptr(), gid.data_ptr() if gid is not None else None, n_inst, r.data_ptr(), n, int(flags),
                  out.data_ptr(), inst.data_ptr(), cnt.data_ptr() if counters else None, _stream()), "intersect_instanced")
    del keep
    return (out, inst, cnt) if counters else (out, inst)


KNN_MAX_K = 64                                  # BVH_AMD_KNN_MAX_K


def knn(bvh: Bvh, prims, points, k: int, max_distance: float = float("inf"), leaf: str = "tri", distances: bool = True,
        original_ids: bool = False, sort_queries=None, counters: bool = False):
    """For each point, the k nearest primitives within max_distance (bvhXX_knn_*), in ascending (distance, BVH-order index) order: the
    k smallest among the primitives the walk tests, which is the brute force's row exactly when distances are computed exactly and
    within rounding of its distances otherwise (a primitive computed nearer than its own box can hide an equal one). prims
    are in BVH order, as for closest_points; points: (n, 3) with the scalar max_distance, or (n, 4) with a per-query radius in column 3
    (max_distance left at its default). Returns (ids, dist, counts): ids int32 (n, k), BVH-order indices (bvh.prim_ids[i] with
    original_ids); dist (n, k) beside them (None without `distances`); counts int32 (n,), the valid entries of each row. The unused
    slots of a row hold -1 (INVALID) and the query's max_distance. With counters, (pairs, tests, leaves) is appended to the result.
    sort_queries: True / False force / forbid reordering the batch internally (None: the library decides)."""
    torch = _torch()
    k = int(k)
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"k must be in [1, {KNN_MAX_K}]")
    q, p, dt = _point_query_args(bvh, prims, points, max_distance, leaf, "knn", "max_distance", float("inf"))
    n = q.shape[0]
    ids = torch.empty((n, k), dtype=torch.int32, device=q.device)
    dist = torch.empty((n, k), dtype=dt, device=q.device) if distances else None
    counts = torch.zeros(n, dtype=torch.int32, device=q.device)
    cnt = _counters(counters, q.device)
    fn = getattr(_lib.load(), f"bvh{bvh._s}_knn_{leaf}")
    _lib.check(fn(bvh._h, p.data_ptr(), q.data_ptr(), n, k, int(_sort_flags(sort_queries, original_ids)), ids.data_ptr(),
                  dist.data_ptr() if distances else None, counts.data_ptr(), cnt.data_ptr() if counters else None, _stream()), "knn")
    out = (ids, dist, counts)
    return out + (cnt,) if counters else out


def hits_to_numpy(hits) -> np.ndarray:
    a = hits.detach().cpu().numpy()
    return a.view(HITF if a.dtype == np.float32 else HITD).reshape(-1)


def reinsertion_stats():
    """(fast, exact) ReinsertionOptimizer iterations run so far in this process (include/bvh_amd.h: bvh_amd_reinsertion_stats)."""
    out = (C.c_uint * 2)()
    _lib.load().bvh_amd_reinsertion_stats(out)
    return int(out[0]), int(out[1])


def last_optimize_profile() -> dict:
    """The calling thread's latest ReinsertionOptimizer run (a High build's optimize step included): iterations, exact heap
    replays among them, pop + push replacements of those replays, GPU milliseconds of the heap kernels."""
    p = _lib.OptimizeProfile()
    _lib.load().bvh_amd_last_optimize_profile(C.byref(p))
    return {"iterations": int(p.iterations), "replayed": int(p.replayed), "replacements": int(p.replacements), "heap_ms": float(p.heap_ms)}


def std_sort_ids(keys):
    """ids sorted exactly like libstdc++'s std::sort(iota, by keys[i] < keys[j]) incl. tie arrangement (int32 tensor)."""
    torch = _torch()
    k = _dev(keys).reshape(-1)
    s = _suffix(k.dtype)
    out = torch.empty(k.shape[0], dtype=torch.int32, device=k.device)
    _lib.check(getattr(_lib.load(), f"bvh_amd_std_sort_ids{s}")(k.data_ptr(), k.shape[0], out.data_ptr(), _stream()), "std_sort_ids")
    return out


def radix_sort_pairs(keys_u32, vals_u32, bits=32):
    """Stable LSD radix sort by the low `bits` bits; returns (keys, vals) as new int32 tensors."""
    torch = _torch()
    k = _dev(keys_u32).to(torch.int32).clone()
    v = _dev(vals_u32).to(torch.int32).clone()
    _lib.check(_lib.load().bvh_amd_radix_sort_pairs_u32(k.data_ptr(), v.data_ptr(), k.shape[0], bits, _stream()), "radix_sort_pairs")
    return k, v


def radix_order(keys_u32, bits=32):
    """The stable order of the keys by their low `bits` bits, as a reordered ray / query batch computes it (int32 tensor)."""
    torch = _torch()
    k = _dev(keys_u32).to(torch.int32).contiguous()
    out = torch.empty(k.shape[0], dtype=torch.int32, device=k.device)
    _lib.check(_lib.load().bvh_amd_radix_order_u32(k.data_ptr(), k.shape[0], bits, out.data_ptr(), _stream()), "radix_order")
    return out
