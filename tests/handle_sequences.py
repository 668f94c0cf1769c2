"""Sequences of operations on ONE BVH handle, run in lockstep on the library and on the reference (test infrastructure: the
generator, the reference model and the executor of tests/test_handle_sequences_host.py and tests/test_gpu_handle_sequences.py).

A handle carries, besides its nodes, about a dozen pieces of derived state ("Derived state of a handle"): the host mirror
and its 2D narrow view, the resident nodes, the traversal records, the root box, the depth that sizes the traversal stack, the
largest primitive id, the measured launch plan. Each is invalidated and refreshed by hand, and a mistake is silent: the handle
answers with the tree of one step ago. So a sequence is 12-16 steps on one handle, and after EVERY step the handle is looked at through
every way there is and compared, byte for byte, with the reference model that took the same steps:

  A  serialize(), serialize_device(), node_count / prim_count, nodes / prim_ids, the 2D accessor view of the root
  B  512 rays, closest and any hit, robust: hit records and the three counters, once with counters and once into an output
     prefilled with a sentinel, as given and reordered, every fourth step on the persistent grid
  C  the queries the reference has no answer for, against a FRESH handle made from the model's arrays: history must not matter

Looking changes the handle: serialize() fills the host mirror, serialize_device() makes the nodes resident and pushes a valid mirror.
So a step looks through everything ("all"), leaves the host mirror alone ("device": the counts, B, C and serialize_device), or leaves
the resident nodes alone too ("records": the counts, B and C), and the paths of a stale mirror and of nodes that are not resident
stay reachable after the first step; a later look shows whether the copies followed. (Three more, for hand-written sequences that
must not wait for the device between two steps: "counts", the counts alone; "cost", traversal_cost alone; "stream", the two streams.)

Two views of the model. bvh_nodeXX_set_bbox edits the host mirror, and the mirror is what serialize(), nodes and (pushed as it is)
serialize_device() and extract_bvh() show: `nodes` has the edit at once. The traversal records have it "at the next refit() /
sync_device()", as the library documents, that is at the next call that re-lays the records out: `rec_nodes` lags until then.

The two sides are reached through adapters (RefAdapter over oracle, GpuAdapter over bvh_amd), so the CPU tests run the executor with
the reference on both sides and with deliberately defective adapters."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import oracle
from test_gpu_fuzz import _rays3
from test_gpu_refit_prims import _wide_array, expected_tree

FAMILIES = ("3f", "3d", "2f", "2d")
SIZES = (1, 2, 3, 17, 65, 300, 2000)
# the kinds that change what the handle holds or which copy of it is current
STATE_KINDS = ("read", "set_bbox", "refit", "optimize", "refit_boxes", "refit_tris", "extract", "roundtrip_host", "roundtrip_device",
               "append_remove", "append_split", "append_chain")
OTHER_KINDS = ("sync_host", "get_node", "refuse_optimize", "refuse_refit")
STARTS = ("build", "from_nodes", "deserialize", "deserialize_device", "wide", "deep")
BUILDS = (("binned", 2, 0), ("sweep", 3, 0), ("serial_low", 0, 0), ("serial_med", 0, 1), ("serial_high", 0, 2),
          ("pool_low", 1, 0), ("pool_med", 1, 1), ("pool_high", 1, 2))
LEAF_LIMITS = ((1, 8), (1, 1), (2, 4), (3, 15), (1, 2))
OPTIMIZE_RATIOS = (0.05, 0.01, 0.3, 1.0, 2.5, 0.0)          # tests/test_gpu_fuzz.py::test_fuzz_configs
OPTIMIZE_ITERS = (0, 1, 2, 3, 4)
CHAIN_PAIRS = 70
N_RAYS = 512
N_QUERIES = 192
SENTINEL = 0xA5                                               # tests/test_gpu_ticket_ranges.py
ERR_ARG, ERR_UNSUPPORTED = -2, -3
REFUSED_OPTIMIZE = (ERR_UNSUPPORTED, "not reachable from the root")
REFUSED_REFIT = (ERR_ARG, "indexed by original primitive id")


def scalar(family):
    return np.float32 if family[1] == "f" else np.float64


def dim_of(family):
    return int(family[0])


# ---------------------------------------------------------------------------------------------------------------- tree facts

def tree_facts(nodes):
    """(reachable node ids, depth of the deepest reachable node, primitives under each node) of a node array."""
    idx = nodes["index"].astype(np.int64)
    cnt, first = idx & 15, idx >> 4
    depth = np.full(len(nodes), -1, np.int64)
    depth[0] = 0
    order, stack = [], [0]
    while stack:
        i = stack.pop()
        order.append(i)
        if cnt[i] == 0:
            for c in (first[i], first[i] + 1):
                depth[c] = depth[i] + 1
                stack.append(int(c))
    under = cnt.copy()
    for i in reversed(order):
        if cnt[i] == 0:
            under[i] = under[first[i]] + under[first[i] + 1]
    return np.array(order, np.int64), int(depth.max()), under


def deep_chain(depth, dtype):
    """tests/test_gpu_traverse.py::test_trees_deeper_than_the_small_stack: depth + 1 stacked triangles, a chain whose inner child is
    always the second of its pair. Returns (triangles, nodes, prim ids)."""
    n = depth + 1
    tris = np.zeros((n, 9), dtype=dtype)
    for k in range(n):
        x = dtype(4000 - k)
        tris[k] = [x, -1, -1, x, 1, -1, x, 0, 1]
    bb = np.concatenate([tris.reshape(n, 3, 3).min(axis=1), tris.reshape(n, 3, 3).max(axis=1)], axis=1)
    nodes = np.zeros(2 * n - 1, dtype=oracle.NODE_DTYPES["3f" if dtype == np.float32 else "3d"])
    suffix = bb.copy()
    for k in range(n - 2, -1, -1):
        suffix[k, :3] = np.minimum(bb[k, :3], suffix[k + 1, :3])
        suffix[k, 3:] = np.maximum(bb[k, 3:], suffix[k + 1, 3:])
    box = lambda b: [b[0], b[3], b[1], b[4], b[2], b[5]]
    nodes[0]["bounds"], nodes[0]["index"] = box(suffix[0]), 1 << 4
    for k in range(n - 1):
        leaf, rest = 2 * k + 1, 2 * k + 2
        nodes[leaf]["bounds"], nodes[leaf]["index"] = box(bb[k]), (k << 4) | 1
        if k == n - 2:
            nodes[rest]["bounds"], nodes[rest]["index"] = box(bb[n - 1]), ((n - 1) << 4) | 1
        else:
            nodes[rest]["bounds"], nodes[rest]["index"] = box(suffix[k + 1]), (2 * k + 3) << 4
    return tris, nodes, np.arange(n, dtype=np.uint64)


# ---------------------------------------------------------------------------------------------------------------- scenes

def make_prims(rng, family, n, lattice):
    """Primitives by original id: (n, 9) triangles for 3D, (n, 3) circles for 2D; finite, on a lattice so that ties occur if asked."""
    dt = scalar(family)
    if dim_of(family) == 3:
        if lattice:
            t = rng.integers(0, 8, size=(n, 1, 3)).astype(dt) + rng.integers(0, 3, size=(n, 3, 3)).astype(dt) * dt(0.5)
        else:
            t = (rng.random((n, 1, 3)) + (rng.random((n, 3, 3)) - 0.5) * 0.1).astype(dt)
        return np.ascontiguousarray(t.reshape(n, 9))
    if lattice:
        ctr = rng.integers(0, 6, size=(n, 2)).astype(dt)
        rad = (rng.integers(0, 3, size=(n, 1)).astype(dt) + 1) * dt(0.25)
    else:
        ctr = rng.random((n, 2)).astype(dt)
        rad = (rng.random((n, 1)) * 0.05 + 0.01).astype(dt)
    return np.ascontiguousarray(np.concatenate([ctr, rad], axis=1))


def moved_prims(prims, family, seed, lattice):
    """The primitives after a seeded move: whole lattice steps on a lattice scene, up to 5 % of the extent otherwise."""
    rng = np.random.default_rng(seed)
    dt, n = prims.dtype.type, len(prims)
    if dim_of(family) == 3:
        v = prims.reshape(n, 3, 3)
        ext = float((v.max(axis=(0, 1)) - v.min(axis=(0, 1))).max()) or 1.0
        d = rng.integers(-1, 2, size=(n, 1, 3)).astype(dt) * dt(0.5) if lattice else ((rng.random((n, 3, 3)) - 0.5) * 0.1 * ext).astype(dt)
        return np.ascontiguousarray((v + d).reshape(n, 9))
    out = prims.copy()
    ext = float((prims[:, :2].max(axis=0) - prims[:, :2].min(axis=0)).max()) or 1.0
    out[:, :2] += rng.integers(-1, 2, size=(n, 2)).astype(dt) if lattice else ((rng.random((n, 2)) - 0.5) * 0.1 * ext).astype(dt)
    return np.ascontiguousarray(out)


def prim_boxes(orc, family, prims):
    """(n, 2 dim) {min, max} boxes and (n, dim) centres of the primitives, by the checker."""
    return orc.prep_tris(prims) if dim_of(family) == 3 else orc.sphere_bboxes(prims)


def prim_bounds(family, prims):
    if dim_of(family) == 3:
        v = prims.reshape(-1, 3).astype(np.float64)
        return v.min(axis=0), v.max(axis=0)
    c, r = prims[:, :2].astype(np.float64), prims[:, 2:3].astype(np.float64)
    return (c - r).min(axis=0), (c + r).max(axis=0)


def rays_for(rng, family, prims):
    r = _rays_around(rng, family, prims)
    # every other ray aimed at a point of some primitive, so that scenes of one or two primitives are hit as well
    dim, pick = dim_of(family), rng.integers(0, len(prims), size=N_RAYS // 2)
    if dim == 3:
        w = rng.dirichlet((1.0, 1.0, 1.0), size=N_RAYS // 2)
        target = (prims[pick].reshape(-1, 3, 3).astype(np.float64) * w[:, :, None]).sum(axis=1)
    else:
        target = prims[pick, :2].astype(np.float64)
    r[::2, dim:2 * dim] = (target - r[::2, :dim].astype(np.float64)).astype(r.dtype)
    return r


def _rays_around(rng, family, prims):
    lo, hi = prim_bounds(family, prims)
    dt = scalar(family)
    if dim_of(family) == 3:
        return _rays3(rng, N_RAYS, lo, hi, dt)
    ext = np.maximum(hi - lo, 1e-3)                             # the 2D counterpart: tests/test_gpu_fuzz.py::test_fuzz_2d
    r = np.zeros((N_RAYS, 6), dtype=dt)
    r[:, 0:2] = lo - 0.2 * ext + rng.random((N_RAYS, 2)) * 1.4 * ext
    d = rng.standard_normal((N_RAYS, 2))
    d[::5, 0] = 0
    d[1::5, 1] = -0.0
    r[:, 2:4] = d
    r[:, 4] = np.where(rng.random(N_RAYS) < 0.1, -2.0, 0.0)
    r[:, 5] = np.where(rng.random(N_RAYS) < 0.3, rng.random(N_RAYS) * ext.max(), np.finfo(dt).max)
    return r


# ---------------------------------------------------------------------------------------------------------------- the reference side

class RefAdapter:
    """The reference model: numpy arrays + oracle.CpuBvh. Also a subject of the executor (the CPU tests run it on both sides)."""

    def __init__(self, orc, family):
        self.orc, self.family, self.dim = orc, family, dim_of(family)
        self.nodes = self.ids = self.rec_nodes = self.prims = None
        self.lattice = False
        self.before = None                                   # (nodes, ids, rec_nodes) before the latest step: what a stale answer would be

    # -- start states
    def reference_start(self, spec, prims):
        """(nodes, prim ids) of the reference for a start state."""
        kind = spec["start"]
        if kind == "deep":
            _, nodes, ids = deep_chain(spec["depth"], scalar(self.family))
            return nodes, ids
        bb, cc = prim_boxes(self.orc, self.family, prims)
        _, builder, quality = spec["build"]
        tree = self.orc.build(bb, cc, builder=builder, quality=quality, min_leaf=spec["leaf"][0], max_leaf=spec["leaf"][1])
        nodes, ids = tree.nodes(), tree.prim_ids()
        if kind == "wide":
            nodes = _wide_array(nodes)
        return nodes, ids

    def start(self, spec, prims, nodes, ids):
        self.prims, self.lattice = prims, spec["lattice"]
        self.nodes, self.ids, self.rec_nodes = nodes.copy(), ids.copy(), nodes.copy()
        self.before = (self.nodes.copy(), self.ids.copy(), self.rec_nodes.copy())

    # -- steps
    def _tree(self, nodes=None):
        return self.orc.from_arrays(self.nodes if nodes is None else nodes, self.ids)

    def _carried(self, nodes):
        self.nodes = nodes
        self.rec_nodes = nodes.copy()

    def _boxes(self, prims):
        return prim_boxes(self.orc, self.family, prims)[0]

    def step(self, st):
        self.before = (self.nodes.copy(), self.ids.copy(), self.rec_nodes.copy())
        return getattr(self, "_" + st["op"])(st)

    def _read(self, st):
        return None

    _sync_host = _get_node = _read

    def _set_bbox(self, st):
        self.nodes["bounds"][st["node"]] = st["box"]
        return None

    def _refit(self, st):
        t = self._tree()
        t.refit()
        self._carried(t.nodes())

    def _optimize(self, st):
        if len(tree_facts(self.nodes)[0]) != len(self.nodes):
            return ("refused",) + REFUSED_OPTIMIZE
        t = self._tree()
        t.optimize(-1, batch_size_ratio=st["ratio"], max_iter_count=st["iters"])
        self._carried(t.nodes())

    _refuse_optimize = _optimize

    def _refit_boxes(self, st):
        moved = moved_prims(self.prims, self.family, st["seed"], self.lattice)
        self._carried(expected_tree(self.orc, self.nodes, self.ids, self._boxes(moved), self.dim).nodes())
        self.prims = moved

    def _refit_tris(self, st):
        self._refit_boxes(st)
        return ("tris", self.orc.precompute_tris(self.prims, self.ids).tobytes())

    def _refuse_refit(self, st):
        assert int(self.ids.max()) >= 1
        return ("refused",) + REFUSED_REFIT

    def _extract(self, st):
        parent = self.serialize()
        child = self._tree().extract(st["root"])
        self.ids = child.prim_ids()
        self._carried(child.nodes())
        return ("parent", parent)

    def _roundtrip_host(self, st):
        self._carried(self.nodes)

    _roundtrip_device = _append_remove = _roundtrip_host

    def _append_split(self, st):
        nodes, leaf = self.nodes, st["leaf"]
        nn = len(nodes)
        index = int(nodes["index"][leaf])
        first, count = index >> 4, index & 15
        extra = np.zeros(2, dtype=nodes.dtype)
        extra["bounds"][:] = nodes["bounds"][leaf]
        extra["index"][0] = (first << 4) | st["left"]
        extra["index"][1] = ((first + st["left"]) << 4) | (count - st["left"])
        nodes = np.concatenate([nodes, extra])
        nodes["index"][leaf] = nn << 4
        self._carried(nodes)

    def _append_chain(self, st):
        nodes, leaf = self.nodes, st["leaf"]
        nn = len(nodes)
        index = nodes["index"][leaf]
        extra = np.zeros(2 * CHAIN_PAIRS, dtype=nodes.dtype)
        extra["bounds"][:] = nodes["bounds"][leaf]
        extra["index"][:] = index                            # every appended leaf repeats the leaf's primitive range
        for p in range(CHAIN_PAIRS - 1):
            extra["index"][2 * p + 1] = (nn + 2 * (p + 1)) << 4
        nodes = np.concatenate([nodes, extra])
        nodes["index"][leaf] = nn << 4
        self.nodes = nodes
        if st["carry"] == "sync_device":
            self._carried(nodes)
        elif st["carry"] == "refit":
            self._refit(st)
        else:
            self._refit_boxes(st)

    # -- looks
    def counts(self):
        return len(self.nodes), len(self.ids)

    def stream(self, nodes, ids):
        idx = np.dtype("<u4" if self.family[1] == "f" else "<u8")
        return np.array([len(nodes), len(ids)], dtype=idx).tobytes() + nodes.tobytes() + ids.astype(idx).tobytes()

    def serialize(self):
        return self.stream(self.nodes, self.ids)

    def serialize_device(self):
        return self.stream(self.nodes, self.ids)

    def arrays(self):
        return self.nodes.tobytes(), self.ids.astype(np.uint64).tobytes()

    def narrow_root(self):
        """(is_leaf, prim_count, first_id, {min, max} box) of node 0 as the 20/40-byte accessors show it."""
        return self._narrow(self.nodes)

    def _narrow(self, nodes):
        index, b = int(nodes["index"][0]), nodes["bounds"][0]
        return (index & 15) != 0, index & 15, index >> 4, tuple(float(v) for v in list(b[0::2]) + list(b[1::2]))

    def ordered_prims(self):
        if self.dim == 3:
            return self.orc.precompute_tris(self.prims, self.ids)
        return np.ascontiguousarray(self.prims[self.ids.astype(np.int64)])

    def trace(self, rays, any_hit, sort_rays, sentinel, persistent):
        """(hit records as bytes, (pairs, tests, leaves)) of the tree the traversal records hold."""
        return self._trace(self.rec_nodes, rays, any_hit)

    def _trace(self, nodes, rays, any_hit):
        t = self._tree(nodes)
        fn = t.intersect_tri if self.dim == 3 else t.intersect_sphere
        hits, cnt = fn(self.ordered_prims(), rays, any_hit, True, threads=1, counters=True)
        return hits.tobytes(), tuple(int(v) for v in cnt)

    def queries(self, pts, boxes, radius, fresh):
        return None                                           # the reference has no answer: check C is between two handles of the library


class StaleMirror(RefAdapter):
    """Defect: nodes / serialize answered from the state before the latest step (a mirror that was not refreshed)."""

    def serialize(self):
        return self.stream(self.before[0], self.before[1])

    def arrays(self):
        return self.before[0].tobytes(), self.before[1].astype(np.uint64).tobytes()


class StaleRecords(RefAdapter):
    """Defect: rays traced through the records of the state before the latest step."""

    def trace(self, rays, any_hit, sort_rays, sentinel, persistent):
        if len(self.before[1]) != len(self.ids) or (self.before[1] != self.ids).any():
            return super().trace(rays, any_hit, sort_rays, sentinel, persistent)
        return self._trace(self.before[2], rays, any_hit)


class DroppedEdit(RefAdapter):
    """Defect: a bvh_nodeXX_set_bbox edit never arrives."""

    def _set_bbox(self, st):
        return None


class StaleNarrow(RefAdapter):
    """Defect: the 2D accessor view is one step behind."""

    def narrow_root(self):
        return self._narrow(self.before[0])


class ExtractMutatesParent(RefAdapter):
    """Defect: extract_bvh changes the handle it is taken from."""

    def _extract(self, st):
        kind, parent = super()._extract(st)
        return kind, parent[:-1] + bytes([parent[-1] ^ 1])


DEFECTS = (StaleMirror, StaleRecords, DroppedEdit, StaleNarrow, ExtractMutatesParent)


# ---------------------------------------------------------------------------------------------------------------- the library side

class GpuAdapter:
    """The handle under test: bvh_amd.Bvh through its Python interface, the node editing through the raw C ABI."""

    def __init__(self, family):
        import bvh_amd
        self.m, self.family, self.dim = bvh_amd, family, dim_of(family)
        self.lib = bvh_amd._lib.load()
        self.bvh = self.prims = self.orc = None               # (orc: the checker the executor works with; it computes the primitives' boxes)
        self.lattice = False
        self.side = None

    def _f(self, name):
        return getattr(self.lib, name.format(S=self.family))

    def start(self, spec, prims, nodes, ids, orc):
        import torch
        m, dt = self.m, scalar(self.family)
        self.prims, self.lattice = prims, spec["lattice"]
        kind = spec["start"]
        if kind == "build":
            bb, cc = prim_boxes(orc, self.family, prims)
            name, builder, quality = spec["build"]
            cfg = m.Config(quality=m.Quality(quality), min_leaf_size=spec["leaf"][0], max_leaf_size=spec["leaf"][1])
            if builder == 2:
                self.bvh = m.BinnedSahBuilder.build(bb, cc, cfg)
            elif builder == 3:
                self.bvh = m.SweepSahBuilder.build(bb, cc, cfg)
            else:
                self.bvh = m.DefaultBuilder.build(bb, cc, cfg, thread_pool=m.ThreadPool() if builder == 1 else None)
        elif kind in ("from_nodes", "wide", "deep"):
            self.bvh = m.Bvh.from_nodes(nodes, ids)
        else:
            idx = np.dtype("<u4" if self.family[1] == "f" else "<u8")
            data = np.array([len(nodes), len(ids)], dtype=idx).tobytes() + nodes.tobytes() + ids.astype(idx).tobytes()
            if kind == "deserialize":
                self.bvh = m.Bvh.deserialize(data, dtype=dt, dim=self.dim)
            else:
                buf = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
                self.bvh = m.Bvh.deserialize_device(buf, dtype=dt, dim=self.dim)

    # -- steps
    def step(self, st):
        return getattr(self, "_" + st["op"])(st)

    def _refusal(self, call):
        try:
            call()
        except self.m.BvhAmdError as exc:
            text = str(exc)
            code = int(text.split("(", 1)[1].split(")", 1)[0])
            return ("refused", code, text)
        return None

    def _read(self, st):
        self.bvh.nodes, self.bvh.prim_ids
        return None

    def _sync_host(self, st):
        self.bvh.sync_host()

    def _get_node(self, st):
        assert self._f("bvh{S}_get_node")(self.bvh._h, 0)

    def _set_bbox(self, st):
        b = st["box"]
        self.bvh.set_node_bbox(st["node"], list(b[0::2]), list(b[1::2]))

    def _refit(self, st):
        self.bvh.refit()

    def _optimize(self, st):
        return self._refusal(lambda: self.bvh.optimize(batch_size_ratio=st["ratio"], max_iter_count=st["iters"]))

    _refuse_optimize = _optimize

    def _on_stream(self, st, call):
        """`call` on the current stream, or on a non-blocking side stream that the current stream then waits for (no host wait)."""
        import torch
        if not st.get("side"):
            return call()
        if self.side is None:
            self.side = torch.cuda.Stream()
        self.side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.side):
            out = call()
        if st.get("wait", True):
            torch.cuda.current_stream().wait_stream(self.side)
        return out

    def _refit_boxes(self, st):
        import torch
        moved = moved_prims(self.prims, self.family, st["seed"], self.lattice)
        bb = torch.from_numpy(prim_boxes(self.orc, self.family, moved)[0]).cuda()
        self._on_stream(st, lambda: self.bvh.refit_boxes(bb))
        self.prims = moved

    def _refit_tris(self, st):
        import torch
        moved = moved_prims(self.prims, self.family, st["seed"], self.lattice)
        d_tris = torch.from_numpy(moved).cuda()
        out = torch.full((self.bvh.prim_count, 12), float("nan"), dtype=d_tris.dtype, device="cuda")
        got = self._on_stream(st, lambda: self.bvh.refit_tris(d_tris, out=out))
        self.prims = moved
        torch.cuda.current_stream().synchronize()
        want = self.m.precompute_tris(d_tris, self.bvh.device_prim_ids())
        assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), "refit_tris: the returned triangles are not precompute_tris(moved, device_prim_ids)"
        return ("tris", got.cpu().numpy().tobytes())

    def _refuse_refit(self, st):
        rows = int(self.bvh.device_prim_ids().max().item())
        bb = prim_boxes(self.orc, self.family, self.prims)[0][:rows]
        return self._refusal(lambda: self.bvh.refit_boxes(bb))

    def _extract(self, st):
        child = self.bvh.extract_bvh(st["root"])
        parent = self.bvh.serialize()
        self.bvh = child
        return ("parent", parent)

    def _roundtrip_host(self, st):
        self.bvh = self.m.Bvh.deserialize(self.bvh.serialize(), dtype=scalar(self.family), dim=self.dim)

    def _roundtrip_device(self, st):
        self.bvh = self.m.Bvh.deserialize_device(self.bvh.serialize_device(), dtype=scalar(self.family), dim=self.dim)

    def _fill(self, i, box, first, count):
        import ctypes as C
        node = self._f("bvh{S}_get_node")(self.bvh._h, i)
        assert node
        ct = C.c_float if self.family[1] == "f" else C.c_double
        self._f("bvh_node{S}_set_bbox")(node, (ct * (2 * self.dim))(*[float(v) for v in list(box[0::2]) + list(box[1::2])]))
        self._f("bvh_node{S}_set_first_id")(node, first)
        self._f("bvh_node{S}_set_prim_count")(node, count)

    def _append(self, n):
        nn = self.bvh.node_count
        for _ in range(n):
            self._f("bvh{S}_append_node")(self.bvh._h)
        assert self.bvh.node_count == nn + n
        return nn

    def _append_remove(self, st):
        nn = self._append(2)
        box = np.arange(2 * self.dim, dtype=np.float64) * 0.25
        self._fill(nn, box, 0, 1)
        self._fill(nn + 1, box, 0, 1)
        for _ in range(2):
            self._f("bvh{S}_remove_last_node")(self.bvh._h)
        assert self.bvh.node_count == nn
        self.bvh.sync_device()

    def _leaf(self, leaf):
        node = self._f("bvh{S}_get_node")(self.bvh._h, leaf)
        first, count = self._f("bvh_node{S}_get_first_id")(node), self._f("bvh_node{S}_get_prim_count")(node)
        b = list(self._f("bvh_node{S}_get_bbox")(node).v)
        box = np.empty(2 * self.dim)
        box[0::2], box[1::2] = b[:self.dim], b[self.dim:]
        return first, count, box

    def _append_split(self, st):
        first, count, box = self._leaf(st["leaf"])
        assert count >= 2
        nn = self._append(2)
        self._fill(nn, box, first, st["left"])
        self._fill(nn + 1, box, first + st["left"], count - st["left"])
        self._fill(st["leaf"], box, nn, 0)
        self.bvh.sync_device()

    def _append_chain(self, st):
        first, count, box = self._leaf(st["leaf"])
        nn = self._append(2 * CHAIN_PAIRS)
        for p in range(CHAIN_PAIRS):
            self._fill(nn + 2 * p, box, first, count)
            if p < CHAIN_PAIRS - 1:
                self._fill(nn + 2 * p + 1, box, nn + 2 * (p + 1), 0)
            else:
                self._fill(nn + 2 * p + 1, box, first, count)
        self._fill(st["leaf"], box, nn, 0)
        if st["carry"] == "sync_device":
            self.bvh.sync_device()
        elif st["carry"] == "refit":
            self.bvh.refit()
        else:
            self._refit_boxes(st)

    # -- looks
    def counts(self):
        return self.bvh.node_count, self.bvh.prim_count

    def serialize(self):
        return self.bvh.serialize()

    def serialize_device(self):
        return self.bvh.serialize_device().cpu().numpy().tobytes()

    def arrays(self):
        return self.bvh.nodes.tobytes(), self.bvh.prim_ids.tobytes()

    def narrow_root(self):
        node = self._f("bvh{S}_get_node")(self.bvh._h, 0)
        assert node
        return (bool(self._f("bvh_node{S}_is_leaf")(node)), self._f("bvh_node{S}_get_prim_count")(node), self._f("bvh_node{S}_get_first_id")(node),
                tuple(float(v) for v in self._f("bvh_node{S}_get_bbox")(node).v))

    def ordered_prims(self, bvh=None):
        bvh = bvh or self.bvh
        if self.dim == 3:
            return self.m.precompute_tris(self.prims, bvh.device_prim_ids())
        return self.m.gather(self.prims, bvh.device_prim_ids())

    def trace(self, rays, any_hit, sort_rays, sentinel, persistent):
        import torch
        m, dt = self.m, scalar(self.family)
        n = len(rays)
        out = None
        if sentinel:
            out = torch.full((n, 4 * np.dtype(dt).itemsize), SENTINEL, dtype=torch.uint8, device="cuda").view(torch.float32 if dt == np.float32 else torch.float64)
        try:
            if persistent:
                self.lib.bvh_amd_experiment(b"one_shot", 0)
            got = m.intersect(self.bvh, self.ordered_prims(), rays, any_hit=any_hit, robust=True, counters=not sentinel, out=out, sort_rays=sort_rays)
            hits, cnt = got if not sentinel else (got, None)
            hits = m.hits_to_numpy(hits).tobytes()
        finally:
            if persistent:
                self.lib.bvh_amd_experiment(b"reset", 0)
        return hits, None if cnt is None else tuple(int(v) for v in cnt.cpu().numpy())

    def queries(self, pts, boxes, radius, fresh):
        """Everything of check C on the aged handle (fresh=None) or on a fresh upload of (nodes, ids): a dict of bytes / numbers."""
        m = self.m
        bvh = self.bvh if fresh is None else m.Bvh.from_nodes(*fresh)
        if self.dim != 3:
            return {}                                         # the point and box queries and traversal_cost are 3D only
        prims = self.ordered_prims(bvh)
        bb = prim_boxes(self.orc, self.family, self.prims)[0]
        raw = lambda t: t.cpu().numpy().tobytes()
        out = {}
        for name, sort in (("flags0", None), ("sorted", True)):
            hits, cnt = m.closest_points(bvh, prims, pts, counters=True, sort_queries=sort)
            out["closest_points", name] = (raw(hits), raw(cnt))
            ids, dist, counts, cnt = m.knn(bvh, prims, pts, 5, counters=True, sort_queries=sort)
            out["knn", name] = (raw(ids), raw(dist), raw(counts), raw(cnt))
            counts, cnt = m.radius_count(bvh, prims, pts, radius, counters=True, sort_queries=sort)
            out["radius_count", name] = (raw(counts), raw(cnt))
            counts, cnt = m.overlap_count(bvh, bb, boxes, counters=True, sort_queries=sort)
            out["overlap_count", name] = (raw(counts), raw(cnt))
        pairs, cnt = m.self_overlaps(bvh, bb, counters=True)
        out["self_overlaps"] = (int(pairs.shape[0]), raw(cnt))
        out["traversal_cost"] = bvh.traversal_cost()
        return out

    def cost(self, fresh):
        bvh = self.bvh if fresh is None else self.m.Bvh.from_nodes(*fresh)
        return bvh.traversal_cost()


# ---------------------------------------------------------------------------------------------------------------- cases

@dataclass
class Case:
    spec: dict
    prims: np.ndarray
    nodes: np.ndarray
    ids: np.ndarray
    steps: list = field(default_factory=list)

    @property
    def id(self):
        return case_id(self.spec)

    @property
    def family(self):
        return self.spec["family"]


def case_id(spec):
    start = spec["start"] if spec["start"] != "deep" else f"deep{spec['depth']}"
    how = spec["build"][0] if spec["start"] != "deep" else "chain"
    return f"{spec['name']}-{spec['family']}-n{spec['n']}-{'lattice' if spec['lattice'] else 'uniform'}-{start}-{how}-s{spec['seed']}"


def needs_growing_stack(case):
    """Sequences whose tree is or becomes deeper than 64 levels trace with the restatement: the compiled reference's harness walks
    with the SmallStack<Index, 64> of the reference's examples."""
    return case.spec["start"] == "deep" or any(st["op"] == "append_chain" for st in case.steps)


def de_bruijn(kinds):
    """A cyclic order of len(kinds)^2 entries in which every ordered pair of kinds is adjacent exactly once (Lyndon words)."""
    k, seq = len(kinds), []
    a = [0] * (2 * 2)

    def db(t, p):
        if t > 2:
            if 2 % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return [kinds[i] for i in seq]


def _spec(name, family, n, seed, start="build", build=BUILDS[2], leaf=(1, 8), lattice=False, depth=0, plan=None, steps=14, cover=False):
    """plan: the kinds of the first steps (the rest is drawn); cover: a sequence laid out for the pair coverage, which keeps its tree large."""
    return {"name": name, "family": family, "n": n, "seed": seed, "start": start, "build": build, "leaf": leaf, "lattice": lattice,
            "depth": depth, "plan": plan, "steps": steps, "cover": cover}


def _committed_specs():
    specs = []
    # 1. every ordered pair of the state-changing kinds as neighbours: a de Bruijn order of the eleven kinds that keep the tree
    #    shallow, cut into overlapping chunks; the twelfth (in-place growth past 64 levels) alternates with all others in two more
    shallow = [k for k in STATE_KINDS if k != "append_chain"]
    order = de_bruijn(shallow)
    order.append(order[0])
    chunk = 13
    for c, at in enumerate(range(0, len(order) - 1, chunk)):
        plan = order[at:at + chunk + 1]
        specs.append(_spec(f"pairs{c}", ("3f", "3d")[c % 2], (300, 2000)[c % 3 == 2], 100 + c, build=BUILDS[c % len(BUILDS)],
                           leaf=((2, 4), (3, 15))[c % 2], lattice=c % 4 == 1, plan=plan, steps=max(len(plan), 12), cover=True))
    half = len(shallow) // 2 + 1
    for c, part in enumerate((shallow[:half], shallow[half:])):
        plan = ["append_chain"] + [k for kind in part for k in (kind, "append_chain")] + (["append_chain"] if c == 0 else [])
        specs.append(_spec(f"growth{c}", ("3f", "3d")[c], 65, 200 + c, leaf=(2, 4), plan=plan, steps=max(len(plan), 12), cover=True))
    # 2. one and two primitives in every family
    for f, family in enumerate(FAMILIES):
        for n in (1, 2):
            specs.append(_spec("tiny", family, n, 300 + 2 * f + n, start=("build", "from_nodes")[(f + n) % 2], build=BUILDS[(f + n) % 5], steps=12))
    # 3. drawn sequences: every start state, every family, every size
    k = 0
    for start in ("build", "from_nodes", "deserialize", "deserialize_device", "wide"):
        for family in FAMILIES:
            n = SIZES[2 + k % 5]
            build = BUILDS[k % (8 if family[0] == "3" else 5)]
            plan = None
            if start == "wide":                              # the refusal, and the documented way out of it
                plan = (["refuse_optimize", "refit_boxes", "extract", "optimize"], ["refit", "extract", "optimize"])[k % 2]
            specs.append(_spec("drawn", family, n, 400 + k, start=start, build=build, leaf=LEAF_LIMITS[k % 5], lattice=k % 3 == 0, plan=plan,
                               steps=12 + k % 5))
            k += 1
    for c, (family, depth) in enumerate((("3f", 65), ("3d", 300), ("3f", 300), ("3d", 65))):
        specs.append(_spec("drawn", family, depth + 1, 500 + c, start="deep", depth=depth, steps=12 + c))
    return specs


SPECS = _committed_specs()


class Generator:
    """Draws the steps of a case while the reference model takes them: what is legal, and with which arguments, comes from the
    model's current arrays (reachability, depth, leaf sizes, primitive ids)."""

    def __init__(self, spec, orc):
        self.spec, self.orc = spec, orc
        self.family, self.dim = spec["family"], dim_of(spec["family"])
        self.rng = np.random.default_rng(spec["seed"])
        self.model = RefAdapter(orc, self.family)
        if spec["start"] == "deep":
            prims = deep_chain(spec["depth"], scalar(self.family))[0]
        else:
            prims = make_prims(self.rng, self.family, spec["n"], spec["lattice"])
        nodes, ids = self.model.reference_start(spec, prims)
        self.model.start(spec, prims, nodes, ids)
        self.case = Case(spec, prims, nodes, ids)
        self.refused = False
        self.used_extract0 = False

    def facts(self):
        nodes = self.model.nodes
        reach, depth, under = tree_facts(nodes)
        cnt = nodes["index"].astype(np.int64) & 15
        return {"reach": reach, "depth": depth, "under": under, "wide": len(reach) != len(nodes),
                "leaves": reach[cnt[reach] > 0], "inner": reach[cnt[reach] == 0], "splittable": reach[cnt[reach] >= 2]}

    def legal(self, f):
        kinds = ["read", "sync_host", "set_bbox", "refit", "refit_boxes", "extract", "roundtrip_host", "roundtrip_device", "append_remove"]
        if self.dim == 2:
            kinds.append("get_node")
        else:
            kinds.append("refit_tris")
            if (f["depth"] < 64 or self.spec["cover"]) and len(self.model.nodes) < 3000:
                kinds.append("append_chain")
        if not f["wide"]:
            kinds.append("optimize")
        elif not self.refused:
            kinds.append("refuse_optimize")
        if len(f["splittable"]):
            kinds.append("append_split")
        if not self.refused and int(self.model.ids.max()) >= 1:
            kinds.append("refuse_refit")
        return kinds

    def draw(self, kind, f, **opts):
        rng, model = self.rng, self.model
        st = {"op": kind}
        if kind == "set_bbox":
            node = int(rng.choice(f["leaves"] if rng.random() < 0.5 or not len(f["inner"]) else f["inner"]))
            b = model.nodes["bounds"][node].astype(np.float64)
            ext = max(float(np.abs(b).max()), 1.0) * 0.25
            lo = b[0::2] - rng.random(self.dim) * ext
            hi = b[1::2] + rng.random(self.dim) * ext
            box = np.empty(2 * self.dim, dtype=scalar(self.family))
            box[0::2], box[1::2] = lo, hi
            st.update(node=node, box=box)
        elif kind in ("optimize", "refuse_optimize"):
            st.update(ratio=float(rng.choice(OPTIMIZE_RATIOS)), iters=int(rng.choice(OPTIMIZE_ITERS)))
        elif kind in ("refit_boxes", "refit_tris"):
            st.update(seed=int(rng.integers(1 << 30)), side=bool(rng.integers(0, 3) == 0))
        elif kind == "extract":
            big = f["inner"][(f["under"][f["inner"]] >= max(4, len(model.ids) // 3)) & (f["inner"] > 0)]
            if f["wide"] and not self.used_extract0:
                root = 0                                      # the documented way to a tree optimize accepts
            elif self.spec["cover"]:                          # (the whole tree once it has grown a chain: a subtree may be the chain alone)
                root = int(rng.choice(big)) if len(big) and f["depth"] < 64 else 0
            else:
                pick = (0, 1, 1, 2, 2, 3)[int(rng.integers(0, 6))]
                pool = (f["leaves"][f["leaves"] > 0], big, f["inner"][f["inner"] > 0], np.array([0]))[pick]
                root = int(rng.choice(pool)) if len(pool) else 0
            self.used_extract0 |= root == 0
            st.update(root=root)
        elif kind == "append_split":
            leaf = int(rng.choice(f["splittable"]))
            st.update(leaf=leaf, left=int(rng.integers(1, int(model.nodes["index"][leaf]) & 15)))
        elif kind == "append_chain":
            st.update(leaf=int(rng.choice(f["leaves"])), carry=("sync_device", "refit", "refit_boxes")[int(rng.integers(0, 3))],
                      seed=int(rng.integers(1 << 30)), side=False)
        st["look"] = ("all", "all", "device", "records")[int(rng.integers(0, 4))]
        st.update(opts)
        return st

    def take(self, kind=None, **opts):
        """Draws (or is told) the next step, and lets the model take it."""
        f = self.facts()
        legal = self.legal(f)
        if kind is None:
            kind = str(self.rng.choice(legal))
        assert kind in legal, f"{case_id(self.spec)}: step {len(self.case.steps)} ({kind}) is not legal here (legal: {legal})"
        st = self.draw(kind, f, **opts)
        out = self.model.step(st)
        refused = out is not None and out[0] == "refused"
        assert refused == kind.startswith("refuse"), (case_id(self.spec), kind, out)
        self.refused |= refused
        self.case.steps.append(st)
        return st

    def run(self):
        plan = list(self.spec["plan"] or [])
        while len(self.case.steps) < self.spec["steps"]:
            self.take(plan.pop(0) if plan else None)
        return self.case


@functools.lru_cache(maxsize=None)
def _restatement():
    return oracle.load_oracle()


@functools.lru_cache(maxsize=None)
def committed_case(index):
    """Case `index` of the committed set (generated with the restatement: the steps do not depend on which checker draws them)."""
    return Generator(SPECS[index], _restatement()).run()


def scripted_case(spec, script):
    """A hand-written sequence: `script` is a list of kinds or (kind, options); arguments a step needs are drawn as usual."""
    g = Generator(spec, _restatement())
    for entry in script:
        kind, opts = (entry, {}) if isinstance(entry, str) else entry
        g.take(kind, **opts)
    return g.case


# ---------------------------------------------------------------------------------------------------------------- the executor

class Mismatch(AssertionError):
    pass


def _same(got, want, case, k, what):
    if got != want:
        op = "start" if k < 0 else case.steps[k]["op"]
        raise Mismatch(f"{case.id}: after step {k} ({op}), {what} differs from the reference")


def execute(case, subject, orc, checks="ABC", log=None):
    """Runs `case` on `subject` and on a reference model over `orc`, with the checks after the start state and after every step.
    Returns the number of executed steps (asserted to be all of them)."""
    family, dim = case.family, dim_of(case.family)
    model = RefAdapter(orc, family)
    model.start(case.spec, case.prims, case.nodes, case.ids)
    subject.orc = orc
    if isinstance(subject, RefAdapter):
        subject.start(case.spec, case.prims, case.nodes, case.ids)
    else:
        subject.start(case.spec, case.prims, case.nodes, case.ids, orc)
    rng = np.random.default_rng(case.spec["seed"] + 77)
    hit = [0]                                                 # closest hits of the reference over the whole sequence

    def look(k, how):
        _same(subject.counts(), model.counts(), case, k, "node_count / prim_count")
        if how == "counts":
            return
        if how == "cost":
            if dim == 3 and "C" in checks and not isinstance(subject, RefAdapter):
                _same(subject.cost(None), subject.cost((model.rec_nodes, model.ids)), case, k, "traversal_cost (aged against fresh)")
            return
        if how == "stream":
            _same(subject.serialize_device(), model.serialize_device(), case, k, "serialize_device()")
            _same(subject.serialize(), model.serialize(), case, k, "serialize()")
            return
        rays = rays_for(rng, family, model.prims)
        if "B" in checks:
            for any_hit in (False, True):
                want = model.trace(rays, any_hit, None, False, False)
                hit[0] += int((np.frombuffer(want[0], dtype=np.uint8).reshape(len(rays), -1)[:, :4].view(np.uint32) != oracle.INVALID).sum())
                for sentinel in (False, True):
                    sort_rays = bool((k + int(sentinel)) % 2)
                    hits, cnt = subject.trace(rays, any_hit, sort_rays, sentinel, persistent=k % 4 == 3)
                    what = f"{'any' if any_hit else 'closest'}-hit, sort_rays={sort_rays}, {'sentinel output' if sentinel else 'counters'}"
                    _same(hits, want[0], case, k, "the hit records (" + what + ")")
                    if cnt is not None:
                        _same(cnt, want[1], case, k, "the counters (" + what + ")")
                    rec = np.frombuffer(hits, dtype=np.uint8).reshape(len(rays), -1)
                    if (rec == SENTINEL).all(axis=1).any():
                        raise Mismatch(f"{case.id}: after step {k}, a hit record keeps the sentinel ({what})")
        if "C" in checks:
            lo, hi = prim_bounds(family, model.prims)
            ext = np.maximum(hi - lo, 1e-3)
            dt = scalar(family)
            pts = (lo - 0.1 * ext + rng.random((N_QUERIES, dim)) * 1.2 * ext).astype(dt)
            qlo = lo + rng.random((N_QUERIES, dim)) * ext
            boxes = np.concatenate([qlo, qlo + rng.random((N_QUERIES, dim)) * 0.2 * ext], axis=1).astype(dt)
            aged = subject.queries(pts, boxes, float(0.15 * ext.max()), None)
            if aged is not None:
                fresh = subject.queries(pts, boxes, float(0.15 * ext.max()), (model.rec_nodes, model.ids))
                for key in fresh:
                    _same(aged[key], fresh[key], case, k, f"{key} (aged handle against a fresh one)")
        if how == "records":
            return
        # A last: what follows may fill the host mirror, and B and C are to see the handle as the step left it
        _same(subject.serialize_device(), model.serialize_device(), case, k, "serialize_device()")
        if how == "all":
            _same(subject.serialize(), model.serialize(), case, k, "serialize()")
            _same(subject.arrays(), model.arrays(), case, k, "nodes / prim_ids")
            if dim == 2:
                _same(subject.narrow_root(), model.narrow_root(), case, k, "the accessor view of the root (get_node(0), get_bbox, get_first_id)")
            _same(subject.serialize_device(), model.serialize_device(), case, k, "serialize_device() once the mirror is valid")

    first = ("all", "device", "records")[case.spec["seed"] % 3]
    look(-1, "device" if first == "all" and case.spec["start"] == "deserialize_device" else first)
    executed = 0
    for k, st in enumerate(case.steps):
        want, got = model.step(st), subject.step(st)
        if want is None:
            _same(got, None, case, k, "the outcome")
        elif want[0] == "refused":
            if got is None or got[0] != "refused" or got[1] != want[1] or want[2] not in got[2]:
                raise Mismatch(f"{case.id}: step {k} ({st['op']}) must be refused with {want[1:]}, got {got}")
        elif want[0] == "parent":
            _same(got, want, case, k, "the parent handle's stream after extract_bvh")
        else:
            _same(got, want, case, k, "the BVH-order triangles refit_tris returned")
        look(k, st.get("look", "all"))
        executed += 1
        if log is not None:
            log.append((k, st["op"], hit[0]))
    assert executed == len(case.steps), (case.id, executed, len(case.steps))
    assert "B" not in checks or hit[0] > 0 or all(st["look"] in ("counts", "cost", "stream") for st in case.steps), f"{case.id}: no ray hit anything in the whole sequence"
    return executed
