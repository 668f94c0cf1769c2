"""CPU: the TEXT of the primitive-driven refit (bvh_amd/csrc/refit_body.inc: leaf fold, record-half store, ticket climb) compiled for
the host by tests/cpp/refit_body_host.cpp, against a numpy model of the fold (leaf boxes) and the checker's Bvh::refit (inner boxes),
on every golden tree; the signed-zero / NaN behaviour of the fold; the declared / exported entry points; the ISA of the climbing
kernels. The device must produce the same bytes (tests/test_gpu_refit_prims.py)."""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle
from conftest import MODES, ROOT, load_golden, parse_stream
from test_kernel_body_host import _aligned, pair_records, parse_stream2

HARNESS = os.path.join(ROOT, "tests", "cpp", "refit_body_host.cpp")
BOXES3, BOXES2, TRIS = 0, 1, 2


def leaf_boxes(nodes, ids, bb, dim=3):                      # bb: (n, 2 dim) {min, max}, original order
    """box = BBox::make_empty(); for i in [first_id, first_id + prim_count): box.extend(bb[ids[i]]), extend = robust_min / robust_max
    with the accumulated value first (bbox.h:23-27, :40-44, utils.h:41-43): min = min < other ? min : other, so the OTHER value is
    taken whenever the comparison is false — on a tie of +0 and -0, and when either side is a NaN. (The comparison is written in
    exactly this direction; `other < min ? other : min` would agree on ordinary numbers and differ in those two cases.)"""
    idx = nodes["index"].astype(np.uint64); cnt = (idx & 15).astype(np.int64); first = (idx >> 4).astype(np.int64)
    leaves = np.flatnonzero(cnt); fmax = np.finfo(bb.dtype).max
    lo = np.full((len(leaves), dim), fmax, bb.dtype); hi = np.full((len(leaves), dim), -fmax, bb.dtype)
    for k in range(int(cnt.max())):
        ok = (cnt[leaves] > k)[:, None]
        p = ids[np.minimum(first[leaves] + k, len(ids) - 1)].astype(np.int64)
        with np.errstate(invalid="ignore"):
            lo = np.where(ok & ~(lo < bb[p, :dim]), bb[p, :dim], lo)      # min = min < other ? min : other
            hi = np.where(ok & ~(hi > bb[p, dim:]), bb[p, dim:], hi)
    out = np.empty((len(leaves), 2 * dim), bb.dtype); out[:, 0::2] = lo; out[:, 1::2] = hi      # node layout {min.x, max.x, ...}
    return leaves, out


def expected_nodes(orc, nodes, ids, bb, dim=3):
    """Leaf boxes from the model, inner boxes from the checker's Bvh::refit: the node array a refit from `bb` must leave."""
    want = nodes.copy()
    leaves, boxes = leaf_boxes(nodes, ids, bb, dim)
    want["bounds"][leaves] = boxes
    tree = orc.from_arrays(want, ids)
    tree.refit()
    return tree.nodes()


def compile_harness(out_dir):
    out = os.path.join(str(out_dir), "librefit_body_host.so")
    cmd = ["g++", "-std=c++20", "-O1", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-strict-aliasing", "-Wall", "-Wextra", "-Wno-unused-parameter",
           "-Wno-unknown-pragmas", "-Werror", "-shared", "-fPIC", "-pthread", HARNESS, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    dll = C.CDLL(out)
    P, Z, I, U = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32
    dll.refit_host_run.restype, dll.refit_host_run.argtypes = I, [I, I, P, P, U, P, Z, P, Z]
    dll.refit_host_fold.restype, dll.refit_host_fold.argtypes = I, [I, I, P, Z, P, Z, Z, U, P]
    return dll


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return compile_harness(tmp_path_factory.mktemp("refit"))


def widen(nodes2):
    """Node<T, 2> (20 / 40 bytes) -> the three-wide nodes the device runs on, z = (+0, +0)."""
    double = nodes2.dtype.itemsize == 40
    out = np.zeros(len(nodes2), dtype=oracle.NODED if double else oracle.NODEF)
    out["bounds"][:, :4] = nodes2["bounds"]
    out["index"] = nodes2["index"]
    return out


def host_refit(dll, nodes3, ids, src, kind):
    """The kernel text over (nodes, pair records) whose boxes were overwritten with junk first: (nodes, records) after the refit,
    and the records before it (index words and padding must come through untouched)."""
    dt = nodes3["bounds"].dtype
    start = nodes3.copy()
    start["bounds"][...] = dt.type(12345.0)                 # nothing of the old boxes may survive
    pairs = _aligned(pair_records(start["bounds"], start["index"]))
    before = pairs.copy()
    work = _aligned(start)
    src = np.ascontiguousarray(src, dtype=dt)
    ids32 = np.ascontiguousarray(ids, dtype=np.uint32)
    assert dll.refit_host_run(int(dt == np.float64), kind, _p(work), _p(pairs), len(work), _p(src), len(src), _p(ids32), len(ids32)) == 0
    return work, pairs, before


def check(dll, orc, nodes, ids, bb, kind, src, dim=3):
    want = expected_nodes(orc, nodes, ids, bb, dim)
    nodes3 = nodes if dim == 3 else widen(nodes)
    want3 = want if dim == 3 else widen(want)
    got, pairs, before = host_refit(dll, nodes3, ids, src, kind)
    assert got.tobytes() == want3.tobytes()
    n_pairs = (len(nodes3) - 1) // 2
    assert pairs.tobytes() == pair_records(want3["bounds"], want3["index"]).tobytes()
    assert (pairs["li"] == before["li"]).all() and (pairs["ri"] == before["ri"]).all() and not pairs["pad"][:n_pairs].any()
    return want


def moved(prims, seed, sphere):
    """Every primitive displaced by up to 2 % of the scene extent (per vertex for triangles, per centre for spheres / circles)."""
    rng = np.random.default_rng(seed)
    p = prims.astype(np.float64)
    if sphere:
        d = p.shape[1] - 1
        ext = float((p[:, :d].max(0) - p[:, :d].min(0)).max())
        p[:, :d] += (rng.random((len(p), d)) - 0.5) * 0.04 * ext
    else:
        v = p.reshape(-1, 3)
        ext = float((v.max(0) - v.min(0)).max())
        p = (v + (rng.random(v.shape) - 0.5) * 0.04 * ext).reshape(-1, 9)
    return p.astype(prims.dtype)


GOLDEN_3D = ["cornell", "soup2k", "terrain2k", "soup2k_f64", "spheres2k_f64"]


@pytest.mark.parametrize("scene", GOLDEN_3D)
@pytest.mark.parametrize("mode", [m[0] for m in MODES])
def test_fold_and_climb_equal_model_and_reference_3d(dll, orc, scene, mode):
    g = load_golden(scene)
    double = g["prims"].dtype == np.float64
    nodes, ids = parse_stream(g[f"bvh_{mode}"].tobytes(), double)
    sphere = "spheres" in scene
    # identity: the build's own boxes give back the built tree, bit for bit
    want = check(dll, orc, nodes, ids, g["bboxes"], BOXES3, g["bboxes"])
    assert want.tobytes() == nodes.tobytes()
    if not sphere:
        check(dll, orc, nodes, ids, g["bboxes"], TRIS, g["prims"])
    # moved
    prims = moved(g["prims"], 7, sphere)
    bb = orc.sphere_bboxes(prims)[0] if sphere else orc.prep_tris(prims)[0]
    want = check(dll, orc, nodes, ids, bb, BOXES3, bb)
    assert want.tobytes() != nodes.tobytes()
    assert (want["bounds"][0, 0::2] == bb[:, :3].min(0)).all() and (want["bounds"][0, 1::2] == bb[:, 3:].max(0)).all()
    if not sphere:
        check(dll, orc, nodes, ids, bb, TRIS, prims)


@pytest.mark.parametrize("scene", ["circles2k_2f", "circles2k_2d"])
@pytest.mark.parametrize("mode", ["binned", "sweep", "serial_low", "serial_med", "serial_high"])
def test_fold_and_climb_equal_model_and_reference_2d(dll, orc, scene, mode):
    """Node<T, 2>: the device runs three wide; z stays (+0, +0) in every node and record."""
    g = load_golden(scene)
    double = g["prims"].dtype == np.float64
    nodes, ids = parse_stream2(g[f"bvh_{mode}"].tobytes(), double)
    want = check(dll, orc, nodes, ids, g["bboxes"], BOXES2, g["bboxes"], dim=2)
    assert want.tobytes() == nodes.tobytes()
    circles = moved(g["prims"], 9, True)
    bb = orc.sphere_bboxes(circles)[0]
    want = check(dll, orc, nodes, ids, bb, BOXES2, bb, dim=2)
    assert want.tobytes() != nodes.tobytes()
    got, pairs, _ = host_refit(dll, widen(nodes), ids, bb, BOXES2)
    zeros = np.zeros(2, dtype=bb.dtype).tobytes()           # +0, +0: not -0
    assert all(row.tobytes() == zeros for row in got["bounds"][:, 4:]) and all(row.tobytes() == zeros for row in pairs["lb"][:, 4:])


def _fold(dll, bb, ids, kind=BOXES3):
    out = np.zeros(6, dtype=bb.dtype)
    ids32 = np.ascontiguousarray(ids, dtype=np.uint32)
    bb = np.ascontiguousarray(bb)
    assert dll.refit_host_fold(int(bb.dtype == np.float64), kind, _p(bb), len(bb), _p(ids32), len(ids32), 0, len(ids32), _p(out)) == 0
    return out


def _one_leaf(dtype, n):
    nodes = np.zeros(1, dtype=oracle.NODED if dtype == np.float64 else oracle.NODEF)
    nodes["index"] = n                                       # first_id 0, prim_count n
    return nodes


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fold_signed_zeros(dll, dtype):
    """Which of +0 / -0 a leaf's bound keeps depends on the order the primitives are met in: `acc < other ? acc : other` keeps the
    OTHER on a tie. The kernel text and the model agree for every arrangement, in every component, for every id order."""
    nodes = _one_leaf(dtype, 3)
    for signs in itertools.product([0.0, -0.0], repeat=3):
        for comp in range(3):
            bb = np.zeros((3, 6), dtype=dtype)
            bb[:, :3], bb[:, 3:] = -1.0, 1.0
            bb[:, comp] = signs                              # a minimum that is a zero of either sign
            bb[:, 3 + (comp + 1) % 3] = signs                # ... and a maximum
            for ids in itertools.permutations(range(3)):
                ids = np.array(ids, dtype=np.uint64)
                _, want = leaf_boxes(nodes, ids, bb)
                assert _fold(dll, bb, ids).tobytes() == want[0].tobytes(), (signs, comp, ids)
    # the last zero met wins (ties keep `other`): +0, -0, +0 -> +0 and -0 last -> -0
    bb = np.zeros((3, 6), dtype=dtype)
    bb[:, 3:] = 1.0
    bb[1, 0] = -0.0
    assert not np.signbit(_fold(dll, bb, [0, 1, 2])[0]) and np.signbit(_fold(dll, bb, [0, 2, 1])[0])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fold_nan(dll, dtype):
    """robust_min(acc, other) returns `other` whenever `acc < other` is false: a NaN bound replaces the accumulated value and is
    itself replaced by the next primitive's — so a NaN in the first or middle position vanishes and one in the last stays, exactly
    as in the reference's own loop."""
    nodes = _one_leaf(dtype, 3)
    rng = np.random.default_rng(3)
    for pos in range(3):
        for col in range(6):
            bb = np.sort(rng.random((3, 2, 3)), axis=1).reshape(3, 6).astype(dtype)
            bb[pos, col] = np.nan
            ids = np.arange(3, dtype=np.uint64)
            _, want = leaf_boxes(nodes, ids, bb)
            got = _fold(dll, bb, ids)
            assert got.tobytes() == want[0].tobytes(), (pos, col)
            k = (col % 3) * 2 + col // 3                     # the node-layout slot of input column `col`
            assert np.isnan(got[k]) == (pos == 2) and np.isnan(got).sum() == (pos == 2), (pos, col)
    # triangles: Tri::get_bbox = BBox(p0).extend(p1).extend(p2) by the same rule — a NaN in p0 or p1 vanishes, one in p2 stays
    for vertex in range(3):
        tris = rng.random((3, 9)).astype(dtype)
        tris[1, 3 * vertex] = np.nan
        t = tris.reshape(3, 3, 3)
        lo, hi = t[:, 0].copy(), t[:, 0].copy()
        for k in (1, 2):
            with np.errstate(invalid="ignore"):
                lo = np.where(lo < t[:, k], lo, t[:, k]); hi = np.where(hi > t[:, k], hi, t[:, k])
        bb = np.concatenate([lo, hi], axis=1)
        assert np.isnan(bb).any() == (vertex == 2)
        for ids in ([0, 1, 2], [1, 0, 2], [0, 2, 1]):
            _, want = leaf_boxes(nodes, np.array(ids, dtype=np.uint64), bb)
            assert _fold(dll, tris, ids, TRIS).tobytes() == want[0].tobytes(), (vertex, ids)


def test_fold_skips_what_is_out_of_range(dll):
    """Belt and braces behind the host's refusal: a slot beyond prim_ids or an id beyond the array is never read."""
    bb = np.array([[0, 0, 0, 1, 1, 1], [5, 5, 5, 6, 6, 6]], dtype=np.float32)
    out = np.zeros(6, dtype=np.float32)
    ids = np.array([0, 7, 1], dtype=np.uint32)
    assert dll.refit_host_fold(0, BOXES3, _p(bb), 2, _p(ids), 3, 0, 9, _p(out)) == 0
    assert out.tolist() == [0, 6, 0, 6, 0, 6]


def test_header_declares_and_library_exports_the_refit_entry_points():
    from bvh_amd import _lib, build
    build.build()
    dll = _lib.load()
    header = open(os.path.join(ROOT, "include", "bvh_amd.h")).read()
    declared = set(re.findall(r"BVH_AMD_API[^;]*?\b(bvh\w+)\s*\(", header))
    want = {f"bvh{s}_refit_boxes" for s in ("3f", "3d", "2f", "2d")} | {f"bvh{s}_{f}" for s in ("3f", "3d") for f in ("refit_tris", "traversal_cost")}
    mine = {n for n in declared if n.endswith(("_refit_boxes", "_refit_tris", "_traversal_cost"))}
    assert mine == want
    assert want <= set(_lib.exported_symbols())
    for name in sorted(want):
        assert hasattr(dll, name), name
    for s in ("2f", "2d"):
        assert not hasattr(dll, f"bvh{s}_refit_tris") and not hasattr(dll, f"bvh{s}_traversal_cost")
        assert f"bvh{s}_refit_tris" not in _lib.exported_symbols()


def test_refit_tickets_wait_for_the_waves_own_stores():
    """tests/test_host_logic.py::test_arrival_tickets_wait_for_the_waves_own_stores for the new climbing kernels: the node box (sc1
    stores) and the record half (plain stores) must have been acknowledged before the arrival ticket is issued. Walking back from
    every returning `global_atomic_add`, `s_waitcnt vmcnt(0)` comes before any global access."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_isa import kernel_isa_lines
    from bvh_amd import _lib, build
    build.build()
    assert os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), "llvm-objdump ships with the ROCm that compiled the library: the ISA check must run"
    for scalar in ("float", "double"):
        for src in (BOXES3, BOXES2, TRIS):
            kernel = f"k_refit_prims<{scalar}, {src}>"
            body = kernel_isa_lines(_lib.LIB_PATH, kernel)
            assert body, kernel
            tickets = [i for i, t in enumerate(body) if t.startswith("global_atomic_add") and " sc0" in t]
            assert tickets, (kernel, "no returning atomic add")
            for i in tickets:
                j = i - 1
                while j >= 0 and not body[j].startswith(("global_store", "global_load", "flat_", "buffer_")):
                    if re.match(r"s_waitcnt\s+vmcnt\(0\)", body[j]):
                        break
                    j -= 1
                assert j >= 0 and body[j].startswith("s_waitcnt"), (kernel, body[max(0, i - 8):i + 1])
            assert not any(t.startswith("scratch_") for t in body), kernel          # no spills in the climb
