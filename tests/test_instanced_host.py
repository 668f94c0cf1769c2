"""CPU: the TEXT of the instanced ray kernels (bvh_amd/csrc/instanced_body.inc + point_walk.inc + trace_device.h) compiled for the host
by tests/cpp/instanced_body_host.cpp, one emulated lane per ray / per instance. The two-level walk against a sequential composition of
the CPU checker's own single-level intersect_tri (instanced_scenes.compose): bit-equal records, instances and counters where the walk
order is fixed (a single-leaf top tree), order-free properties under a built top tree; the instance preparation against float64. The
device's results must equal this harness's bit for bit (tests/test_gpu_instanced.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
from conftest import ROOT, load_golden, parse_stream
import instanced_scenes as sc
from instanced_scenes import INVALID, MODES4


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return sc.compile_harness(tmp_path_factory.mktemp("instanced"))


def expect_single_leaf(scene, rays, any_hit, robust, original_ids=False):
    """H1's expectation: the composition in slot order, and one top leaf per ray that is not NaN-flagged."""
    hits, inst, cnt = sc.compose(scene, rays, scene.top_ids, any_hit, robust, original_ids)
    cnt[2] += int((~sc.nan_flagged(np.asarray(rays))).sum())
    return hits, inst, cnt


# ---- H1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_single_leaf_top_tree_equals_the_composition_bit_for_bit(dll, orc, dtype):
    scene = sc.scene12(dll, orc, dtype)
    rays = sc.scene_rays(scene, 1000, seed=5)
    some_hit = False
    for any_hit, robust in MODES4:
        for original_ids in (False, True):
            want, want_inst, want_cnt = expect_single_leaf(scene, rays, any_hit, robust, original_ids)
            got, got_inst, got_cnt = sc.host_walk(scene, rays, any_hit, robust, original_ids)
            assert sc.same_records(got, want), (any_hit, robust, original_ids)
            assert (got_inst == want_inst).all()
            assert (got_cnt == want_cnt).all(), (got_cnt, want_cnt)
            hit = got["prim"] != INVALID
            assert ((got_inst == INVALID) == ~hit).all()
            some_hit |= 300 < hit.sum() < 1000
            # the disabled instance and the one with a geometry index outside the table are never reported
            assert not np.isin(got_inst[hit], [5, 9]).any()
    assert some_hit
    # every usable instance is hit by some ray, through every geometry
    _, inst, _ = sc.host_walk(scene, rays, False, True)
    assert set(inst[inst != INVALID].tolist()) == set(range(12)) - {5, 9}
    # NaN-flagged rays: a miss that reports the ray's own tmax; a NaN / inf origin walks like any ray
    hits, inst, _ = sc.host_walk(scene, rays, False, True)
    flagged = sc.nan_flagged(rays)
    assert flagged.sum() == 2 and (hits["prim"][flagged] == INVALID).all()
    assert hits["t"][flagged].tobytes() == rays[flagged, 7].tobytes()


# ---- H2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene_name", ["soup2k", "soup2k_f64"])
def test_one_identity_instance_reproduces_the_single_level_query(dll, orc, scene_name):
    g = load_golden(scene_name)
    double = g["prims"].dtype == np.float64
    nodes, ids = parse_stream(g["bvh_serial_low"].tobytes(), double)
    geom = sc.Geometry(orc, g["prims"], nodes, ids)
    identity = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).reshape(1, 12)
    scene = sc.Scene(dll, [geom], identity.astype(geom.dtype), None).single_leaf_top()
    assert (scene.world2obj == identity).all()                # (its translation is -0: x + -0 = x for every x)
    for any_hit, robust in MODES4:
        rays = np.ascontiguousarray(g["rays_shadow" if any_hit else "rays_closest"])
        assert not (rays[:, 3:6] == 0).any() and not sc.nan_flagged(rays).any()
        want, want_cnt = geom.cpu.intersect_tri(geom.tris12, rays, any_hit, robust, counters=True)
        got, inst, cnt = sc.host_walk(scene, rays, any_hit, robust)
        assert sc.same_records(got, want), (any_hit, robust)
        assert ((inst == 0) == (got["prim"] != INVALID)).all() and (inst[got["prim"] == INVALID] == INVALID).all()
        assert (cnt == want_cnt + np.array([0, 0, len(rays)], dtype=np.uint64)).all()


# ---- H3 ---------------------------------------------------------------------------------------------------------------------------
def single_triangle_records(orc, scene, rays, inst, prim, robust):
    """For ray k the checker's evaluation of triangle prim[k] of instance inst[k] alone, the ray carried into that instance's space."""
    leaf = np.zeros(1, dtype=oracle.NODED if scene.double else oracle.NODEF)
    leaf[0]["index"] = 1                                      # one leaf: first = 0, count = 1 (the root's box is never tested)
    one = orc.from_arrays(leaf, np.zeros(1, dtype=np.uint64))
    out = np.zeros(len(rays), dtype=oracle.HITD if scene.double else oracle.HITF)
    for k in range(len(rays)):
        geom = scene.geoms[scene.gid(inst[k])]
        local = sc.transform_rays(scene.world2obj[inst[k]], rays[k:k + 1])
        out[k] = one.intersect_tri(geom.tris12[prim[k]:prim[k] + 1], local, True, robust)[0]
    return out


def h3_scene(dll, orc):
    scene = sc.scene200(dll, orc)
    rays = sc.scene_rays(scene, 2000, seed=9)
    forward, _, _ = sc.compose(scene, rays, range(scene.n), False, True)
    backward, _, _ = sc.compose(scene, rays, range(scene.n - 1, -1, -1), False, True)
    # the precondition: the reference alone is insensitive to the order of the instances on these inputs
    assert forward["t"].tobytes() == backward["t"].tobytes() and ((forward["prim"] == INVALID) == (backward["prim"] == INVALID)).all()
    return scene, rays, forward


def check_order_free(orc, scene, rays, common, got, inst, got_any, inst_any):
    """H3's properties of closest-hit records `got` and any-hit records `got_any` against the composition's `common` t."""
    assert got["t"].tobytes() == common["t"].tobytes()
    hit = common["prim"] != INVALID
    assert 500 < hit.sum() < len(rays)
    assert ((got["prim"] != INVALID) == hit).all() and ((inst != INVALID) == hit).all()
    assert (got["u"][~hit] == 0).all() and (got["v"][~hit] == 0).all()
    for i in np.unique(inst[hit]):
        idx = np.nonzero(hit & (inst == i))[0]
        alone, alone_inst, _ = sc.compose(scene, rays[idx], [i], False, True, tmax=common["t"][idx])
        assert (alone_inst == i).all() and sc.same_records(alone, got[idx]), i
    # any-hit: the same rays hit something, and each record is that triangle's own evaluation
    hit_any = got_any["prim"] != INVALID
    assert (hit_any == hit).all() and ((inst_any != INVALID) == hit).all()
    idx = np.nonzero(hit_any)[0]
    single = single_triangle_records(orc, scene, rays[idx], inst_any[idx], got_any["prim"][idx], True)
    assert (single["prim"] == 0).all()
    for f in ("t", "u", "v"):
        assert single[f].tobytes() == np.ascontiguousarray(got_any[f][idx]).tobytes(), f
    assert got_any["t"][~hit_any].tobytes() == rays[~hit_any, 7].tobytes()


def test_built_top_tree_order_free_properties(dll, orc):
    scene, rays, common = h3_scene(dll, orc)
    assert scene.top_depth() >= 4                             # a multi-level top tree
    got, inst, cnt = sc.host_walk(scene, rays, False, True)
    got_any, inst_any, _ = sc.host_walk(scene, rays, True, True)
    check_order_free(orc, scene, rays, common, got, inst, got_any, inst_any)
    assert cnt[0] > 0 and cnt[1] > 0 and cnt[2] > 0


# ---- H4 ---------------------------------------------------------------------------------------------------------------------------
def h4_maps(dtype):
    rng = np.random.default_rng(404)
    maps = []
    for k in range(500):
        t = rng.uniform(-5, 5, size=3) * (1e4 if k % 5 == 1 else 1.0)
        m = sc.affine(rng, t, (0.2, 3.0)).reshape(3, 4)
        if k % 4 == 2:                                        # near-singular: one axis scaled by 1e-3
            m[:, :3] = m[:, :3] @ np.diag(np.roll([1e-3, 1.0, 1.0], k))
        maps.append(m.reshape(12))
    boxes = [np.array([-1, 1, -1, 1, -1, 1.0]), np.array([0.25, 3.5, -2.0, -1.5, 10.0, 10.0]), np.array([-1e3, 2e3, -5.0, 7.0, 0.5, 0.75])]
    gids = rng.integers(0, 3, size=500).astype(np.uint32)
    return np.array(maps).astype(dtype), [b.astype(dtype) for b in boxes], gids


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_instance_boxes_are_conservative_and_tight_and_inverses_accurate(dll, dtype):
    """Inverse: the worst measured |W - inv64(M)|_max / (eps kappa_inf(M) |M^-1|_inf) over these seeds is 0.083 (float32) and 0.135
    (float64) with M the 4 x 4 homogeneous matrix, far below c / 2 = 8, so c stays 16 (about 8 roundings on the longest chain, doubled)."""
    maps, boxes, gids = h4_maps(dtype)
    w, bb, cc = sc.host_prepare(dll, boxes, sc._aligned(maps), gids)
    eps = float(np.finfo(dtype).eps)
    rng = np.random.default_rng(8)
    worst_inverse = worst_pad = 0.0
    for i in range(len(maps)):
        m = maps[i].astype(np.float64).reshape(3, 4)
        box = boxes[gids[i]].astype(np.float64)
        lo, hi = box[0::2], box[1::2]
        corners = np.array([[(hi if (c >> k) & 1 else lo)[k] for k in range(3)] for c in range(8)])
        inner = (lo + (hi - lo) * rng.random((56, 3))).astype(dtype).astype(np.float64)
        pts = np.concatenate([corners, np.clip(inner, lo, hi)])
        image = pts @ m[:, :3].T + m[:, 3]
        out_lo, out_hi = bb[i, :3].astype(np.float64), bb[i, 3:].astype(np.float64)
        assert (image >= out_lo).all() and (image <= out_hi).all(), i
        assert (cc[i] >= bb[i, :3]).all() and (cc[i] <= bb[i, 3:]).all()
        # tight: beyond the exact image of the box by at most 32 eps (sum_j |m_ij| max(|lo_j|, |hi_j|) + |t_i|)
        c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
        exact_c, exact_h = m[:, :3] @ c + m[:, 3], np.abs(m[:, :3]) @ h
        cap = 32 * eps * (np.abs(m[:, :3]) @ np.maximum(np.abs(lo), np.abs(hi)) + np.abs(m[:, 3]))
        pad = np.maximum(out_hi - (exact_c + exact_h), (exact_c - exact_h) - out_lo)
        assert (pad <= cap).all(), (i, pad, cap)
        worst_pad = max(worst_pad, float((pad / cap).max()))
        m4 = np.vstack([m, [0, 0, 0, 1.0]])
        inv4 = np.linalg.inv(m4)
        err = float(np.abs(w[i].astype(np.float64).reshape(3, 4) - inv4[:3]).max())
        bound = eps * np.linalg.cond(m4, np.inf) * np.linalg.norm(inv4, np.inf)
        worst_inverse = max(worst_inverse, err / bound)
    print(f"instance_prepare {np.dtype(dtype).name}: worst inverse error / (eps kappa |M^-1|) = {worst_inverse:.3g}, worst pad / cap = {worst_pad:.3g}")
    assert worst_inverse <= 16


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_disabled_instances_come_out_as_specified(dll, dtype):
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    m = np.stack([eye] * 6)
    m[0, :, 3] = [1, 2, 3]                                    # fine
    m[1, 1, :3] = 0                                           # determinant 0
    m[1, :, 3] = [4, 5, 6]
    m[2, 0, 1] = np.nan                                       # a NaN entry
    m[2, :, 3] = [7, 8, 9]
    m[3, :, 3] = [np.inf, 0, 0]                               # a translation that is not finite
    m[4, 2, 2] = np.inf
    m[4, :, 3] = [-1, -2, -3]
    m[5, :, 3] = [3, 2, 1]                                    # fine, but its geometry index is outside the table
    gids = np.array([0, 0, 0, 0, 0, 4], dtype=np.uint32)
    box = np.array([-1, 1, -2, 2, -3, 3.0], dtype=dtype)
    w, bb, cc = sc.host_prepare(dll, [box], sc._aligned(m.reshape(6, 12).astype(dtype)), gids)
    assert not np.isnan(w[0]).any() and (bb[0] < np.array([0, 0, 0, 2, 4, 6.0])).sum() == 3 and (cc[0] == [1, 2, 3]).all()
    for i, at in ((1, [4, 5, 6]), (2, [7, 8, 9]), (3, [0, 0, 0]), (4, [-1, -2, -3])):
        assert np.isnan(w[i]).all(), i
        assert (bb[i] == np.array(at + at, dtype=dtype)).all() and (cc[i] == np.array(at, dtype=dtype)).all(), i
    assert not np.isnan(w[5]).any() and (bb[5] == np.array([3, 2, 1, 3, 2, 1], dtype=dtype)).all() and (cc[5] == [3, 2, 1]).all()
    assert not np.isnan(bb).any() and not np.isnan(cc).any()


# ---- H5 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [65, 300])
def test_deep_stack_spills_and_equals_the_composition(dll, orc, depth):
    scene, rays, deep_cap = sc.chain_scene(dll, orc, depth)
    assert deep_cap == depth - 62
    for any_hit, robust in MODES4:
        want, want_inst, want_cnt = expect_single_leaf(scene, rays, any_hit, robust)
        got, got_inst, got_cnt = sc.host_walk(scene, rays, any_hit, robust, deep_cap=deep_cap)
        assert sc.same_records(got, want) and (got_inst == want_inst).all() and (got_cnt == want_cnt).all(), (any_hit, robust)
        assert (got["prim"] != INVALID).sum() >= 16
    # closest-hit walks the whole chain: the deepest triangle is the nearest, and every level's record is fetched at least once per ray
    got, _, cnt = sc.host_walk(scene, rays, False, True, deep_cap=deep_cap)
    assert (got["prim"][got["prim"] != INVALID] == depth).any() and cnt[0] >= depth * (got["prim"] != INVALID).sum()


# ---- the C struct ------------------------------------------------------------------------------------------------------------------
def test_geometry_struct_matches_the_c_header(tmp_path):
    """struct bvh_amd_geometry3f / 3d as gcc lays them out (C11, no HIP) against the ctypes structure the binding passes."""
    from bvh_amd import _lib
    src = ["#include <bvh/v2/c_api/bvh.h>", "#include <stddef.h>", "#include <stdio.h>", "int main(void) {"]
    for name in ("bvh_amd_geometry3f", "bvh_amd_geometry3d"):
        src.append(f'    printf("{name} %zu %zu %zu\\n", sizeof(struct {name}), offsetof(struct {name}, bvh), offsetof(struct {name}, d_tris12));')
    src += ["    return 0;", "}"]
    c_file = tmp_path / "layout.c"
    c_file.write_text("\n".join(src) + "\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c_file), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = subprocess.run([str(exe)], capture_output=True, text=True).stdout.strip().splitlines()
    assert len(lines) == 2
    for line in lines:
        got = line.split()
        assert [int(x) for x in got[1:]] == [C.sizeof(_lib.Geometry), _lib.Geometry.bvh.offset, _lib.Geometry.d_tris12.offset], line
    names = _lib.exported_symbols()
    for s in ("3f", "3d"):
        assert f"bvh{s}_instance_prepare" in names and f"bvh{s}_intersect_rays_instanced" in names
    assert "bvh2f_instance_prepare" not in names
