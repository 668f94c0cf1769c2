"""The C++20 mirror's winding entry points (bvh::v2::amd::winding_prepare, winding_numbers_batch, signed_distance_batch):
tests/cpp/winding_amd.cpp, compiled with g++ -Wall -Wextra -Werror against the built library, gives the bytes the C ABI gives (through
bvh_amd.winding_numbers / signed_distance) on the same tree."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def cube(side=6):
    """The program's mesh, rebuilt here: the six faces of [0, side]^3, side x side cells each, normals outward."""
    tris = []
    for a in range(3):
        for s in range(2):
            for i in range(side):
                for j in range(side):
                    def corner(di, dj):
                        p = [0.0, 0.0, 0.0]
                        p[a], p[(a + 1) % 3], p[(a + 2) % 3] = s * side, i + di, j + dj
                        return p
                    p00, p10, p11, p01 = corner(0, 0), corner(1, 0), corner(1, 1), corner(0, 1)
                    tris += [p00 + p10 + p11, p00 + p11 + p01] if s else [p00 + p11 + p10, p00 + p01 + p11]
    return np.array(tris, dtype=np.float32)


def test_cpp_mirror_agrees(tmp_path):
    import bvh_amd
    lib = os.path.join(ROOT, "bvh_amd", "lib")
    assert os.path.exists(os.path.join(lib, "libbvh_amd.so"))
    exe = str(tmp_path / "winding_amd")
    cmd = ["g++", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "winding_amd.cpp"),
           "-L", lib, "-lbvh_amd", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    prim_ids = [int(x) for x in lines[0].split()[1:]]
    tris = cube()
    queries = np.array([[np.float32(-1.5 + 9.0 * ((k * 37) % 200) / 200.0), np.float32(-1.5 + 9.0 * ((k * 53) % 200) / 200.0),
                         np.float32(-1.5 + 9.0 * ((k * 91) % 200) / 200.0)] for k in range(200)], dtype=np.float32)
    bb, cc = bvh_amd.tri_bounds(tris)
    bvh = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.High))
    assert list(bvh.prim_ids) == prim_ids
    dprims = bvh_amd.precompute_tris(tris, bvh.device_prim_ids())
    mom = bvh_amd.winding_prepare(bvh, dprims)
    w = bvh_amd.winding_numbers(bvh, dprims, mom, queries).cpu().numpy()
    hits = bvh_amd.hits_to_numpy(bvh_amd.signed_distance(bvh, dprims, mom, queries))
    assert len(lines) == 201
    for line, wk, hit in zip(lines[1:], w, hits):
        lw, p, t, u, v = line.split()
        assert np.float32(float.fromhex(lw)) == wk, (line, wk)
        assert int(p) == hit["prim"] and np.float32(float.fromhex(t)) == hit["t"], (line, hit)
        assert np.float32(float.fromhex(u)) == hit["u"] and np.float32(float.fromhex(v)) == hit["v"], (line, hit)
    inside = ((queries > 0) & (queries < 6)).all(axis=1)
    assert inside.sum() > 20 and (~inside).sum() > 20
    assert (np.rint(w) == inside).all() and ((hits["t"] < 0) == inside).all()
