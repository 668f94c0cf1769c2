"""The C++20 mirror's sphere-cast entry point (bvh::v2::amd::sphere_cast_batch, host form over the device form):
tests/cpp/sphere_cast_amd.cpp compiles with plain g++ against include/ and, on a GPU, prints the records bvh_amd.sphere_cast gives on
the same tree, rays and radii."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "sphere_cast_amd.cpp")


def _compile(out):
    """Against the library as it was built (no rebuild from here)."""
    lib = os.path.join(ROOT, "bvh_amd", "lib")
    assert os.path.exists(os.path.join(lib, "libbvh_amd.so")), "build the library first (python -m bvh_amd.build)"
    cmd = ["g++", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), SRC,
           "-L", lib, "-lbvh_amd", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def program_batch():
    """The program's mesh, rays and radii, rebuilt here."""
    side = 12
    h = lambda i, j: np.float32(0.1 * np.sin(0.7 * i) * np.cos(0.4 * j))
    tris, rays, radii = [], [], []
    for i in range(side):
        for j in range(side):
            a, b = [i, h(i, j), j], [i + 1, h(i + 1, j), j]
            c, d = [i + 1, h(i + 1, j + 1), j + 1], [i, h(i, j + 1), j + 1]
            tris += [a + b + c, a + c + d]
    for k in range(200):
        rays.append([-1.5 + 15.0 * ((k * 37) % 200) / 200.0, 0.5 + 2.0 * ((k * 53) % 200) / 200.0, -1.5 + 15.0 * ((k * 91) % 200) / 200.0,
                     -1.0 + 2.0 * ((k * 29) % 200) / 200.0, -1.0, -1.0 + 2.0 * ((k * 71) % 200) / 200.0, 0.0, np.inf if k % 3 else 1.0])
        radii.append(np.float32(0.125) * np.float32(k % 5))
    return np.array(tris, dtype=np.float32), np.array(rays, dtype=np.float32), np.array(radii, dtype=np.float32)


def test_sphere_cast_program_compiles_with_gxx(tmp_path):
    _compile(str(tmp_path / "sphere_cast_amd"))


@pytest.mark.gpu
def test_cpp_sphere_cast_equals_python(tmp_path):
    import bvh_amd
    exe = _compile(str(tmp_path / "sphere_cast_amd"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    tris, rays, radii = program_batch()
    bb, cc = bvh_amd.tri_bounds(tris)
    bvh = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.High))
    assert list(bvh.prim_ids) == [int(x) for x in lines[0].split()[1:]]
    prims = bvh_amd.precompute_tris(tris, bvh.device_prim_ids())
    hits = bvh_amd.hits_to_numpy(bvh_amd.sphere_cast(bvh, prims, rays, radii))
    one = bvh_amd.hits_to_numpy(bvh_amd.sphere_cast(bvh, prims, rays[:50], 0.25, robust=True))
    want = np.concatenate([hits, one])
    assert len(lines) == 1 + len(want) and 50 < (hits["prim"] != 0xFFFFFFFF).sum() < len(hits)
    for line, hit in zip(lines[1:], want):
        p, t, u, v = line.split()
        assert int(p) == hit["prim"] and np.float32(float.fromhex(t)) == hit["t"], (line, hit)
        assert np.float32(float.fromhex(u)) == hit["u"] and np.float32(float.fromhex(v)) == hit["v"], (line, hit)
