"""The C++20 mirror's triangle-distance entry point (bvh::v2::amd::tri_distance_batch, host form over the device form):
tests/cpp/tri_distance_amd.cpp compiles with plain g++ against include/ and, on a GPU, prints the records bvh_amd.tri_distance gives on
the same tree, triangles, queries and max distances."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "tri_distance_amd.cpp")


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
    """The program's mesh, queries and max distances, rebuilt here."""
    side = 12
    h = lambda i, j: np.float32(0.1 * np.sin(0.7 * i) * np.cos(0.4 * j))
    f = np.float32
    tris, queries, limits = [], [], []
    for i in range(side):
        for j in range(side):
            a, b = [i, h(i, j), j], [i + 1, h(i + 1, j), j]
            c, d = [i + 1, h(i + 1, j + 1), j + 1], [i, h(i, j + 1), j + 1]
            tris += [a + b + c, a + c + d]
    for k in range(200):
        x, y, z = f(-1.5 + 15.0 * ((k * 37) % 200) / 200.0), f(-0.25 + 1.0 * ((k * 53) % 200) / 200.0), f(-1.5 + 15.0 * ((k * 91) % 200) / 200.0)
        dx, dz = f(-0.5 + 1.0 * ((k * 29) % 200) / 200.0), f(-0.5 + 1.0 * ((k * 71) % 200) / 200.0)
        a, b, c = [x, y, z], [x + dx, y - f(0.25), z + dz], [x - dz, y + f(0.125), z + dx]
        queries.append(a + b + (c if k % 5 else b))
        limits.append(np.inf if k % 3 else 0.25)
    return np.array(tris, dtype=np.float32), np.array(queries, dtype=np.float32), np.array(limits, dtype=np.float32)


def test_tri_distance_program_compiles_with_gxx(tmp_path):
    _compile(str(tmp_path / "tri_distance_amd"))


@pytest.mark.gpu
def test_cpp_tri_distance_equals_python(tmp_path):
    import bvh_amd
    exe = _compile(str(tmp_path / "tri_distance_amd"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    tris, queries, limits = program_batch()
    bb, cc = bvh_amd.tri_bounds(tris)
    bvh = bvh_amd.DefaultBuilder.build(bb, cc, bvh_amd.Config(quality=bvh_amd.Quality.High))
    assert list(bvh.prim_ids) == [int(x) for x in lines[0].split()[1:]]
    hits, uv = bvh_amd.tri_distance(bvh, tris, queries, limits, query_uv=True)
    hits, uv = bvh_amd.hits_to_numpy(hits), uv.cpu().numpy()
    one = bvh_amd.hits_to_numpy(bvh_amd.tri_distance(bvh, tris, queries[:50], 0.5, original_ids=True))
    assert len(lines) == 1 + len(hits) + len(one)
    found = hits["prim"] != 0xFFFFFFFF
    assert 50 < found.sum() < len(hits) and (hits["t"][found] == 0).sum() > 5 and (hits["t"][found] > 0).sum() > 50
    x = lambda s: np.float32(float.fromhex(s))
    for line, hit, bary in zip(lines[1:1 + len(hits)], hits, uv):
        p, t, u, v, s, w = line.split()
        assert int(p) == hit["prim"] and x(t) == hit["t"] and x(u) == hit["u"] and x(v) == hit["v"], (line, hit)
        assert x(s) == bary[0] and x(w) == bary[1], (line, bary)
    for line, hit in zip(lines[1 + len(hits):], one):
        p, t, u, v = line.split()
        assert int(p) == hit["prim"] and x(t) == hit["t"] and x(u) == hit["u"] and x(v) == hit["v"], (line, hit)
