"""The C++20 mirror's nearest-hits ray entry point (bvh::v2::amd::intersect_nearest_batch in host and device form):
tests/cpp/intersect_nearest_amd.cpp compiles with plain g++ and, on a GPU, its rows equal the per-ray walk with a recording leaf_fn,
sorted by (t, prim) and cut at k."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_cpp_mirror import _compile

SRC = os.path.join(ROOT, "tests", "cpp", "intersect_nearest_amd.cpp")


def test_intersect_nearest_program_compiles_with_gxx(tmp_path):
    _compile(str(tmp_path / "intersect_nearest_amd"), SRC)


@pytest.mark.gpu
def test_cpp_intersect_nearest_equals_the_sorted_per_ray_walk(tmp_path):
    exe = _compile(str(tmp_path / "intersect_nearest_amd"), SRC)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 3 and all(line.endswith("intersect_nearest_batch == sorted per-ray walk") for line in lines), r.stdout
    assert lines[0].startswith("float:") and lines[1].startswith("float robust:") and lines[2].startswith("double:")
