"""The C++20 mirror's all-hits ray entry point (bvh::v2::amd::intersect_all_batch in host and device form):
tests/cpp/intersect_all_amd.cpp compiles with plain g++ and, on a GPU, its lists equal the per-ray walk with a recording leaf_fn."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_cpp_mirror import _compile

SRC = os.path.join(ROOT, "tests", "cpp", "intersect_all_amd.cpp")


def test_intersect_all_program_compiles_with_gxx(tmp_path):
    _compile(str(tmp_path / "intersect_all_amd"), SRC)


@pytest.mark.gpu
def test_cpp_intersect_all_equals_the_per_ray_walk(tmp_path):
    exe = _compile(str(tmp_path / "intersect_all_amd"), SRC)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 3 and all(line.endswith("intersect_all_batch == per-ray walk") for line in lines), r.stdout
    assert lines[0].startswith("float:") and lines[1].startswith("float robust:") and lines[2].startswith("double:")
