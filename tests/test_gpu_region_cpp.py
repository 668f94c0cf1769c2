"""The C++20 mirror's convex-region entry points (bvh::v2::amd::region_tris_batch in device and host form, region_spheres_batch):
tests/cpp/region_amd.cpp compiles with plain g++ and, on a GPU, its lists and inside flags equal a brute force written in the program."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_cpp_mirror import _compile

SRC = os.path.join(ROOT, "tests", "cpp", "region_amd.cpp")


def test_region_program_compiles_with_gxx(tmp_path):
    _compile(str(tmp_path / "region_amd"), SRC)


@pytest.mark.gpu
def test_cpp_region_equals_the_brute_force(tmp_path):
    exe = _compile(str(tmp_path / "region_amd"), SRC)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 2 and all(line.endswith("region_tris == region_spheres == brute force") for line in lines), r.stdout
    assert lines[0].startswith("float:") and lines[1].startswith("double:")
