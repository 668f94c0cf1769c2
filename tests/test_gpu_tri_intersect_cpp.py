"""The C++20 mirror's triangle-intersection entry points (bvh::v2::amd::intersect_tris_batch in device and host form,
intersect_tris_self_batch): tests/cpp/tri_intersect_amd.cpp compiles with plain g++ and, on a GPU, its lists equal a brute force
written in the program (an integer separating-axis test on integer coordinates)."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_cpp_mirror import _compile

SRC = os.path.join(ROOT, "tests", "cpp", "tri_intersect_amd.cpp")


def test_tri_intersect_program_compiles_with_gxx(tmp_path):
    _compile(str(tmp_path / "tri_intersect_amd"), SRC)


@pytest.mark.gpu
def test_cpp_tri_intersect_equals_the_brute_force(tmp_path):
    exe = _compile(str(tmp_path / "tri_intersect_amd"), SRC)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 2 and all(line.endswith("intersect_tris == intersect_tris_self == brute force") for line in lines), r.stdout
    assert lines[0].startswith("float:") and lines[1].startswith("double:")
