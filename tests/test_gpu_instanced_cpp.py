"""The C++20 mirror's instanced entry points (bvh::v2::amd::instance_prepare, intersect_instanced_batch<IsAnyHit, IsRobust>):
tests/cpp/instanced_amd.cpp compiles with plain g++ and, on a GPU, its hits equal a brute force written in the program, before and
after every instance moves and the top tree is refitted."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_cpp_mirror import _compile

SRC = os.path.join(ROOT, "tests", "cpp", "instanced_amd.cpp")


def test_instanced_program_compiles_with_gxx(tmp_path):
    _compile(str(tmp_path / "instanced_amd"), SRC)


@pytest.mark.gpu
def test_cpp_instanced_equals_the_brute_force(tmp_path):
    exe = _compile(str(tmp_path / "instanced_amd"), SRC)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 2 and all(line.endswith("intersect_instanced == brute force") for line in lines), r.stdout
    assert lines[0].startswith("float:") and lines[1].startswith("double:")
