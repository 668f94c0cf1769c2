"""The C++20 mirror's moving-geometry entry points (bvh::v2::amd::refit_boxes / refit_tris / traversal_cost): tests/cpp/refit_prims_amd.cpp
compiles with plain g++ and, on a GPU, the device refit equals the loop a reference user writes inside Bvh::refit(leaf_fn)."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_cpp_mirror import _compile

SRC = os.path.join(ROOT, "tests", "cpp", "refit_prims_amd.cpp")


def test_refit_prims_program_compiles_with_gxx(tmp_path):
    _compile(str(tmp_path / "refit_prims_amd"), SRC)


@pytest.mark.gpu
def test_cpp_refit_from_primitives_equals_the_host_loop(tmp_path):
    exe = _compile(str(tmp_path / "refit_prims_amd"), SRC)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 2 and all(line.endswith("refit_tris == refit_boxes == host loop") for line in lines), r.stdout
    assert lines[0].startswith("float:") and lines[1].startswith("double:")
