"""use_fp32_operator_lines of the C++ mirror (include/cedar/multilevel.h): a five-point cdr2::solver on gallery::poisson with line-xy
relaxation switches the operator and line factors of its levels to single precision and then runs pcg to the tolerance
(tests/cxx/op32_lines.cc).  The cycle is V(1,1): pcg refuses the default V(2,1), which is not symmetric."""
import json
import subprocess

import pytest

from test_cxx_api import build


def test_op32_lines_program_builds(tmp_path):
    build("op32_lines.cc", tmp_path / "op32_lines")


@pytest.mark.gpu
def test_cxx_solver_use_fp32_operator_lines_then_pcg(tmp_path):
    json.dump({"solver": {"relaxation": "line-xy", "cycle": {"nrelax-pre": 1, "nrelax-post": 1}},
               "pcg": {"max-iter": 30, "tol": 1e-10, "stop-test": "rel-l2", "precon": "mg", "nmg-cycles": 1}},
              open(tmp_path / "config.json", "w"))
    exe = tmp_path / "op32_lines"
    build("op32_lines.cc", exe)
    p = subprocess.run([str(exe), str(tmp_path)], check=True, capture_output=True, text=True)
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["nlevels"] >= 4
    assert 0 <= got["default"] <= got["all"]
    # 141 x 129 and 71 x 65 are above the 64 x 64 of the small-level kernels, 36 x 33 and below are not: two levels
    assert got["all"] == got["fp32_levels"] == 2
    assert got["point_call"] == -1  # the _2d call keeps refusing line relaxation
    assert 2 < len(got["h"]) <= 31 and got["h"][-1] < 1e-10
