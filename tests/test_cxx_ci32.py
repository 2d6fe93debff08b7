"""use_fp32_interpolation of the C++ mirror (include/cedar/multilevel.h): a 7-point cdr3::solver on gallery::poisson
switches the interpolation weights of its grid transfers to single precision and then runs pcg to the tolerance
(tests/cxx/ci32.cc).  The cycle is V(1,1): pcg refuses the default V(2,1), which is not symmetric."""
import json
import subprocess

import pytest

from test_cxx_api import build


def test_ci32_program_builds(tmp_path):
    build("ci32.cc", tmp_path / "ci32")


@pytest.mark.gpu
def test_cxx_solver_use_fp32_interpolation_then_pcg(tmp_path):
    json.dump({"solver": {"cycle": {"nrelax-pre": 1, "nrelax-post": 1}},
               "pcg": {"max-iter": 30, "tol": 1e-10, "stop-test": "rel-l2", "precon": "mg", "nmg-cycles": 1}},
              open(tmp_path / "config.json", "w"))
    exe = tmp_path / "ci32"
    build("ci32.cc", exe)
    p = subprocess.run([str(exe), str(tmp_path)], check=True, capture_output=True, text=True)
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["nlevels"] >= 3
    assert 0 <= got["default"] <= got["all"]
    assert got["all"] == got["fp32_interp_levels"] == got["nlevels"] - 1  # every level pair
    assert got["fp32_levels"] == 0  # the operator switches keep their own count
    assert 2 < len(got["h"]) <= 31 and got["h"][-1] < 1e-10
