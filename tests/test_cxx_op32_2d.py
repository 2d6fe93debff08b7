"""use_fp32_operator_2d of the C++ mirror (include/cedar/multilevel.h): a five-point cdr2::solver on gallery::poisson
switches its operator to single precision and then runs pcg to the tolerance (tests/cxx/op32_2d.cc).  The cycle is
V(1,1): pcg refuses the default V(2,1), which is not symmetric."""
import json
import subprocess

import pytest

from test_cxx_api import build


def test_op32_2d_program_builds(tmp_path):
    build("op32_2d.cc", tmp_path / "op32_2d")


@pytest.mark.gpu
def test_cxx_solver_use_fp32_operator_2d_then_pcg(tmp_path):
    json.dump({"solver": {"cycle": {"nrelax-pre": 1, "nrelax-post": 1}},
               "pcg": {"max-iter": 30, "tol": 1e-10, "stop-test": "rel-l2", "precon": "mg", "nmg-cycles": 1}},
              open(tmp_path / "config.json", "w"))
    exe = tmp_path / "op32_2d"
    build("op32_2d.cc", exe)
    p = subprocess.run([str(exe), str(tmp_path)], check=True, capture_output=True, text=True)
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["nlevels"] >= 4
    assert 0 <= got["default"] <= got["all"]
    assert got["all"] == got["fp32_levels"] == got["nlevels"] - 1  # every smoothed level, the five-point level 0 included
    assert 2 < len(got["h"]) <= 31 and got["h"][-1] < 1e-10
