"""pcg_many of the C++ mirror (include/cedar/multilevel.h): three right-hand sides on a 27-point 33^3 solver give the
histories and solutions pcg() gives for each, bit for bit (tests/cxx/pcg_many.cc prints the histories with 17 digits and
compares the solutions itself); a mismatched vector count is reported through log::error."""
import json
import subprocess

import pytest

from test_cxx_many import build


def test_pcg_many_program_builds(tmp_path):
    build("pcg_many.cc", tmp_path / "pcg_many")


@pytest.mark.gpu
def test_pcg_many_of_the_cxx_mirror(tmp_path):
    json.dump({"solver": {"max-rhs": 3, "cycle": {"nrelax-pre": 1, "nrelax-post": 1}},
               "pcg": {"max-iter": 30, "tol": 1e-10, "stop-test": "abs-l2", "precon": "mg", "nmg-cycles": 1}},
              open(tmp_path / "config.json", "w"))
    exe = tmp_path / "pcg_many"
    build("pcg_many.cc", exe)
    p = subprocess.run([str(exe), str(tmp_path)], check=True, capture_output=True, text=True)
    got = json.loads(p.stdout.strip().splitlines()[-1])
    for m in range(3):
        single, many, it = got["single%d" % m], got["many%d" % m], got["iters"][m]
        assert len(single) > 2 and it == len(single) - 1
        assert many == single, (m, many, single)
    assert got["same_x"] is True
    assert len(set(got["iters"])) > 1, got["iters"]  # an absolute target on right-hand sides of different size
    assert got["mismatch_histories"] == 0 and got["mismatch_iterations"] == 0
    assert "pcg_many: b and x must hold the same number" in p.stdout + p.stderr
