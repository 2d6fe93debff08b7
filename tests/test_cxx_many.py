"""solve_many of the C++ mirror (include/cedar/multilevel.h): two right-hand sides on a 27-point 33^3 solver give the
histories solve() gives for each, bit for bit (tests/cxx/many.cc prints them with 17 digits)."""
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FLAGS = ["-std=c++17", "-O1", "-Wall", f"-I{ROOT}/include", f"-L{ROOT}/cedar_amd/lib", "-lcedar_amd", "-L/opt/rocm/lib",
         f"-Wl,-rpath,{ROOT}/cedar_amd/lib", "-Wl,-rpath,/opt/rocm/lib"]


def build(src, exe):
    from cedar_amd import capi  # noqa: F401  (builds libcedar_amd.so if missing)
    subprocess.run(["g++", os.path.join(HERE, "cxx", src)] + FLAGS + ["-o", str(exe)], check=True)


def test_many_program_builds(tmp_path):
    build("many.cc", tmp_path / "many")


@pytest.mark.gpu
def test_solve_many_of_the_cxx_mirror(tmp_path):
    json.dump({"solver": {"max-rhs": 2, "cycle": {"nrelax-pre": 2, "nrelax-post": 1}}}, open(tmp_path / "config.json", "w"))
    exe = tmp_path / "many"
    build("many.cc", exe)
    p = subprocess.run([str(exe), str(tmp_path)], check=True, capture_output=True, text=True)
    got = json.loads(p.stdout.strip().splitlines()[-1])
    for m in (0, 1):
        single, many, it = got["single%d" % m], got["many%d" % m], got["iters"][m]
        assert len(single) > 2 and it == len(single) - 1
        assert many[: it + 1] == single, (m, many, single)
    assert len(got["many0"]) == len(got["many1"]) == max(got["iters"]) + 1
