"""fcg_semidefinite of the C++ mirror (include/cedar/multilevel.h) with the key solver.semidefinite: true on the fully
periodic Poisson operator, 32 x 24 in 2D and 16 x 16 x 8 in 3D (tests/cxx/semidefinite.cc): the right-hand side is not
compatible, the call converges, the residual of the projected system formed on the host is what the history says, x has
zero mean, and pcg() of the same solver refuses."""
import json
import subprocess

import numpy as np
import pytest

from test_cxx_api import build


def test_semidefinite_program_builds(tmp_path):
    build("semidefinite.cc", tmp_path / "semidefinite")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [[32, 24], [16, 16, 8]], ids=str)
def test_cxx_solver_fcg_semidefinite(tmp_path, n):
    tol = 1e-10
    json.dump({"log": ["status", "error"],
               "grid": {"n": n, "periodic": [True] * len(n)},
               "solver": {"semidefinite": True, "relaxation": "point", "cycle": {"nrelax-pre": 2, "nrelax-post": 1},
                          "min-coarse": 3},
               "pcg": {"tol": tol, "max-iter": 40}}, open(tmp_path / "config.json", "w"))
    exe = tmp_path / "semidefinite"
    build("semidefinite.cc", exe)
    p = subprocess.run([str(exe), str(tmp_path / "config.json")], check=True, capture_output=True, text=True)
    got = json.loads(p.stdout.strip().splitlines()[-1])
    h = got["hist"]
    npts = int(np.prod(n))
    assert got["pcg_len"] == 0 and "cedar_amd_solver_fcg_semidefinite" in p.stderr + p.stdout  # pcg refuses the handle
    assert 2 < len(h) - 1 <= 40 and h[-1] < tol
    # |P b - A x| / |P b| against the recurrence's: hist[0] = |P b| (x0 = 0); the host sum rounds differently
    assert abs(got["rel_res"] - h[-1]) <= 0.01 * tol
    assert got["mean_abs_x"] > 0 and abs(got["mean_x"]) <= 2 * npts * np.finfo(float).eps * got["mean_abs_x"]
