"""fcg of the C++ mirror (include/cedar/multilevel.h): a default-configured 3D solver -- V(2,1), which pcg() refuses --
fills `history` with what Solver.fcg gives through the C ABI (tests/cxx/fcg.cc prints it with 17 digits)."""
import json
import subprocess

import numpy as np
import pytest

import problems as pb
from test_cxx_api import build


def test_fcg_program_builds(tmp_path):
    build("fcg.cc", tmp_path / "fcg")


@pytest.mark.gpu
def test_cxx_solver_fcg(tmp_path):
    from cedar_amd import capi
    json.dump({"pcg": {"max-iter": 30, "tol": 1e-10, "stop-test": "rel-l2", "precon": "mg", "nmg-cycles": 1}},
              open(tmp_path / "config.json", "w"))
    exe = tmp_path / "fcg"
    build("fcg.cc", exe)
    p = subprocess.run([str(exe), str(tmp_path)], check=True, capture_output=True, text=True)
    got = json.loads(p.stdout.strip().splitlines()[-1])
    so = pb.fe3(17, 15, 13)
    b = np.zeros(so.shape[1:])
    i = np.arange(1, 18)[None, None, :]
    j = np.arange(1, 16)[None, :, None]
    k = np.arange(1, 14)[:, None, None]
    b[1:-1, 1:-1, 1:-1] = 1.0 / (1.0 + i + 2.0 * j + 3.0 * k)
    s = capi.Solver(so)  # the defaults: V(2,1)
    h3 = s.fcg(b, np.zeros_like(b), max_iter=30, tol=1e-10)
    s.close()
    assert got["pcg_len"] == 0  # pcg refused the non-symmetric cycle
    assert len(got["h3"]) == len(h3) > 2 and h3[-1] < 1e-10
    np.testing.assert_allclose(got["h3"], h3, rtol=1e-13)
