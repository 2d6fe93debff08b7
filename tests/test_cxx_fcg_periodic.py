"""fcg_periodic of the C++ mirror (include/cedar/multilevel.h) on the periodic example configurations
(examples/periodic-config.json: 300 x 300, periodic in x, V(1,1); examples/periodic-config-3d.json: 32^3, periodic in z,
V(2,1)): `history` and x are what Solver.fcg_periodic gives through the C ABI, bit for bit (tests/cxx/fcg_periodic.cc
prints them with 17 digits), while pcg() and fcg() of the same solver refuse."""
import json
import os
import subprocess

import numpy as np
import pytest

import problems as pb
from test_cxx_api import ROOT, build


def test_fcg_periodic_program_builds(tmp_path):
    build("fcg_periodic.cc", tmp_path / "fcg_periodic")


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["periodic-config.json", "periodic-config-3d.json"])
def test_cxx_solver_fcg_periodic(tmp_path, cfg):
    from cedar_amd import capi
    path = os.path.join(ROOT, "examples", cfg)
    conf = json.load(open(path))
    n, per = conf["grid"]["n"], conf["grid"]["periodic"]
    exe = tmp_path / "fcg_periodic"
    build("fcg_periodic.cc", exe)
    p = subprocess.run([str(exe), path], check=True, capture_output=True, text=True)
    got = json.loads(p.stdout.strip().splitlines()[-1])
    sv = conf["solver"]
    st = dict(relax=sv["relaxation"], nrelax_pre=sv["cycle"]["nrelax-pre"], nrelax_post=sv["cycle"]["nrelax-post"],
              max_iter=sv["max-iter"], tol=sv["tol"], min_coarse=sv["min-coarse"])
    if len(n) == 2:
        so = pb.periodic_poisson2(n[0], n[1], per)
        ibc = pb.ibc_of(per)
        i = np.arange(1, n[0] + 1)[None, :]
        j = np.arange(1, n[1] + 1)[:, None]
        rhs = 1.0 / (1.0 + i + 2.0 * j)
    else:
        so = pb.periodic_poisson3(n[0], n[1], n[2], per)
        ibc = pb.ibc3_of(per)
        i = np.arange(1, n[0] + 1)[None, None, :]
        j = np.arange(1, n[1] + 1)[None, :, None]
        k = np.arange(1, n[2] + 1)[:, None, None]
        rhs = 1.0 / (1.0 + i + 2.0 * j + 3.0 * k)
    b = np.zeros(so.shape[1:])
    b[tuple(slice(1, -1) for _ in b.shape)] = rhs
    x = np.zeros_like(b)
    s = capi.Solver(so, ibc=ibc, **st)
    try:
        h = s.fcg_periodic(b, x)  # the library's default settings, as a configuration without pcg.* keys gives
    finally:
        s.close()
    assert got["pcg_len"] == 0 and got["fcg_len"] == 0  # both refuse the periodic solver
    assert got["ghosts_ok"] == 1
    assert 2 < len(h) - 1 < 50 and h[-1] < 1e-8
    assert got["hist"] == h.tolist()
    row = x.reshape(-1, x.shape[-1])[1 if x.ndim == 2 else x.shape[1] + 1]
    assert got["x"] == row.tolist()
