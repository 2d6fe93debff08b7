"""solve_many and fcg_periodic_many of the C++ mirror on a periodic 2D solver: examples/periodic-config.json (300^2,
periodic in x, V(1,1)) plus solver.max-rhs: 3 and solver.periodic-batch: true, written to a temporary file.  Histories,
iteration counts and three rows of x spread over the grid (the first, a middle and the last interior row) are what the
Python binding gives on a handle made with periodic_batch2d=True, bit for bit (tests/cxx/periodic_many2d.cc prints them
with 17 digits).  Without the new key the solver holds one right-hand side and both calls are refused, as before."""
import json
import os
import subprocess

import numpy as np
import pytest

import problems as pb
from test_cxx_api import ROOT, build


def test_periodic_many2d_program_builds(tmp_path):
    build("periodic_many2d.cc", tmp_path / "periodic_many2d")


def _config(tmp_path, name, **solver_keys):
    conf = json.load(open(os.path.join(ROOT, "examples", "periodic-config.json")))
    conf["solver"].update(solver_keys)
    path = tmp_path / name
    path.write_text(json.dumps(conf))
    return conf, str(path)


def _run(exe, path):
    p = subprocess.run([str(exe), path], check=True, capture_output=True, text=True)
    return json.loads(p.stdout.strip().splitlines()[-1]), p.stderr


@pytest.mark.gpu
def test_cxx_periodic_many2d(tmp_path):
    from cedar_amd import capi
    exe = tmp_path / "periodic_many2d"
    build("periodic_many2d.cc", exe)
    conf, path = _config(tmp_path, "batch.json", **{"max-rhs": 3, "periodic-batch": True})
    got, _ = _run(exe, path)
    n, per = conf["grid"]["n"], conf["grid"]["periodic"]
    sv = conf["solver"]
    st = dict(relax=sv["relaxation"], nrelax_pre=sv["cycle"]["nrelax-pre"], nrelax_post=sv["cycle"]["nrelax-post"],
              max_iter=sv["max-iter"], tol=sv["tol"], min_coarse=sv["min-coarse"])
    so = pb.periodic_poisson2(n[0], n[1], per)
    i = np.arange(1, n[0] + 1)[None, :]
    j = np.arange(1, n[1] + 1)[:, None]
    b = np.full((3,) + so.shape[1:], -7.5)  # the program's garbage in the ghost layers of b
    b[0, 1:-1, 1:-1] = 1.0 / (1.0 + i + 2.0 * j)
    b[1, 1:-1, 1:-1] = ((i * 7 + j * 13) % 17) - 8.0
    b[2, 1:-1, 1:-1] = 0.125 * (((i * 5 + j * 3) % 7) - 3.0)
    rows = [1, n[1] // 2, n[1]]

    def sample(x):
        return [np.concatenate([x[m][r] for r in rows]).tolist() for m in range(3)]
    s = capi.Solver(so, ibc=pb.ibc_of(per), max_rhs=3, periodic_batch2d=True, **st)
    try:
        assert s.max_rhs() == 3
        x = np.zeros_like(b)
        rel, iters = s.solve_many(b, x)
        assert got["solve_many"]["iters"] == iters and 2 < max(iters) <= st["max_iter"]
        assert got["solve_many"]["hist"] == [r.tolist() for r in rel]
        assert got["solve_many"]["x"] == sample(x)
        x = np.zeros_like(b)
        hist, iters = s.fcg_periodic_many(b, x)  # the library's default settings, as a configuration without pcg.* keys gives
        assert got["fcg_periodic_many"]["iters"] == iters and all(2 < v < 50 for v in iters)
        assert got["fcg_periodic_many"]["hist"] == [h.tolist() for h in hist] and all(h[-1] < 1e-8 for h in hist)
        assert got["fcg_periodic_many"]["x"] == sample(x)
    finally:
        s.close()
    # without solver.periodic-batch: one right-hand side, the batched calls refused, x left as it was
    _, path = _config(tmp_path, "plain.json", **{"max-rhs": 3})
    got, err = _run(exe, path)
    for call in ("solve_many", "fcg_periodic_many"):
        assert got[call]["iters"] == [] and got[call]["hist"] == [], call
        assert all(not any(r) for r in got[call]["x"]), call
    assert "periodic boundary conditions (ibc != 0) are not supported" in err
