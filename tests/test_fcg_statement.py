"""The numpy statement of flexible CG (tests/fcg_statement.py) on the oracle, without a GPU: it reproduces the PCG statement
where the cycle is symmetric, converges where the cycle is not, and keeps its iteration count where the standard beta
loses half of its.  These are the numbers tests/test_gpu_fcg.py leans on."""
import numpy as np
import pytest

import fcg_statement as fs
import pcg_statement as ps
import problems as pb

SYMMETRIC = [
    ("fe3", lambda: pb.fe3(25, 22, 19)),
    ("poisson3", lambda: pb.poisson3(23, 21, 19)),
    ("contrast7", lambda: ps.high_contrast7(24, 24, 24)),
]


def compare_hist(h, hs, n, ns):
    """the rule of tests/test_gpu_pcg.py"""
    assert abs(n - ns) <= 1, (n, ns, h, hs)
    m = min(len(h), len(hs))
    np.testing.assert_allclose(h[0], hs[0], rtol=1e-10)
    keep = hs[1:m] >= 1e-10
    np.testing.assert_allclose(h[1:m][keep], hs[1:m][keep], rtol=1e-8)


def run(oracle, solver, so, st, **kw):
    g = so.shape[1:]
    b, x = ps.random_field(g, 17), ps.random_field(g, 23)
    ml = oracle.ml_create(so, **st)
    try:
        return solver(oracle, so, b, x, ml=ml, tol=1e-10, max_iter=40, **kw)
    finally:
        ml.close()


@pytest.mark.parametrize("name,mk", SYMMETRIC, ids=[c[0] for c in SYMMETRIC])
def test_symmetric_cycle_reproduces_pcg(oracle, name, mk):
    so = mk()
    st = dict(nrelax_pre=1, nrelax_post=1)
    n, h = run(oracle, fs.fcg, so, st)
    ns, hs = run(oracle, ps.pcg, so, st)
    compare_hist(h, hs, n, ns)
    assert h[-1] < 1e-10


def test_nonsymmetric_cycle_keeps_its_iteration_count(oracle):
    """V(2,0) on 7-point Poisson: 10 iterations with the flexible beta, 20 with the standard one"""
    so = pb.poisson3(23, 21, 19)
    st = dict(nrelax_pre=2, nrelax_post=0)
    n, h = run(oracle, fs.fcg, so, st)
    ns, hs = run(oracle, ps.pcg, so, st)
    assert n <= 11 and h[-1] < 1e-10, (n, h)
    assert ns >= 15, (ns, hs)


@pytest.mark.parametrize("st", [dict(nrelax_pre=2, nrelax_post=1), dict(nrelax_pre=1, nrelax_post=2),
                                dict(nrelax_pre=1, nrelax_post=1, cycle="f"), dict(nrelax_pre=2, nrelax_post=1, cycle="f")],
                         ids=["v21", "v12", "f11", "f21"])
def test_nonsymmetric_cycles_converge(oracle, st):
    """measured: 6, 6, 5, 4 iterations"""
    n, h = run(oracle, fs.fcg, pb.fe3(25, 22, 19), st)
    assert n <= 8 and h[-1] < 1e-10, (n, h)
