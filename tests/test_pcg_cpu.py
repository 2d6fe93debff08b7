"""CPU checks of the PCG reference statement (tests/pcg_statement.py) that the GPU suite (test_gpu_pcg.py) compares
cedar_amd_solver_pcg against: on the oracle, the statement converges, minimises the A-norm of the error at least as
well as the same number of stationary V-cycles, and is plain CG when the preconditioner is the identity."""
import numpy as np
import pytest

import pcg_statement as ps
import problems as pb

CASES = [
    ("poisson2", lambda: pb.poisson2(31, 27), {}),
    ("varcoef9", lambda: pb.varcoef9(33, 30, sigma=8.0), {}),
    ("poisson3", lambda: pb.poisson3(15, 13, 11), {}),
    ("fe3", lambda: pb.fe3(13, 12, 15), {"nrelax_pre": 1, "nrelax_post": 1}),
    ("contrast7", lambda: ps.high_contrast7(16, 16, 16), {}),
]


@pytest.mark.parametrize("name,mk,kw", CASES, ids=[c[0] for c in CASES])
def test_statement_energy_norm_bound(oracle, name, mk, kw):
    """b = A x*, x0 = 0: ||x* - x_k^PCG||_A <= ||x* - x_k^MG||_A for k = 1..6 (CG minimises the A-norm over a Krylov
    space that contains the k-th stationary iterate of a symmetric V-cycle)"""
    so = mk()
    kw = dict({"nrelax_pre": 2, "nrelax_post": 2}, **kw)
    ml = oracle.ml_create(so, **kw)
    try:
        xs = ps.random_field(so.shape[1:], 11)
        b = ps.apply_A(oracle, so, xs)
        xmg = np.zeros_like(b)
        for k in range(1, 7):
            ml.vcycle(xmg, b)
            x = np.zeros_like(b)
            n, _ = ps.pcg(oracle, so, b, x, ml=ml, max_iter=k, tol=0.0)
            assert n == k
            e_pcg, e_mg = ps.a_norm(oracle, so, xs - x), ps.a_norm(oracle, so, xs - xmg)
            assert e_pcg <= (1 + 1e-8) * e_mg, (name, k, e_pcg, e_mg)
    finally:
        ml.close()


@pytest.mark.parametrize("name,mk,kw", CASES[:3], ids=[c[0] for c in CASES[:3]])
def test_statement_converges(oracle, name, mk, kw):
    so = mk()
    ml = oracle.ml_create(so, nrelax_pre=1, nrelax_post=1)
    try:
        b = ps.random_field(so.shape[1:], 5)
        x = np.zeros_like(b)
        n, h = ps.pcg(oracle, so, b, x, ml=ml, tol=1e-10)
        assert h[-1] < 1e-10 and n < 25, (n, h)
        r = b - ps.apply_A(oracle, so, x)
        assert np.linalg.norm(ps.inner(r)) <= 1e-9 * h[0]
    finally:
        ml.close()


def test_statement_unpreconditioned_is_plain_cg(oracle):
    """precon none on 2D Poisson equals a textbook CG on the interior unknowns as a dense matrix"""
    so = pb.poisson2(9, 7)
    g = so.shape[1:]
    n = 9 * 7
    A = np.zeros((n, n))
    for c in range(n):
        e = np.zeros(g)
        ps.inner(e).flat[c] = 1.0
        A[:, c] = ps.inner(ps.apply_A(oracle, so, e)).ravel()
    b = ps.random_field(g, 3)
    x = np.zeros(g)
    it, h = ps.pcg(oracle, so, b, x, precon="none", max_iter=12, tol=0.0)
    bb = ps.inner(b).ravel()
    xx = np.zeros(n)
    r = bb.copy()
    p = r.copy()
    for _ in range(it):
        w = A @ p
        a = (r @ r) / (p @ w)
        xx += a * p
        rn = r - a * w
        p = rn + (rn @ rn) / (r @ r) * p
        r = rn
    np.testing.assert_allclose(ps.inner(x).ravel(), xx, rtol=1e-9, atol=1e-12 * np.abs(xx).max())
