"""CPU checks of tests/krylov_statement.py, the per-pass reference the GPU suite (test_gpu_krylov.py) compares
krylov.hip with: chained in the order of cedar_amd_solver_pcg the statements reproduce tests/pcg_statement.py, the scalar
rules do what set_alpha / set_rho state on hand-made inputs, and the exact dots are exact."""
import math
from fractions import Fraction

import numpy as np
import pytest

import krylov_statement as ks
import pcg_statement as ps
import problems as pb

V11 = dict(nrelax_pre=1, nrelax_post=1)
CHAIN = [
    ("poisson2-none", lambda: pb.poisson2(31, 27), "none", "rel_l2"),
    ("poisson2-diag", lambda: pb.poisson2(31, 27), "diag", "rel_l2"),
    ("varcoef9-diag", lambda: pb.varcoef9(33, 30, sigma=8.0), "diag", "abs_l2"),
    ("poisson3-none", lambda: pb.poisson3(15, 13, 11), "none", "rel_l2"),
    ("contrast7-diag", lambda: ps.high_contrast7(12, 12, 12), "diag", "rel_l2"),
    ("poisson2-mg", lambda: pb.poisson2(31, 27), "mg", "rel_l2"),
    ("varcoef9-mg", lambda: pb.varcoef9(33, 30, sigma=8.0), "mg", "rel_m"),
    ("poisson3-mg", lambda: pb.poisson3(15, 13, 11), "mg", "abs_m"),
    ("fe3-mg", lambda: pb.fe3(13, 12, 15), "mg", "rel_l2"),
]


@pytest.mark.parametrize("name,mk,precon,stop", CHAIN, ids=[c[0] for c in CHAIN])
def test_chained_passes_reproduce_the_pcg_statement(oracle, name, mk, precon, stop):
    """same iteration count, history equal to 1e-13 relative, for plain, Jacobi and multigrid-preconditioned CG"""
    so = mk()
    g = so.shape[1:]
    b, x0 = ps.random_field(g, 17), ps.random_field(g, 23)
    tol = 1e-9 if stop.startswith("rel") else 1e-9 * np.linalg.norm(ps.inner(b))
    ml = oracle.ml_create(so, **V11) if precon == "mg" else None
    try:
        for max_iter in (3, 600 if precon != "mg" else 40):
            xs, xc = x0.copy(), x0.copy()
            ns, hs = ps.pcg(oracle, so, b, xs, ml=ml, precon=precon, tol=tol, stop=stop, max_iter=max_iter)
            nc, hc = ks.pcg_chained(oracle, so, b, xc, ml=ml, precon=precon, tol=tol, stop=stop, max_iter=max_iter)
            assert nc == ns and len(hc) == len(hs), (name, max_iter, nc, ns)
            assert ns == 3 if max_iter == 3 else 3 < ns < max_iter
            np.testing.assert_allclose(hc, hs, rtol=1e-13, atol=0)
            np.testing.assert_allclose(xc, xs, rtol=1e-12, atol=1e-13 * np.abs(xs).max())
    finally:
        if ml:
            ml.close()


def test_chained_passes_edge_cases(oracle):
    so = pb.poisson2(9, 7)
    g = so.shape[1:]
    n, h = ks.pcg_chained(oracle, so, np.zeros(g), np.zeros(g), precon="none")
    assert n == 0 and h.tolist() == [0.0]
    b, x0 = ps.random_field(g, 3), ps.random_field(g, 4)
    x = x0.copy()
    n, h = ks.pcg_chained(oracle, so, b, x, precon="diag", max_iter=0)
    assert n == 0 and len(h) == 1 and h[0] > 0 and np.array_equal(x, x0)
    # a negative definite operator: sigma < 0 at the first direction, no step taken
    x = x0.copy()
    n, h = ks.pcg_chained(oracle, -so, b, x, precon="none")
    assert n == 0 and len(h) == 1 and np.array_equal(x, x0)


def sc_of(**kw):
    sc = np.array([0.0, 11.0, 12.0, 13.0, 14.0, 15.0, 0.0, 0.0])  # marks in the slots a rule must not touch
    for k, v in kw.items():
        sc[getattr(ks, k.upper())] = v
    return sc


def test_set_alpha_rules():
    sc = ks.set_alpha(4.0, sc_of(rho=3.0))
    assert sc.tolist() == [3.0, 4.0, 0.75, 13.0, 14.0, 15.0, 0.0, 0.0]
    sc = ks.set_alpha(3.0, sc_of(rho=1.0))
    assert sc[ks.ALPHA] == 1.0 / 3.0 and sc[ks.FLAG] == 0.0
    sc = ks.set_alpha(ks.DBL_MAX, sc_of(rho=1.0))  # the largest finite sigma is no breakdown
    assert sc[ks.ALPHA] == 1.0 / ks.DBL_MAX and sc[ks.FLAG] == 0.0
    sc = ks.set_alpha(4.0, sc_of(rho=-3.0))  # a negative rho is the preconditioner's business, not a breakdown
    assert sc[ks.ALPHA] == -0.75 and sc[ks.FLAG] == 0.0
    for sigma in (0.0, -0.0, -1.0, math.inf, -math.inf, math.nan):
        sc = ks.set_alpha(sigma, sc_of(rho=3.0))
        assert sc[ks.ALPHA] == 0.0 and sc[ks.FLAG] == 1.0 and sc[ks.RHO] == 3.0, sigma
        assert sc[ks.SIGMA] == sigma or (math.isnan(sigma) and math.isnan(sc[ks.SIGMA]))  # sigma is stored all the same
        assert sc[[ks.BETA, ks.RR, ks.RZ]].tolist() == [13.0, 14.0, 15.0]
    sc = ks.set_alpha(4.0, sc_of(rho=0.0))
    assert sc[ks.SIGMA] == 4.0 and sc[ks.ALPHA] == 0.0 and sc[ks.FLAG] == 1.0
    sc = ks.set_alpha(4.0, sc_of(rho=3.0, flag=1.0))  # a raised flag stays raised
    assert sc[ks.ALPHA] == 0.75 and sc[ks.FLAG] == 1.0


def test_set_rho_rules():
    # zmode 1 / 2 (has_rz 1): beta = rz / rho_old, then rho = rz
    for zmode in (1, 2):
        sc = ks.update_scalars(zmode, 9.0, 6.0, False, sc_of(rho=4.0))
        assert sc.tolist() == [6.0, 11.0, 12.0, 1.5, 9.0, 6.0, 0.0, 0.0]
    # zmode 0 (has_rz 2): r.z = r.r whatever is handed in
    sc = ks.update_scalars(0, 9.0, 1234.0, False, sc_of(rho=4.0))
    assert sc.tolist() == [9.0, 11.0, 12.0, 2.25, 9.0, 9.0, 0.0, 0.0]
    # zmode 3 (has_rz 0): r.r only
    sc = ks.update_scalars(3, 9.0, 1234.0, False, sc_of(rho=4.0))
    assert sc.tolist() == [4.0, 11.0, 12.0, 13.0, 9.0, 15.0, 0.0, 0.0]
    # first: beta = 0, rho taken over
    sc = ks.update_scalars(2, 9.0, 6.0, True, sc_of(rho=4.0))
    assert sc[ks.BETA] == 0.0 and sc[ks.RHO] == 6.0 and sc[ks.RZ] == 6.0
    # rho_old = 0: beta = 0, no division
    sc = ks.update_scalars(1, 9.0, 6.0, False, sc_of(rho=0.0))
    assert sc[ks.BETA] == 0.0 and sc[ks.RHO] == 6.0 and sc[ks.FLAG] == 0.0
    assert [ks.has_rz_of(z) for z in range(4)] == [2, 1, 1, 0]


def test_rank_order_sum_is_left_to_right():
    g = np.array([1.0, 100.0, 2.0 ** -53, 200.0, 2.0 ** -53, 300.0, -1.0, 400.0])
    assert ks.rank_sum(g, 4, 2, 0) == 0.0  # ((1 + u) + u) - 1 with both u lost; any other order keeps them
    assert ks.rank_sum(g[::-1].copy(), 4, 2, 1) == 2.0 ** -52
    assert ks.rank_sum(g, 4, 2, 1) == 1000.0 and ks.rank_sum(g, 1, 2, 0) == 1.0
    sc = ks.rank_rho(1, g, 4, 2, False, sc_of(rho=10.0))
    assert sc[ks.RR] == 0.0 and sc[ks.RZ] == 1000.0 and sc[ks.BETA] == 100.0 and sc[ks.RHO] == 1000.0
    sc = ks.rank_rho(0, g, 4, 2, False, sc_of(rho=10.0))
    assert sc[ks.RZ] == 0.0 and sc[ks.BETA] == 0.0
    sc = ks.rank_alpha(g, 2, 4, sc_of(rho=2.0))
    assert sc[ks.SIGMA] == 1.0 and sc[ks.ALPHA] == 2.0  # 1 + 2^-53 rounds to 1


def test_exact_dots_are_exact():
    g = (6, 7, 9)
    u = np.floor(pb.uniform(g, 1, -8, 9)) * 0.5
    v = np.floor(pb.uniform(g, 2, -8, 9)) / 8.0
    tot, sab, sh = ks.exact_dot_dyadic(u, v)
    want = sum(Fraction(a) * Fraction(b) for a, b in zip(ks.inner(u).ravel().tolist(), ks.inner(v).ravel().tolist()))
    assert Fraction(tot, 2 ** sh) == want and sab >= abs(tot) and ks.dyadic_value(tot, sh) == float(want)
    with pytest.raises(AssertionError):
        ks.exact_dot_dyadic(u / 3.0, v)
    a, b = pb.uniform(g, 3, -1, 1), pb.uniform(g, 4, -1, 1) * 2.0 ** 20
    s, sab, n = ks.exact_dot_real(a, b)
    fa, fb = ks.inner(a).ravel().tolist(), ks.inner(b).ravel().tolist()
    want = sum(Fraction(p) * Fraction(q) for p, q in zip(fa, fb))
    assert n == 4 * 5 * 7 and s == float(want)  # float(Fraction) rounds correctly, as fsum does
    assert abs(sab - float(sum(abs(Fraction(p) * Fraction(q)) for p, q in zip(fa, fb)))) <= 1e-12 * sab
    # a plain floating-point dot of the same data lies within the any-order bound, a dot without its largest term does not
    t = np.array(fa) * np.array(fb)
    assert abs(float(np.sum(t)) - s) <= ks.any_order_bound(n, sab)
    assert abs(float(np.sum(t)) - t[np.argmax(np.abs(t))] - s) > 1e6 * ks.any_order_bound(n, sab)


def test_array_statements_keep_ghosts_and_rounding_order(oracle):
    g = (7, 8)
    so = pb.random_op(g, 5, 3, zero_ghost=False)
    z, p = pb.uniform(g, 4, -1, 1), pb.uniform(g, 5, -1, 1)
    pn0, w0 = pb.uniform(g, 6, 1, 2), pb.uniform(g, 7, 1, 2)
    pn, w = ks.direction(oracle, so, z, p, pn0, w0, 0.3, False)
    m = pb.interior_mask(g)
    assert np.array_equal(pn[~m], pn0[~m]) and np.array_equal(w[~m], w0[~m])
    assert np.array_equal(pn[m], (z + 0.3 * p)[m])
    # w at a boundary point sees the ghost values of z + beta p, not those of pn
    full = np.zeros(g)
    oracle.matvec2(so, z + 0.3 * p, full)
    assert np.array_equal(w[m], full[m]) and not np.array_equal(w[m], ps.apply_A(oracle, so, pn)[m])
    pn1, _ = ks.direction(oracle, so, z, np.full(g, np.nan), pn0, w0, 0.3, True)
    assert np.array_equal(pn1[m], z[m])
    x, r, d = pb.uniform(g, 8, -1, 1), pb.uniform(g, 9, -1, 1), pb.uniform(g, 10, 1, 3)
    x2, r2, z2 = ks.update(1, True, x, r, pn, w, pn0, d, 0.7)
    assert np.array_equal(x2[m], (x + 0.7 * pn)[m]) and np.array_equal(r2[m], (r - 0.7 * w)[m])
    assert np.array_equal(z2[m], (r2 / d)[m]) and np.array_equal(z2[~m], pn0[~m]) and np.array_equal(x2[~m], x[~m])
    bad = np.full(g, np.inf)
    x3, r3, _ = ks.update(3, True, x, r, bad, np.full(g, np.nan), None, None, 0.0)
    assert np.array_equal(x3, x) and np.array_equal(r3, r)
