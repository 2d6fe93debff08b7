"""The numpy statement of the semidefinite solve (tests/semidefinite_statement.py) on the oracle, without a GPU.

Every case of tests/semidefinite_cases.py -- fully periodic and pure Neumann operators with zero row sums, 2D point and
line relaxation, 3D point relaxation, V(1,1), V(2,1), F(2,1) -- with b = random_field(g, 17), x0 = random_field(g, 23),
relative tolerance 1e-10, at most 40 iterations.  Asserted: the assembled coarsest matrix has zero row sums, the
oracle's coarse solve with the replaced factor solves A_c y = f for a zero-sum f, flexible CG converges, its true
residual is the recurrence's, and it needs no more iterations than the stationary iteration where that one converges.

MEASURED: (flexible CG, stationary iteration; None = not below 1e-10 within 40) as this test prints them (-s).  The table
is a record; the assertions below are on what a run computes.
"""
import numpy as np
import pytest

import pcg_statement as ps
import problems as pb
import semidefinite_cases as sc
import semidefinite_statement as sd

EPS = np.finfo(np.float64).eps

MEASURED = {
    "perpoisson5_64x48_v21": (7, 8),
    "perpoisson5_64x48_v11": (9, 11),
    "perpoisson5_64x48_linex": (7, 9),
    "perpoisson5_64x48_linexy": (5, 6),
    "perpoisson5_64x48_f21": (6, 8),
    "perpoisson5_32_v21": (6, 7),
    "perregime9_xy_48x32_v21": (14, 29),
    "perregime9_xy_48x32_linexy": (10, 19),
    "perregime9_x_48x33_v21": (15, 33),
    "neumann9_33x29_v21": (14, 29),
    "neumann5_40x36_linexy": (15, 38),
    "neumann9_40x36_f21": (12, 23),
    "perpoisson7_xyz_32x16x24_v21": (12, 21),
    "perpoisson7_xyz_16_v21": (8, 9),
    "perregime27_xyz_16x24x16_v21": (7, 9),
    "perregime27_z_16x13x16_v21": (8, 10),
    "neumann27_17x13x11_v21": (8, 10),
    "neumann27_17x13x11_v11": (9, 12),
    "neumann7_17x13x11_v21": (23, None),
}


def test_the_table_lists_every_case():
    assert sorted(MEASURED) == sorted(sc.CASES) and len(sc.CASES) == 19


@pytest.mark.parametrize("name", list(sc.CASES))
def test_flexible_cg_on_the_semidefinite_cycle(oracle, name):
    mk, ibc, st = sc.CASES[name]
    so = mk()
    g = so.shape[1:]
    ml, Ac = sd.ml_create(oracle, so, ibc, **st)
    try:
        # the Galerkin coarsest operator keeps the null space
        assert np.max(np.abs(Ac.sum(axis=1))) <= 1e-12 * np.max(np.abs(Ac))
        assert np.max(np.abs(Ac - Ac.T)) <= 1e-12 * np.max(np.abs(Ac))
        # the coarse solve with the replaced factor is exact on zero-sum data
        last = ml.nlevels() - 1
        nx, ny, nz = ml.dims(last)
        gc = (ny + 2, nx + 2) if so.ndim == 3 else (nz + 2, ny + 2, nx + 2)
        f = ps.random_field(gc, 41)
        sd.project(f)
        n, kappa = Ac.shape[0], sd.kappa_plus(Ac)
        y = np.zeros(gc)
        abd = ml.array(last, "ABD").reshape(n, -1)
        (oracle.solve_cg2 if so.ndim == 3 else oracle.solve_cg3)(y, f, abd, ibc)
        yi = np.array(ps.inner(y)).reshape(-1)
        yi -= yi.mean()
        ref = np.linalg.lstsq(Ac, np.array(ps.inner(f)).reshape(-1), rcond=None)[0]
        ref -= ref.mean()
        err = np.linalg.norm(yi - ref) / np.linalg.norm(ref)
        print(f"\n{name}: coarsest n={n} kappa={kappa:.3g} coarse-solve error={err:.2e} bound={64 * n * EPS * kappa:.2e}")
        assert err <= 64 * n * EPS * kappa

        b, x = ps.random_field(g, 17), ps.random_field(g, 23)
        sd.project(b)
        sd.project(x)
        it, hist = sd.fcg_semidefinite(oracle, so, b, x, ml, ibc, max_iter=sc.MAX_ITER, tol=sc.TOL)
        true = sd.true_residual(oracle, so, b, x, ibc) / hist[0]
        xs = np.array(ps.random_field(g, 23))
        sd.project(xs)
        its, hs = sd.stationary(oracle, so, b, xs, ml, ibc, max_iter=sc.MAX_ITER, tol=sc.TOL)
        conv = bool(np.isfinite(hs[-1]) and hs[-1] < sc.TOL)
        print(f"{name}: fcg {it} (hist[-1]={hist[-1]:.2e}, true={true:.2e}), stationary {its if conv else None} "
              f"(hist[-1]={hs[-1]:.2e}), mean(x)={np.mean(ps.inner(x)):.1e}")
        assert it <= sc.MAX_ITER and hist[-1] < sc.TOL
        assert true <= 1.01 * sc.TOL
        assert abs(np.mean(ps.inner(x))) <= 2 * EPS * np.mean(np.abs(ps.inner(x))) * x.size
        if conv:
            assert it <= its
    finally:
        ml.close()


@pytest.mark.parametrize("name", list(sc.CASES))
def test_the_plain_recurrence_takes_the_same_iterations(oracle, name):
    """r0 and the final x alone projected, the cycle as it is: the same in exact arithmetic as the P M P form the library
    runs, so it converges in the same number of iterations, to the same true residual bound, with histories that agree
    to 1e-5 of an entry above 1e-10: an entry near 1e-10 is fixed to eps / 1e-10 = 2e-6 of its value at best, and the plain
    form was measured to move by up to 4e-6 under rounding-level changes (ProjectedCycle)"""
    mk, ibc, st = sc.CASES[name]
    so = mk()
    g = so.shape[1:]
    mask = pb.interior_mask(g)
    b = ps.random_field(g, 17) + 3.0 * mask
    ml, _ = sd.ml_create(oracle, so, ibc, **st)
    try:
        out = []
        for projected in (False, True):
            x = ps.random_field(g, 23) - 2.0 * mask
            it, hist = sd.fcg_semidefinite(oracle, so, b, x, ml, ibc, projected=projected, max_iter=sc.MAX_ITER, tol=sc.TOL)
            assert hist[-1] < sc.TOL and sd.true_residual(oracle, so, b, x, ibc) / hist[0] <= 1.01 * sc.TOL
            out.append((it, hist))
    finally:
        ml.close()
    (itp, hp), (it, h) = out
    keep = h >= 1e-10
    print(f"\n{name}: plain {itp}, P M P {it}, largest relative difference above 1e-10 {np.max(np.abs(hp[:len(h)][keep] / h[keep] - 1)):.1e}")
    assert itp == it == MEASURED[name][0]
    np.testing.assert_allclose(hp[:len(h)][keep], h[keep], rtol=1e-5)


def test_the_dense_reference_solves_the_projected_system(oracle):
    so = sc.wrapped_poisson2(16, 12)
    b = ps.random_field(so.shape[1:], 17) + 3.0 * pb.interior_mask(so.shape[1:])
    x, kappa = sd.solve_reference(so, b, 3)
    assert abs(np.mean(ps.inner(x))) <= 1e-14 * np.max(np.abs(x))
    assert sd.true_residual(oracle, so, b, x, 3) <= 64 * x.size * EPS * kappa * np.linalg.norm(ps.inner(b))
