"""The numpy statement of flexible CG on periodic handles (tests/fcg_periodic_statement.py) on the oracle, without a GPU.

Every periodic solve case of tests/cases.py (SOLVES_PER, SOLVES_PER3: 2D point and line relaxation, 3D point relaxation,
V(1,1), V(2,1), F(2,1), every boundary code the cases cover) with b = random_field(g, 17), x0 = random_field(g, 23),
relative tolerance 1e-10, at most 40 iterations.  Asserted: convergence, the true residual, an iteration count no
larger than the stationary defect-correction iteration's, and strictly fewer iterations on the Poisson cases.  These
are the numbers tests/test_gpu_fcg_periodic.py leans on.

MEASURED: (flexible CG, standard beta, stationary iteration, symmetry defect of M) as this test prints them (-s); the
standard beta and the defect (fields random_field(g, 31), random_field(g, 37)) are printed for DESIGN.md section 19.  The
table is a record; the assertions below are on what a run computes.
"""
import numpy as np
import pytest

import cases
import fcg_periodic_statement as fps
import pcg_statement as ps

ALL = [("2d", k) for k in cases.SOLVES_PER] + [("3d", k) for k in cases.SOLVES_PER3]

MEASURED = {
    "perpoisson5_x_300_v11": (11, 11, 17, 1.3e-03),
    "perpoisson5_y_128x96_v21": (9, 10, 23, 6.2e-03),
    "perrand9_xy_96x80_v21": (3, 3, 4, 3.7e-05),
    "perrand9_x_100x75_v21": (3, 3, 4, 4.8e-05),
    "perrand5_xy_64_v21": (3, 3, 3, 2.8e-05),
    "perpoisson5_x_200x60_linex": (9, 10, 26, 5.5e-02),
    "perpoisson5_y_60x200_liney": (11, 15, 26, 1.8e-01),
    "perrand9_xy_96x80_linexy": (2, 2, 2, 1.2e-07),
    "perrand9_x_100x75_linexy": (2, 2, 2, 2.9e-07),
    "perrand9_xy_96x80_f21": (3, 3, 4, 1.6e-04),
    "perpoisson5_x_200x60_linex_f21": (5, 5, 7, 6.6e-05),
    "perpoisson7_z_32_v21": (9, 10, 17, 1.0e-02),
    "perpoisson7_z_24x20x32_v11": (13, 13, 20, 1.5e-02),
    "perrand27_z_20x24x32_v21": (3, 3, 3, 1.6e-04),
    "perpoisson7_x_32_v21": (10, 10, 16, 1.2e-03),
    "perpoisson7_xy_32x32x24_v21": (11, 12, 27, 2.0e-02),
    "perrand27_y_24x32x20_v21": (3, 3, 3, 8.6e-06),
    "perrand27_xz_32x20x24_v21": (3, 3, 3, 1.3e-05),
    "perrand27_yz_20x32x32_v11": (4, 4, 4, 2.8e-16),
    "perrand27_xyz_32_v21": (3, 3, 3, 9.8e-05),
    "perrand27_z_20x24x32_f21": (3, 3, 3, 1.5e-04),
    "perpoisson7_xy_32x32x24_f21": (8, 8, 12, 2.4e-02),
}


def setup(oracle, dim, name):
    mk_op, _, st = (cases.SOLVES_PER if dim == "2d" else cases.SOLVES_PER3)[name]
    so = mk_op()
    g = so.shape[1:]
    return so, st, ps.random_field(g, 17), ps.random_field(g, 23)


def test_the_case_lists_are_the_22_the_gpu_test_runs():
    assert len(ALL) == 22 and len([n for _, n in ALL if n.startswith("perpoisson")]) == 10


@pytest.mark.parametrize("dim,name", ALL, ids=[n for _, n in ALL])
def test_flexible_cg_on_the_periodic_cycle(oracle, dim, name):
    so, st, b, x0 = setup(oracle, dim, name)
    ibc = st["ibc"]
    ml = oracle.ml_create(so, **st)
    try:
        x = x0.copy()
        n, h = fps.fcg_periodic(oracle, so, b, x, ml, ibc, tol=1e-10, max_iter=40)
        xs = x0.copy()
        ns, hs = fps.fcg_periodic(oracle, so, b, xs, ml, ibc, standard=True, tol=1e-10, max_iter=40)
        xd = x0.copy()
        nd_, hd = fps.stationary(oracle, so, b, xd, ml, ibc, tol=1e-10, max_iter=40)
        defect = fps.symmetry_defect(oracle, ml, so.shape[1:], ibc, so.ndim - 1)
    finally:
        ml.close()
    true = fps.true_residual(oracle, so, b, x, ibc) / h[0]
    print("%-34s fcg %2d  standard %2d  stationary %2d  defect %.1e  true %.2e" % (name, n, ns, nd_, defect, true))
    assert n <= 40 and h[-1] < 1e-10, (n, h)
    assert true < 1e-10, true
    assert hd[-1] < 1e-10, (nd_, hd)  # the stationary count is a count to convergence
    assert n <= nd_, (n, nd_)
    if name.startswith("perpoisson"):
        assert n < nd_, (n, nd_)

