"""Singular problems on the device: cedar_amd_solver_create_semidefinite, cedar_amd_solver_fcg_semidefinite / _many and the
projection kernel cedar_amd_project_mean, against numpy and the statement of tests/semidefinite_statement.py on the oracle.

Tolerances.  The projection's mean: any summation order of n terms is within n eps mean|v| of the exact mean.  The
coarsest factor and solve: 64 n eps times the norm / the condition number on the range (Cholesky and two triangular
solves of n unknowns are backward stable with a constant of order n; 64 covers the band or dense kernels' constant).
Histories: test_gpu_pcg.compare_hist, the project's rule.  The mean of a returned x: the projection subtracts a mean
that is within n eps mean|x| of the exact one and the subtraction rounds once more, so 2 n eps mean|x|.
"""
import numpy as np
import pytest

import fcg_periodic_statement as fps
import pcg_statement as ps
import problems as pb
import semidefinite_cases as sc
import semidefinite_statement as sd
from test_gpu_pcg import compare_hist

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def capi():
    from cedar_amd import capi
    assert capi.device_count() >= 1, "no GPU visible"
    return capi


@pytest.fixture(scope="module")
def K(capi):
    return capi.Kernels()


def interior(a):
    return a[tuple(slice(1, -1) for _ in a.shape)]


def level_shape(ext):
    """interior (nx, ny[, nz]) -> array shape with ghosts, slowest first"""
    return tuple(n + 2 for n in ext[::-1])


# ------------------------------------------------------------------ 1. the projection kernel
# row lengths either side of the 64 / 128 / 256 lane steps and rows walked in several trips; one and several row groups
PM_SHAPES = [(3, 3), (66, 5), (130, 4), (258, 3), (1030, 3), (9, 8, 7), (130, 6, 5), (514, 3, 4)]


@pytest.mark.parametrize("ext", [(64, 32), (128, 4, 4)], ids=str)
def test_project_mean_is_exact_on_integer_data(K, ext):
    g = level_shape(ext)
    v = np.floor(pb.uniform(g, 5, -50.0, 51.0))
    v0 = v.copy()
    mean = K.project_mean(v)
    want = v0.copy()
    m = np.mean(interior(v0))
    interior(want)[...] -= m
    assert np.array_equal(mean, [m]) and m != 0.0
    assert np.array_equal(v, want)


@pytest.mark.parametrize("ext", PM_SHAPES, ids=str)
def test_project_mean_against_numpy_single_and_batched(K, ext):
    g = level_shape(ext)
    n = int(np.prod(ext))
    items = [pb.uniform(g, 11 + m, -1.0, 3.0) for m in range(3)]  # ghosts filled too: they must come back bit for bit
    single = []
    for v0 in items:
        v = v0.copy()
        mean = K.project_mean(v)
        exact = np.mean(interior(v0).astype(np.longdouble))
        assert abs(np.longdouble(mean[0]) - exact) <= n * EPS * np.mean(np.abs(interior(v0)))
        assert mean[0] == sd.mean_interior(v0)  # the sum is carried in two doubles: the correctly rounded mean
        want = v0.copy()
        interior(want)[...] -= mean[0]  # one rounding per point, as the kernel's subtraction
        assert np.array_equal(v, want)
        single.append((v, mean[0]))
    batch = np.stack(items)
    means = K.project_mean(batch, nrhs=3, active=0b101)
    assert np.array_equal(batch[1], items[1]) and means[1] == 0.0
    for m in (0, 2):
        assert np.array_equal(batch[m], single[m][0]) and means[m] == single[m][1], m
    batch = np.stack(items)
    means = K.project_mean(batch, nrhs=3)
    for m in range(3):
        assert np.array_equal(batch[m], single[m][0]) and means[m] == single[m][1], m


def test_project_mean_refusals(capi, capfd):
    v = np.ones((5, 5))
    for nrhs, a in ((0, v), (33, v), (1, np.ones((5, 2)))):
        assert capi.lib.cedar_amd_project_mean(nrhs, 1, a.ctypes.data, a.shape[-1], a.shape[-2], 1, None) == -1
        assert "cedar_amd_project_mean" in capfd.readouterr().err
    assert np.array_equal(v, np.ones((5, 5)))


# ------------------------------------------------------------------ 2. the coarsest solve on one-level handles
def one_level_op(ext, ibc):
    nd = len(ext)
    per = sd.per_of(nd, ibc)[:nd]
    return pb.regime_op(level_shape(ext), 5 if nd == 2 else 14, 7, p_zero=1, per=per)


def factor_of(abd, n, ibc, ext):
    """U from the handle's ABD: dense column-major (ibc != 0) or LAPACK upper band storage (ibc == 0)"""
    if ibc != 0:
        return np.triu(abd.reshape(n, n).T)
    kd = ext[0] + 1 if len(ext) == 2 else ext[0] * (ext[1] + 1) + 1
    ab = abd.reshape(n, kd + 1)
    U = np.zeros((n, n))
    for j in range(n):
        lo = max(0, j - kd)
        U[lo: j + 1, j] = ab[j, kd + lo - j: kd + 1]
    return U


ONE_LEVEL = [((5, 4), 0), ((5, 4), 3), ((4, 3), 0), ((4, 3), 3)] + [(e, c) for e in ((4, 3, 3), (3, 4, 4)) for c in (0, 5, 8)]


@pytest.mark.parametrize("ext,ibc", ONE_LEVEL, ids=str)
def test_coarsest_factor_and_solve_on_a_one_level_handle(capi, ext, ibc):
    so = one_level_op(ext, ibc)
    g = so.shape[1:]
    n = int(np.prod(ext))
    Ac = sd.assemble(so, ibc)
    assert np.max(np.abs(Ac.sum(axis=1))) <= 64 * EPS * np.max(np.abs(Ac))
    s = capi.Solver(so, ibc=ibc, num_levels=1, semidefinite=True)
    sm = capi.Solver(so, ibc=ibc, num_levels=1, semidefinite=True, max_rhs=3)
    try:
        assert s.nlevels() == 1 and sm.max_rhs() == 3
        U = factor_of(s.array(0, "ABD"), n, ibc, ext)
        B = Ac.copy()
        B[-1, -1] += B[-1, -1]
        assert np.max(np.abs(U.T @ U - B)) <= 64 * n * EPS * np.linalg.norm(Ac, 2)
        kd = None if ibc != 0 else ext[0] + 1 if len(ext) == 2 else ext[0] * (ext[1] + 1) + 1
        assert np.array_equal(U, sd.bumped_factor(Ac, kd))  # the statement restates the routine's operation order
        kappa = sd.kappa_plus(Ac)
        fs_, ys = [], []
        for m in range(3):
            f = ps.random_field(g, 41 + m)
            sd.project(f)
            y = np.zeros(g)
            s.vcycle(y, f)
            yi = interior(y).reshape(-1)
            assert abs(yi.mean()) <= 2 * n * EPS * np.mean(np.abs(yi))
            ref = np.linalg.lstsq(Ac, interior(f).reshape(-1), rcond=None)[0]
            ref -= ref.mean()
            assert np.linalg.norm(yi - ref) <= 64 * n * EPS * kappa * np.linalg.norm(ref)
            fs_.append(f)
            ys.append(y)
        Y = np.zeros((3,) + g)
        sm.vcycle_many(Y, np.stack(fs_))
        for m in range(3):
            assert np.array_equal(Y[m], ys[m]), m
    finally:
        s.close()
        sm.close()


# ------------------------------------------------------------------ 3. parity with the statement
_STATEMENT = {}


def statement(oracle, name):
    """(so, ibc, settings, b, x0, iterations, hist, x) of the statement on a case, computed once.  b and x0 are NOT
    compatible / zero-mean: both projections are exercised"""
    if name not in _STATEMENT:
        mk, ibc, st = sc.CASES[name]
        so = mk()
        g = so.shape[1:]
        mask = pb.interior_mask(g)
        b = ps.random_field(g, 17) + 3.0 * mask
        x0 = ps.random_field(g, 23) - 2.0 * mask
        ml, _ = sd.ml_create(oracle, so, ibc, **st)
        x = x0.copy()
        it, hist = sd.fcg_semidefinite(oracle, so, b, x, ml, ibc, max_iter=sc.MAX_ITER, tol=sc.TOL)
        ml.close()
        for a in (so, b, x0, hist, x):
            a.setflags(write=False)
        _STATEMENT[name] = (so, ibc, st, b, x0, it, hist, x)
    return _STATEMENT[name]


_DEVICE = {}


def device(capi, oracle, name):
    """(x, hist) of cedar_amd_solver_fcg_semidefinite on the case, computed once; b must come back unwritten"""
    if name not in _DEVICE:
        so, ibc, st, b, x0, its, hs, xs = statement(oracle, name)
        s = capi.Solver(so, ibc=ibc, semidefinite=True, **st)
        try:
            x = x0.copy()
            b0 = b.copy()
            h = s.fcg_semidefinite(b0, x, max_iter=sc.MAX_ITER, tol=sc.TOL)
        finally:
            s.close()
        assert np.array_equal(b0, b)
        _DEVICE[name] = (x, h)
    return _DEVICE[name]


@pytest.mark.parametrize("name", list(sc.CASES))
def test_fcg_semidefinite_against_the_statement(capi, oracle, name):
    """counts within one, histories to rtol 1e-8 above 1e-10 (test_gpu_pcg.compare_hist, the project's rule).

    The rule holds because the cycle is applied as P M P (solver.cpp pcg_run, semidefinite_statement.ProjectedCycle).  With
    r0 and the final x alone projected 12 of these 19 cases missed it in their last entries above 1e-10, by 2e-8 to
    1.2e-6, although the mean removed from r0 and the coarsest factor had the statement's bits: the history then depends
    on rounding through the constants.  With the two projections around every cycle the largest relative difference
    above 1e-10 is 1.4e-14 to 1.6e-12 over the 19 cases on the MI355X (printed with -s)."""
    so, ibc, st, b, x0, its, hs, xs = statement(oracle, name)
    x, h = device(capi, oracle, name)
    n = len(h) - 1
    m = min(len(h), len(hs))
    keep = hs[1:m] >= 1e-10
    worst = np.max(np.abs(h[1:m][keep] / hs[1:m][keep] - 1.0)) if keep.any() else 0.0
    print(f"\n{name}: device {n} iterations (hist[-1]={h[-1]:.2e}), statement {its} (hist[-1]={hs[-1]:.2e}), "
          f"|h0/hs0 - 1|={abs(h[0] / hs[0] - 1):.1e}, largest relative difference above 1e-10: {worst:.1e}, "
          f"|x - xs|/|xs|={np.linalg.norm(interior(x - xs)) / np.linalg.norm(interior(xs)):.1e}")
    compare_hist(h, hs, n, its)


@pytest.mark.parametrize("name", list(sc.CASES))
def test_fcg_semidefinite_converges_to_the_zero_mean_solution(capi, oracle, name):
    so, ibc, st, b, x0, its, hs, xs = statement(oracle, name)
    x, h = device(capi, oracle, name)
    assert abs(len(h) - 1 - its) <= 1
    assert h[-1] < sc.TOL
    np.testing.assert_allclose(h[0], hs[0], rtol=1e-10)
    assert sd.true_residual(oracle, so, b, x, ibc) / h[0] <= 1.01 * sc.TOL
    xi = interior(x)
    assert abs(xi.mean()) <= 2 * xi.size * EPS * np.mean(np.abs(xi))
    if ibc != 0:
        assert np.array_equal(x, fps.wrap(x.copy(), sd.per_of(so.ndim - 1, ibc)))
    else:
        ghosts = 1 - pb.interior_mask(x.shape)
        assert np.array_equal(x * ghosts, x0 * ghosts)


# ------------------------------------------------------------------ 4. the dense solution
DENSE = {
    "perpoisson5_16x12": (lambda: sc.wrapped_poisson2(16, 12), 3),
    "neumann9_13x11": (lambda: pb.regime_op((13, 15), 5, 9, p_zero=1), 0),
    "perpoisson7_8x6x8": (lambda: pb.periodic_poisson3(8, 6, 8, (1, 1, 1)), 8),
}


@pytest.mark.parametrize("name", list(DENSE))
def test_fcg_semidefinite_against_the_dense_solution(capi, oracle, name):
    mk, ibc = DENSE[name]
    so = mk()
    g = so.shape[1:]
    b = ps.random_field(g, 17) + 3.0 * pb.interior_mask(g)
    xref, kappa = sd.solve_reference(so, b, ibc)
    s = capi.Solver(so, ibc=ibc, semidefinite=True)
    try:
        x = ps.random_field(g, 23) - 2.0 * pb.interior_mask(g)
        h = s.fcg_semidefinite(b, x, max_iter=sc.MAX_ITER, tol=sc.TOL)
    finally:
        s.close()
    assert h[-1] < sc.TOL
    pb_ = b * pb.interior_mask(g)
    sd.project(pb_)
    rel_res = sd.true_residual(oracle, so, b, x, ibc) / np.linalg.norm(interior(pb_))
    err = np.linalg.norm(interior(x - xref)) / np.linalg.norm(interior(xref))
    print(f"\n{name}: kappa={kappa:.3g} relative residual={rel_res:.2e} error={err:.2e}")
    assert err <= kappa * rel_res


# ------------------------------------------------------------------ 5. batches
BATCH = ["perpoisson5_32_v21", "neumann5_40x36_linexy", "perregime27_xyz_16x24x16_v21"]


@pytest.mark.parametrize("name", BATCH)
def test_fcg_semidefinite_many_equals_the_single_call_per_item(capi, name):
    mk, ibc, st = sc.CASES[name]
    so = mk()
    g = so.shape[1:]
    mask = pb.interior_mask(g)
    B = np.stack([ps.random_field(g, 17 + m) + 3.0 * mask for m in range(4)])
    X0 = np.stack([ps.random_field(g, 23 + m) - 2.0 * mask for m in range(4)])
    B[2] = 0.0  # nothing to do for this item: it freezes at once
    X0[2] = 0.0
    sm = capi.Solver(so, ibc=ibc, semidefinite=True, max_rhs=4, **st)
    s1 = capi.Solver(so, ibc=ibc, semidefinite=True, **st)
    try:
        assert sm.max_rhs() == 4
        single = []
        for m in range(4):
            x = X0[m].copy()
            h = s1.fcg_semidefinite(B[m], x, max_iter=sc.MAX_ITER, tol=sc.TOL)
            single.append((x, h))
        assert len(single[2][1]) == 1 and single[2][1][0] == 0.0 and not single[2][0].any()
        assert min(len(single[m][1]) for m in (0, 1, 3)) > 3
        for nrhs in (4, 1, 3):
            X = X0[:nrhs].copy()
            hist, iters = sm.fcg_semidefinite_many(B[:nrhs].copy(), X, max_iter=sc.MAX_ITER, tol=sc.TOL)
            for m in range(nrhs):
                x, h = single[m]
                assert iters[m] == len(h) - 1 and np.array_equal(hist[m], h), (nrhs, m, hist[m], h)
                assert np.array_equal(X[m], x), (nrhs, m, np.max(np.abs(X[m] - x)))
    finally:
        sm.close()
        s1.close()


# ------------------------------------------------------------------ 6. solve and vcycle on a semidefinite handle
def test_solve_and_vcycle_run_the_semidefinite_cycle(capi, oracle):
    name = "perpoisson5_64x48_v21"
    mk, ibc, st = sc.CASES[name]
    so = mk()
    g = so.shape[1:]
    b = ps.random_field(g, 17)
    sd.project(b)  # solve does not project: a compatible right-hand side
    ml, _ = sd.ml_create(oracle, so, ibc, **st)
    its, hs = sd.stationary(oracle, so, b, np.zeros(g), ml, ibc, max_iter=20, tol=1e-8)
    z = np.zeros(g)
    fps.WrappedCycle(ml, sd.per_of(2, ibc)).vcycle(z, b)
    ml.close()
    assert hs[-1] < 1e-8
    s = capi.Solver(so, ibc=ibc, semidefinite=True, max_iter=20, tol=1e-8, **st)
    try:
        x = np.zeros(g)
        h = s.solve(b, x)
        y = np.zeros(g)
        s.vcycle(y, b)
    finally:
        s.close()
    print(f"\nsolve: device {len(h) - 1} cycles (rel={h[-1]:.2e}), statement {its} (rel={hs[-1]:.2e})")
    assert h[-1] < 1e-8 and len(h) - 1 <= its + 1
    assert np.max(np.abs(interior(y) - interior(z))) <= 1e-11 * np.max(np.abs(interior(z)))


# ------------------------------------------------------------------ 7. refusals
def test_creation_refusals(capi, capfd):
    who = "cedar_amd_solver_create_semidefinite"
    neumann3 = pb.regime_op((13, 15, 19), 14, 5, p_zero=1)
    for so, kw, text in [
        (pb.poisson2(15, 15), dict(), "null space is not the constants"),
        (neumann3, dict(relax="plane-xy"), "plane relaxation is not served"),
        (neumann3, dict(relax="plane-xyz"), "plane relaxation is not served"),
        (sc.wrapped_poisson2(32, 32), dict(ibc=-3), "boundary codes below zero"),
        # nx 10 -> 5 -> 3: the level with 5 is coarsened
        (pb.regime_op((18, 18, 12), 14, 5, p_zero=1, per=(1, 0, 0)), dict(ibc=2), "even extent"),
        (sc.wrapped_poisson2(32, 32), dict(ibc=3, max_rhs=2, cycle="f"), "only the V-cycle is supported"),
        (pb.regime_op((31, 35), 5, 9, p_zero=1), dict(max_rhs=2, cycle="f"), "only the V-cycle is supported"),
    ]:
        with pytest.raises(RuntimeError):
            capi.Solver(so, semidefinite=True, **kw)
        err = capfd.readouterr().err
        assert who in err and text in err, (text, err)
    with pytest.raises(RuntimeError):  # as before the new call existed
        capi.Solver(pb.periodic_random_op3(8, 8, 8, 14, (1, 0, 0), 1), ibc=-2)
    err = capfd.readouterr().err
    assert "periodic" in err and who not in err


@pytest.mark.parametrize("name", ["perpoisson5_32_v21", "neumann9_33x29_v21", "neumann27_17x13x11_v21"])
def test_the_other_calls_refuse_a_semidefinite_handle(capi, capfd, name):
    mk, ibc, st = sc.CASES[name]
    so = mk()
    g = so.shape[1:]
    b = ps.random_field(g, 17)
    x0 = ps.random_field(g, 23)
    s = capi.Solver(so, ibc=ibc, semidefinite=True, **st)
    sm = capi.Solver(so, ibc=ibc, semidefinite=True, max_rhs=2, **st)
    try:
        for call in (s.pcg, s.fcg, s.fcg_periodic):
            x = x0.copy()
            with pytest.raises(RuntimeError):
                call(b, x)
            assert "cedar_amd_solver_fcg_semidefinite" in capfd.readouterr().err and np.array_equal(x, x0)
        for call in (sm.pcg_many, sm.fcg_many, sm.fcg_periodic_many):
            X = np.stack([x0, x0])
            with pytest.raises(RuntimeError):
                call(np.stack([b, b]), X)
            assert "cedar_amd_solver_fcg_semidefinite" in capfd.readouterr().err and np.array_equal(X[1], x0)
        z = x0.copy()
        s.precondition(z, b)
        assert "cedar_amd_solver_fcg_semidefinite" in capfd.readouterr().err and np.array_equal(z, x0)
        for switch in (s.use_fp32_operator, s.use_fp32_operator_all, s.use_fp32_operator_2d, s.use_fp32_operator_lines,
                       s.use_fp32_interpolation, sm.use_fp32_operator_many):
            assert switch(1) == -1
            assert "cedar_amd_solver_fcg_semidefinite" in capfd.readouterr().err
        assert s.fp32_levels() == 0
        # the handle still serves its own call afterwards
        x = x0.copy()
        assert s.fcg_semidefinite(b, x, max_iter=sc.MAX_ITER, tol=sc.TOL)[-1] < sc.TOL
    finally:
        s.close()
        sm.close()


def test_fcg_semidefinite_refuses_other_handles_and_null_vectors(capi, capfd):
    so = pb.poisson2(15, 15)
    b = pb.rhs2(15, 15)
    s = capi.Solver(so)
    sm = capi.Solver(so, max_rhs=2)
    sd_ = capi.Solver(pb.regime_op((31, 35), 5, 9, p_zero=1), semidefinite=True)
    try:
        x = np.zeros_like(b)
        with pytest.raises(RuntimeError):
            s.fcg_semidefinite(b, x)
        assert "not made by cedar_amd_solver_create_semidefinite" in capfd.readouterr().err and not x.any()
        X = np.zeros((2,) + b.shape)
        with pytest.raises(RuntimeError):
            sm.fcg_semidefinite_many(np.stack([b, b]), X)
        assert "not made by cedar_amd_solver_create_semidefinite" in capfd.readouterr().err and not X.any()
        assert capi.lib.cedar_amd_solver_fcg_semidefinite(sd_.h, None, None, None, None) == -1
        assert "b and x must not be NULL" in capfd.readouterr().err
        g = (31, 35)
        bb, xx = ps.random_field(g, 17), np.zeros(g)
        with pytest.raises(RuntimeError):
            sd_.fcg_semidefinite(bb, xx, max_iter=-1)
        assert "max_iter must not be negative" in capfd.readouterr().err and not xx.any()
        with pytest.raises(RuntimeError):  # a handle of one right-hand side
            sd_.fcg_semidefinite_many(np.stack([bb, bb]), np.zeros((2,) + g))
        assert "nrhs exceeds" in capfd.readouterr().err
    finally:
        s.close()
        sm.close()
        sd_.close()
