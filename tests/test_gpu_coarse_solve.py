"""The coarsest-grid direct solves past every lane and LDS step, entry by entry against the oracle, and against the
operator itself.

cgsolve.hip factors the band on one workgroup of 256 threads (dpbtf2_upper_wg strides its scaling loop and its rank-one
update over the band width kd: steps at kd 256|257, a third trip from 513) and solves on one wavefront
(dpbtrs_upper_wave strides over kd: steps at 64|65, a third trip from 129); solve_cg2/3 stage the factor in LDS when
(nabd1 * nabd2 + nabd2 + 2) doubles fit into 60 KiB.  periodic3d.hip factors and solves the dense periodic operator with
1024 threads striding over N = nx ny nz (step at 1024|1025, N <= 2048 admitted); periodic2d.hip does the same on one lane.
The shapes below sit on both sides of every one of these steps; _band_coverage() asserts it at import time.

Two comparisons per case:
* bit for bit with the oracle, whose orc_dpbtrf_upper / orc_dpbtrs_upper / orc_dpotrf_upper / orc_dpotrs_upper restate
  the unblocked LAPACK loops whose order the kernels claim (-ffp-contract=off on both sides);
* r = b - A x in np.longdouble with a matvec written here from the stencil arrays alone (no oracle, no library): the
  answer solves the system the operator defines, whatever the oracle and the kernel agree on.
"""
import numpy as np
import pytest

import cases
import problems as pb

pytestmark = pytest.mark.gpu

LDS_DOUBLES = 60 * 1024 // 8  # solve_cg2/3: the factor and the right-hand side are staged in LDS up to this size


@pytest.fixture(scope="module")
def capi():
    from cedar_amd import capi
    assert capi.device_count() >= 1, "no GPU visible"
    return capi


@pytest.fixture(scope="module")
def K(capi):
    return capi.Kernels()


# ------------------------------------------------------------------ the operator, applied in extended precision
# slot s stored at point P couples the points P + EA[s] and P + EB[s] (offsets (di, dj[, dk]); BoxMG's symmetric storage:
# W, S, SW, NW in 2D; the same in the plane and the nine couplings to the plane below in 3D).  Off-diagonals are stored
# with the opposite sign.
E2 = {pb.KW: ((0, 0), (-1, 0)), pb.KS: ((0, 0), (0, -1)), pb.KSW: ((0, 0), (-1, -1)), pb.KNW: ((0, -1), (-1, 0))}
E3 = {pb.KPW: ((0, 0, 0), (-1, 0, 0)), pb.KPS: ((0, 0, 0), (0, -1, 0)), pb.KB: ((0, 0, 0), (0, 0, -1)),
      pb.KPSW: ((0, 0, 0), (-1, -1, 0)), pb.KPNW: ((0, -1, 0), (-1, 0, 0)), pb.KBW: ((0, 0, 0), (-1, 0, -1)),
      pb.KBNW: ((0, -1, 0), (-1, 0, -1)), pb.KBN: ((0, -1, 0), (0, 0, -1)), pb.KBNE: ((-1, -1, 0), (0, 0, -1)),
      pb.KBE: ((-1, 0, 0), (0, 0, -1)), pb.KBSE: ((-1, 0, 0), (0, -1, -1)), pb.KBS: ((0, 0, 0), (0, -1, -1)),
      pb.KBSW: ((0, 0, 0), (-1, -1, -1))}


def _shifted(a, off):
    """a at the interior points displaced by off = (di, dj[, dk]) (numpy axes are reversed: last axis = i)"""
    return a[tuple(slice(1 + d, a.shape[ax] - 1 + d) for ax, d in enumerate(reversed(off)))]


def matvec_ld(so, x):
    """(A x) at the interior points, np.longdouble.  x carries whatever the caller put into its ghost layer (zeros for a
    Dirichlet problem, the periodic image for a periodic one); so carries the matching coefficients there."""
    so, x = so.astype(np.longdouble), x.astype(np.longdouble)
    nd = x.ndim
    table = E2 if nd == 2 else E3
    zero = (0,) * nd
    y = _shifted(so[0], zero) * _shifted(x, zero)
    for s, (ea, eb) in table.items():
        if s >= so.shape[0]:
            continue
        for a, b in ((ea, eb), (eb, ea)):
            # the coefficient stored at P = n - a couples n with n - a + b
            na = tuple(-v for v in a)
            y = y - _shifted(so[s], na) * _shifted(x, tuple(q - p for p, q in zip(a, b)))
    return y


def trimmed(so):
    """so without the couplings that reach outside the interior.  BoxMG's Dirichlet operators carry none (the galleries
    drop them), and the band assembly relies on it: it files the W coefficient of the first point of a row under the pair
    (that point, last point of the row before).  Still strictly diagonally dominant."""
    so = so.copy()
    m = pb.interior_mask(so.shape[1:])
    for s, (ea, eb) in (E2 if so.ndim == 3 else E3).items():
        if s < so.shape[0]:
            for e in (ea, eb):  # keep the coefficient at P when P + e is an interior point
                so[s] *= np.roll(m, tuple(-d for d in reversed(e)), axis=tuple(range(m.ndim)))
    return so


def wrap_ld(x, per):
    """copy of x with the periodic image in its ghost layers, corners included (per = (px, py[, pz]))"""
    x = x.copy()
    for ax, p in zip(range(x.ndim - 1, -1, -1), per):
        if p:
            lo = [slice(None)] * x.ndim
            lo[ax] = 0
            src = list(lo)
            src[ax] = -2
            x[tuple(lo)] = x[tuple(src)]
            lo[ax], src[ax] = -1, 1
            x[tuple(lo)] = x[tuple(src)]
    return x


def inner(a):
    return a[tuple(slice(1, -1) for _ in a.shape)]


# The oracle's own x, measured on the CPU over every case below with matvec_ld: the worst max|b - A x| / max|b| is
# 3.2e-15 over the band solves (26x19x3, 27-point), 3.8e-15 over the dense periodic ones in 3D (8x16x16, per_yz) and
# 8.6e-16 in 2D.  The bound is ten times the worst of them: 10 * 3.8e-15.
RESIDUAL_TOL = 3.8e-14


def check_residual(so, b, x, per=None):
    """max|b - A x| <= RESIDUAL_TOL max|b| at the interior points.  Periodic solves return x minus its mean (SOLVE_cg
    removes it whenever the boundary code is periodic), so b - A x = t A 1 with t = mean of the solution of A y = b: the
    multiple t of A 1 is taken out first (least squares), and the mean of x must vanish to the rounding of that
    subtraction -- N terms summed in order, one division, one addition each: |sum x| <= (N + 2) eps N (max|x| + |t|)."""
    if per is None:
        r = inner(b).astype(np.longdouble) - matvec_ld(so, x)
    else:
        # ghosts rebuilt here: zero on the Dirichlet sides (the dense assembly drops those couplings), the image elsewhere
        a1 = matvec_ld(so, wrap_ld(np.ones_like(x) * pb.interior_mask(x.shape), per))
        r = inner(b).astype(np.longdouble) - matvec_ld(so, wrap_ld(x * pb.interior_mask(x.shape), per))
        t = np.sum(r * a1) / np.sum(a1 * a1)
        r = r - t * a1
        n = inner(x).size
        mean = abs(np.sum(inner(x).astype(np.longdouble))) / n
        assert mean <= (n + 2) * np.finfo(np.float64).eps * (np.max(np.abs(inner(x))) + abs(t)), (mean, float(t))
    worst = float(np.max(np.abs(r)) / np.max(np.abs(inner(b))))
    assert worst <= RESIDUAL_TOL, worst
    return worst


# ------------------------------------------------------------------ 1. band Cholesky, Dirichlet
def band_dims(shape):
    """(n, kd) of the coarsest system of a grid of shape (nx, ny[, nz])"""
    nx, ny = shape[0], shape[1]
    if len(shape) == 2:
        return nx * ny, nx + 1
    return nx * ny * shape[2], nx * (ny + 1) + 1


def band_in_lds(shape, pad=False):
    n, kd = band_dims(shape)
    nabd1, nabd2 = (kd + 1 + 4, n + 3) if pad else (kd + 1, n)
    return nabd1 * nabd2 + nabd2 + 2 <= LDS_DOUBLES


# (shape, nst, padded): padded = ABD(kd + 1 + 4, n + 3), a leading dimension and a column count beyond what the band needs
BAND2 = [((62, 4), 3, 0), ((62, 4), 5, 0), ((63, 5), 5, 0), ((64, 3), 3, 0), ((64, 3), 5, 0), ((130, 4), 3, 0),
         ((130, 4), 5, 0), ((255, 3), 5, 0), ((256, 5), 3, 0), ((256, 5), 5, 0), ((520, 3), 5, 0),
         ((49, 3), 3, 0), ((49, 3), 5, 0), ((50, 3), 3, 0), ((50, 3), 5, 0),   # the last shape staged in LDS, the first that is not
         ((2, 30), 5, 0), ((40, 2), 3, 0),                                     # extents of 2 (min_coarse = 2)
         ((40, 3), 5, 1), ((300, 3), 3, 1)]                                    # padded
BAND3 = [((6, 9, 4), 14, 0), ((6, 9, 4), 4, 0), ((7, 8, 4), 14, 0), ((7, 8, 4), 4, 0), ((8, 7, 4), 4, 0), ((8, 7, 4), 14, 0),
         ((17, 14, 3), 14, 0), ((17, 14, 3), 4, 0), ((16, 15, 3), 4, 0), ((16, 15, 3), 14, 0), ((26, 19, 3), 14, 0),
         ((6, 6, 4), 14, 0), ((7, 6, 4), 14, 0),                               # LDS / global
         ((2, 9, 8), 14, 0), ((30, 2, 5), 4, 0), ((12, 9, 2), 14, 0),          # extents of 2
         ((5, 6, 4), 14, 1), ((20, 13, 3), 4, 1)]                              # padded
BAND = BAND2 + BAND3


def band_aliased(shape):
    """nx = 2, or ny = 2 in 3D: two slots share a row of the band (W and NW lie 1 and nx - 1 columns back, S and BN nx and
    nx (ny - 1)), and the reference's assembly -- an assignment per slot, zeros included -- keeps the last: the S
    coupling of a 7-point operator with ny = 2 is overwritten by the zero of BN.  The oracle and the kernel reproduce
    that; the band is then not the operator, and only the bits are compared.  Extents of 2 that do not alias ((40, 2),
    (12, 9, 2)) are held against the operator like every other case."""
    return shape[0] == 2 or (len(shape) == 3 and shape[1] == 2)


def band_id(case):
    shape, nst, pad = case
    n, kd = band_dims(shape)
    return "%s_%d_n%d_kd%d%s" % ("x".join(str(v) for v in shape), nst, n, kd, "_padded" if pad else "")


def _band_coverage():
    """bands on both sides of every step of the two LAPACK restatements, and of the LDS switch within one grid row"""
    for tab in (BAND2, BAND3):
        kds = [band_dims(c[0])[1] for c in tab]
        for want in (64, 65, 256, 257):
            assert want in kds, (want, kds)
        assert any(kd <= 63 for kd in kds) and any(kd > 128 for kd in kds) and any(kd > 512 for kd in kds), kds
        shapes = {c[0] for c in tab if not c[2]}
        assert any(band_in_lds(s) and (s[0] + 1,) + s[1:] in shapes and not band_in_lds((s[0] + 1,) + s[1:]) for s in shapes)
        assert {c[1] for c in tab} == ({3, 5} if tab is BAND2 else {4, 14})
        pads = [band_dims(c[0])[1] for c in tab if c[2]]
        assert any(kd < 64 for kd in pads) and any(kd > 256 for kd in pads), pads
        assert sum(1 for c in tab if 2 in c[0]) >= 2
        for c in tab:  # the oracle factors at about 0.5 GFlop/s: a second per case at the most
            n, kd = band_dims(c[0])
            assert n * kd * kd <= 5e8, (c, n * kd * kd)


_band_coverage()

PAD_SEED = 97


def band_solve(impl, case, trim=False):
    """set-up and one solve of a case through impl (the oracle or the C ABI): the whole ABD array, x, and the inputs"""
    shape, nst, pad = case
    n, kd = band_dims(shape)
    g = tuple(v + 2 for v in reversed(shape))
    sd = cases._seed(band_id((shape, nst, 0)))  # a padded case and its plain twin share the problem
    so = pb.random_op(g, nst, sd)
    if trim:
        so = trimmed(so)
    b = pb.uniform(g, sd + 1, -1, 1)
    abd = np.zeros((n + 3, kd + 1 + 4) if pad else (n, kd + 1))
    if pad:  # everything outside the band's n columns of kd + 1 entries
        junk = pb.uniform(abd.shape, PAD_SEED, 1, 2)
        abd[n:, :] = junk[n:, :]
        abd[:, kd + 1:] = junk[:, kd + 1:]
    x = np.zeros(g)
    if len(shape) == 2:
        impl.setup_cg2(so, abd)
        impl.solve_cg2(x, b, abd)
    else:
        impl.setup_cg3(so, abd)
        impl.solve_cg3(x, b, abd)
    return {"abd": abd, "x": x, "so": so, "b": b}


def band_solve_trimmed(impl, case):
    return band_solve(impl, case, trim=True)


_RESULTS = {}


def result(impl, tag, fn, case):
    """fn(impl, case), computed once per (implementation, case) and shared by the tests; never modified"""
    key = (tag, fn.__name__, case)
    if key not in _RESULTS:
        _RESULTS[key] = fn(impl, case)
    return _RESULTS[key]


def check_band_bits(got, want_of, case):
    """want_of(case) -> the oracle's result.  A padded case is held against the oracle's run of the same problem in an
    array of exactly (n, kd + 1): the same bits in the band, the padding as it came in."""
    shape, nst, pad = case
    n, kd = band_dims(shape)
    want = want_of((shape, nst, 0) if pad else case)
    abd = got["abd"]
    if pad:
        junk = pb.uniform(abd.shape, PAD_SEED, 1, 2)
        assert np.array_equal(abd[n:, :], junk[n:, :]) and np.array_equal(abd[:, kd + 1:], junk[:, kd + 1:])
        abd = abd[:n, :kd + 1]
    diff = abd != want["abd"]
    # a differing entry names its column step and its trip: (column of the matrix, row of the band)
    assert not diff.any(), (band_id(case), int(diff.sum()), np.argwhere(diff)[:8].tolist())
    diff = got["x"] != want["x"]
    assert not diff.any(), (band_id(case), int(diff.sum()), np.argwhere(diff)[:8].tolist())


@pytest.mark.parametrize("case", BAND, ids=band_id)
def test_band_factor_and_solve_vs_oracle(K, oracle, case):
    """setup_cg2/3 and solve_cg2/3 through the C ABI: the whole factor and the solution, bit for bit the oracle's
    DPBTF2 / DTBSV restatement"""
    check_band_bits(result(K, "K", band_solve, case), lambda c: result(oracle, "oracle", band_solve, c), case)


# ------------------------------------------------------------------ 2. the answer solves the system
@pytest.mark.parametrize("case", BAND, ids=band_id)
def test_band_solution_solves_the_system(K, oracle, case):
    """the same cases on the operator without couplings across the boundary -- the only kind whose band matrix is the
    operator (see trimmed) -- again bit for bit, and b - A x by the matvec of this file"""
    got = result(K, "K", band_solve_trimmed, case)
    check_band_bits(got, lambda c: result(oracle, "oracle", band_solve_trimmed, c), case)
    assert not got["x"][~pb.interior_mask(got["x"].shape)].any()
    if not band_aliased(case[0]):
        check_residual(got["so"], got["b"], got["x"])


# ------------------------------------------------------------------ 3. dense Cholesky, 3D periodic
# N on both sides of the 1024-thread step and at the admitted limit; per_z, per_xyz (assembled wrongly by the reference),
# per_x, per_yz; an extent of 2 in y (two slots name the same pair: the assembly keeps the serial order)
DENSE3 = [("f11x3x31_z", 11, 3, 31, 5), ("f16x8x8_xyz", 16, 8, 8, 8), ("f5x5x41_x", 5, 5, 41, 2), ("f8x16x16_yz", 8, 16, 16, 7),
          ("f4x2x4_y", 4, 2, 4, 1)]
assert sorted(c[1] * c[2] * c[3] for c in DENSE3)[1:] == [1023, 1024, 1025, 2048]


def aliased(per, shape):
    """an extent of 2 in a periodic direction: the stencil names the same pair of unknowns twice (to the left and, round
    the wrap, to the right), and the reference's assembly -- an assignment per coefficient -- keeps the last one only.
    The oracle and the kernels reproduce that; the matrix is then not the periodic operator, and only the bits are
    compared."""
    return any(p and n == 2 for p, n in zip(per, shape))


def dense3_solve(impl, case):
    out = cases.coarse_solve_per3(impl, case)
    name, nx, ny, nz, ibc = case
    sd = cases._seed(name)
    out["so"] = pb.periodic_random_op3(nx, ny, nz, 14, pb.per3_of(ibc), sd)
    out["b"] = pb.uniform(out["q"].shape, sd + 1, -1, 1)
    return out


@pytest.mark.parametrize("case", DENSE3, ids=lambda c: "%s_N%d" % (c[0], c[1] * c[2] * c[3]))
def test_periodic3_dense_factor_and_solve(K, oracle, case):
    """setup_cg3_per / solve_cg3_per: the upper triangle of the factor and q (ghosts included) bit for bit the oracle's
    DPOTF2 / DPOTRS order; q solves the wrapped operator up to the mean the solve removes"""
    got, want = result(K, "K", dense3_solve, case), result(oracle, "oracle", dense3_solve, case)
    diff = got["abd_upper"] != want["abd_upper"]
    assert not diff.any(), (case[0], int(diff.sum()), np.flatnonzero(diff)[:8].tolist())
    assert np.array_equal(got["q"], want["q"]), np.argwhere(got["q"] != want["q"])[:8].tolist()
    per = pb.per3_of(case[4])
    assert np.array_equal(got["q"], pb.wrap3(got["q"].copy(), per))
    if not aliased(per, case[1:4]):
        check_residual(got["so"], got["b"], got["q"], per)


def test_periodic3_coarsest_level_limit(capi, oracle, capfd):
    """(32, 20, 26) periodic in x: two levels leave (16, 10, 13) = 2080 unknowns for the dense factor -- refused, no
    solver, the reason on the error stream; three levels leave (8, 5, 7) and run like the oracle"""
    so = pb.periodic_random_op3(32, 20, 26, 14, (1, 0, 0), 21)
    b = pb.periodic_rhs3(32, 20, 26, (1, 0, 0))
    st = dict(relax="point", nrelax_pre=2, nrelax_post=1, ibc=2)
    capfd.readouterr()
    with pytest.raises(RuntimeError):
        capi.Solver(so, num_levels=2, **st)
    assert "at most 2048 unknowns on the coarsest level" in capfd.readouterr().err
    s = capi.Solver(so, num_levels=3, max_iter=4, **st)  # tol 1e-8 on both sides
    assert s.nlevels() == 3 and s.dims(1) == (16, 10, 13) and s.dims(2) == (8, 5, 7)
    x = np.zeros_like(b)
    h = s.solve(b, x)
    s.close()
    ml = oracle.ml_create(so, num_levels=3, **st)
    xo = np.zeros_like(b)
    want = ml.solve(b, xo, maxiter=4)
    ml.close()
    assert len(h) == len(want) >= 4  # three cycles to 1e-8 in the oracle: every one of them is compared
    np.testing.assert_allclose(h, want, rtol=1e-10, atol=1e-14)
    assert np.max(np.abs(x - xo)) <= 1e-11 * np.max(np.abs(xo))


# ------------------------------------------------------------------ 4. dense Cholesky, 2D periodic (one lane)
# (name, nx, ny, nst, ibc): N = 60 .. 128, both stencils, periodic in x (2), y (1) and both (3), odd and even extents,
# an extent of 2 in the periodic direction
DENSE2 = [("g10x6_5_x", 10, 6, 3, 2), ("g9x11_9_y", 9, 11, 5, 1), ("g11x10_9_xy", 11, 10, 5, 3), ("g8x15_5_xy", 8, 15, 3, 3),
          ("g16x8_9_x", 16, 8, 5, 2), ("g7x13_5_y", 7, 13, 3, 1), ("g2x40_9_x", 2, 40, 5, 2), ("g50x2_5_y", 50, 2, 3, 1)]
assert all(60 <= c[1] * c[2] <= 128 for c in DENSE2)
PER2 = {1: (0, 1), 2: (1, 0), 3: (1, 1)}


def dense2_solve(impl, case):
    """cases.coarse_solve_per with the factor's INFO (the oracle returns it; the C ABI reports a failure on the error
    stream) and the inputs"""
    name, nx, ny, nst, ibc = case
    sd = cases._seed(name)
    g = (ny + 2, nx + 2)
    so = pb.periodic_random_op(nx, ny, nst, PER2[ibc][0:2], sd)
    so[0] *= 4.0
    n = nx * ny
    abd = np.zeros((n, n))
    info = impl.setup_cg2(so, abd, ibc=ibc)
    b = pb.uniform(g, sd + 1, -1, 1)
    q = pb.uniform(g, sd + 2, -1, 1)
    impl.solve_cg2(q, b, abd, ibc=ibc)
    return {"abd_upper": abd.T[np.triu_indices(n)].copy(), "q": q, "so": so, "b": b, "info": info}


@pytest.mark.parametrize("case", DENSE2, ids=lambda c: "%s_N%d" % (c[0], c[1] * c[2]))
def test_periodic2_dense_factor_and_solve(K, oracle, case):
    """setup_cg2_per / solve_cg2_per on one lane, bit for bit the oracle's DPOTF2 / DPOTRS order: with random ghost
    coefficients (cases.coarse_solve_per: every entry the assembly reads is its own number) and with the periodic image
    in the ghosts, where q also solves the wrapped operator up to the mean the solve removes"""
    for fn in (cases.coarse_solve_per, dense2_solve):
        got, want = result(K, "K", fn, case), result(oracle, "oracle", fn, case)
        diff = got["abd_upper"] != want["abd_upper"]
        assert not diff.any(), (case[0], fn.__name__, int(diff.sum()), np.flatnonzero(diff)[:8].tolist())
        assert np.array_equal(got["q"], want["q"]), (fn.__name__, np.argwhere(got["q"] != want["q"])[:8].tolist())
    assert want["info"] == 0  # positive definite in the oracle
    per = PER2[case[4]]
    if not aliased(per, case[1:3]):
        check_residual(got["so"], got["b"], got["q"], per)


# ------------------------------------------------------------------ 5. the resident solver and the batch
def _rhs_items(b0, n=3):
    m = pb.interior_mask(b0.shape)
    return np.stack([b0] + [pb.uniform(b0.shape, 4242 + t, -1, 1) * m * np.max(np.abs(b0)) for t in range(1, n)])


# (id, operator, right-hand side, coarsest extents): the default min_coarse = 3 stops (520, 5) at (260, 3) -- n = 780,
# kd = 261, factor not staged in LDS -- and (9, 33, 5) at (5, 17, 3): n = 255, kd = 5 * 18 + 1 = 91
WIDE = {"varcoef9_520x5": (lambda: pb.varcoef9(520, 5), lambda: pb.rhs2(520, 5), (260, 3, 1)),
        "poisson5_520x5": (lambda: pb.poisson2(520, 5), lambda: pb.rhs2(520, 5), (260, 3, 1)),
        "fe27_9x33x5": (lambda: pb.fe3(9, 33, 5), lambda: pb.rhs3(9, 33, 5), (5, 17, 3))}


@pytest.mark.parametrize("name", list(WIDE), ids=str)
def test_resident_solver_history_on_a_wide_coarsest_level(capi, oracle, name):
    """six cycles of V(2,1) on a hierarchy of two levels whose direct solve has a band wider than a wavefront: the oracle's
    history iteration for iteration (the rule of test_resident_solver_history_on_long_rows) and its solution"""
    mk_op, mk_rhs, coarsest = WIDE[name]
    so, b = mk_op(), mk_rhs()
    ml = oracle.ml_create(so, nrelax_pre=2, nrelax_post=1)
    xo = np.zeros_like(b)
    want = ml.solve(b, xo, maxiter=6)
    ml.close()
    s = capi.Solver(so, nrelax_pre=2, nrelax_post=1, max_iter=6)
    assert s.nlevels() == 2 and s.dims(1) == coarsest, (s.nlevels(), s.dims(s.nlevels() - 1))
    x = np.zeros_like(b)
    h = s.solve(b, x)
    s.close()
    assert len(h) == len(want)
    np.testing.assert_allclose(h, want, rtol=1e-10, atol=1e-14)
    assert np.max(np.abs(x - xo)) <= 1e-12 * np.max(np.abs(xo))


@pytest.mark.parametrize("name", list(WIDE), ids=str)
def test_solve_many_on_a_wide_coarsest_level(capi, name):
    """three right-hand sides: item m carries the bits of solve on it alone -- bbd + nabd2 * item under a band of more than
    64 (the property of tests/test_gpu_many.py)"""
    mk_op, mk_rhs, coarsest = WIDE[name]
    so, b = mk_op(), _rhs_items(mk_rhs())
    # tol out of reach: the batch cycles an item on after it has met tol (lockstep), a single solve stops there; with
    # six cycles for everyone the solutions are comparable too
    sm = capi.Solver(so, max_iter=6, tol=1e-30, max_rhs=3)
    assert sm.max_rhs() == 3 and sm.dims(sm.nlevels() - 1) == coarsest
    xs = np.zeros_like(b)
    rel, iters = sm.solve_many(b, xs)
    sm.close()
    s1 = capi.Solver(so, max_iter=6, tol=1e-30)
    for m in range(3):
        x1 = np.zeros_like(b[m])
        h1 = s1.solve(b[m], x1)
        assert iters[m] == len(h1) - 1 == 6, (m, iters, len(h1))
        assert np.array_equal(rel[m][: iters[m] + 1], h1), (m, rel[m], h1)
        assert np.array_equal(xs[m], x1), (m, np.max(np.abs(xs[m] - x1)))
    s1.close()
    assert len(rel[0]) - 1 == max(iters)


@pytest.mark.parametrize("name", list(WIDE), ids=str)
def test_pcg_many_on_a_wide_coarsest_level(capi, name):
    """the same for conjugate gradients preconditioned by V(2,2): histories and solutions of pcg item by item"""
    from test_gpu_pcg_many import check_pcg_many
    mk_op, mk_rhs, coarsest = WIDE[name]
    so, b = mk_op(), _rhs_items(mk_rhs())
    st = dict(relax="point", nrelax_pre=2, nrelax_post=2)
    _, iters = check_pcg_many(capi, so, st, b, lambda: capi.Solver(so, **st), tol=1e-10)
    assert min(iters) > 1
