"""The line solves on data for which all arithmetic is exact (tests/line_exact.py): every comparison is np.array_equal.

The line kernels share one device routine, affine_scan (cedar_amd/csrc/lines_dev.h), which re-associates the DPTTRS
recurrences y_i = a_i y_(i-1) + c_i.  The other line tests run operators of problems.random_op, whose multipliers are
about 0.04: the product over one lane's chunk of 8 is below their 1e-12 tolerance, so the multiplier half of the scan
(the product in the Kogge-Stone step, the chain over the wavefronts, the carry between tiles, the multiplier tables of
the scan-ordered factor copy) is multiplied away before it reaches an unknown
(tests/test_line_exact_statement.py::test_carry_defects_are_invisible_on_random_op_multipliers).  Here every multiplier is
-1, 0 or +1 and every value a small multiple of a power of two, so any association has one correct result, which the
sequential reference of line_exact.py computes; that reference is the CPU oracle bit for bit on every case of this file
(test_line_exact_statement.py).

Entry points and what they reach:
  K.relax_lines2, ibc 0          line_pttrs on x lines; gather, ylines_solve and scatter on y lines
  K.relax_lines2, cyclic lines   the Sherman-Morrison closure, x (ibc 2, 3) and y (ibc 1, 3)
  K.relax2_lines_op32, _many     the float-factor kernels of linesf.hip: line_pttrs_pf on the scan-ordered float copy
                                 beyond 512 unknowns, the transposed y lines, the batch index
  cedar_amd_affine_lines         affine_lines_kernel of the distributed line relaxation, on device pointers
  K.setup_lines2                 DPTTRF on an operator on which it is exact, then the sweep on its factors

Not reachable with hand-made factors: the FP64 instantiation of line_pttrs_pf, lines_small.hip and the batched line
kernels of the resident solver take their factors from a handle, which computes them from its operator.  The kernels
themselves can be run from outside -- Solver.time_relax(x, b, n) runs n sweeps of a handle's level-0 smoother on the
caller's x and b, which tests/test_gpu_guarded_handles.py uses -- but not on factors made by hand.  For undamped
multipliers they rest on bit-identity tests against the kernels above --
test_line_solve_on_scan_ordered_factors_is_bit_identical, test_y_lines_on_transposed_arrays...,
test_small_level_line_sweeps... -- which run on aniso9, whose multipliers are near one over half the domain.  So the
chain of evidence for those variants is: the kernels tested here are exact on undamped data, and the variants have the
bits of these kernels on a weakly dominant operator.

CEDAR_AMD_LINE_BS is read once per process: the 512- and 1024-lane variants are not run here.
"""
import ctypes as C

import numpy as np
import pytest

import line_exact as le

pytestmark = pytest.mark.gpu

DOWN, UP = 0, 1


@pytest.fixture(scope="module")
def capi():
    from cedar_amd import capi
    assert capi.device_count() >= 1, "no GPU visible"
    return capi


@pytest.fixture(scope="module")
def K(capi):
    return capi.Kernels()


# (CEDAR_AMD_LINE_BS is latched at the first long line solve of the process: if an earlier test module ran one with 512 or
# 1024 lanes set, deleting the variable here changes nothing and line_exact.lanes_for no longer names the lanes in use.
# The expected values do not depend on it: on this data every association gives the same result.)
@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for v in ("CEDAR_AMD_LINE_BS", "CEDAR_AMD_LINE_PERM", "CEDAR_AMD_LINES_SMALL", "CEDAR_AMD_YLINES_TRANSPOSED",
              "CEDAR_AMD_YCHUNK", "CEDAR_AMD_LINE_DBG"):
        monkeypatch.delenv(v, raising=False)


def ghosts(a):
    m = np.ones(a.shape, dtype=bool)
    m[1:-1, 1:-1] = False
    return a[m]


def interior(a):
    return a[1:-1, 1:-1]


def first_difference(got, want):
    bad = np.argwhere(got != want)
    return None if not len(bad) else (tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])], len(bad))


# ---------------------------------------------------------------- 1. Dirichlet lines
@pytest.mark.parametrize("d", ["x", "y"])
@pytest.mark.parametrize("n", le.LENGTHS)
def test_dirichlet_sweep_is_the_sequential_sweep(K, n, d):
    """BMG2_SymStd_relax_lines_x / _y, DOWN and UP, five lines of n unknowns: every element of q, ghost cells included"""
    case = le.dirichlet_case(n, d)
    for ud in (DOWN, UP):
        want = le.sweep(case, ud)
        got = case.q0.copy()
        K.relax_lines2(case.so, case.qf, got, case.sor, ud, d)
        assert np.array_equal(interior(got), interior(want)), (n, d, ud, first_difference(got, want))
        assert np.array_equal(ghosts(got), ghosts(case.q0))
        assert not np.array_equal(got, case.q0)


# ---------------------------------------------------------------- 2. cyclic lines
@pytest.mark.parametrize("n", le.CYCLIC_LENGTHS)
@pytest.mark.parametrize("d,ibc", le.CYCLIC)
def test_cyclic_sweep_is_the_sequential_sweep_with_the_kernels_closure(K, d, ibc, n):
    """dyadic pivots, closure couplings in {1, 2, 3}: interiors against the reference; the ghost cells of the periodic
    directions are the periodic image of the result, the others are unchanged"""
    for nst in (3, 5):
        case = le.cyclic_case(n, d, ibc, nst)
        for ud in (DOWN, UP):
            want = le.sweep(case, ud, ibc)
            got = case.q0.copy()
            K.relax_lines2(case.so, case.qf, got, case.sor, ud, d, ibc)
            assert np.array_equal(interior(got), interior(want)), (n, d, ibc, nst, ud, first_difference(got, want))
            image = got.copy()
            le.wrap(image, ibc)
            assert np.array_equal(got, image)
            if ibc != 3:  # the rows (ibc 2) or columns (ibc 1) of ghost cells across the other direction, corners aside
                keep = (lambda a: a[[0, -1], 1:-1]) if ibc == 2 else (lambda a: a[1:-1, [0, -1]])
                assert np.array_equal(keep(got), keep(case.q0))
            assert np.array_equal(got, want)


# ---------------------------------------------------------------- 3. float factors
def items_of(case, nitems):
    """`nitems` pairs (qf, q0) for one operator and one factor array: the case's own, then fresh integers"""
    rng = np.random.default_rng(31 + case.n)
    out = [case]
    for m in range(1, nitems):
        g = case.q0.shape
        out.append(case._replace(qf=rng.integers(-4, 5, g).astype(np.float64), q0=rng.integers(-4, 5, g).astype(np.float64)))
    return out


@pytest.mark.parametrize("dyadic", [False, True], ids=["unit", "dyadic"])
@pytest.mark.parametrize("d", [0, 1], ids=["x", "y"])
@pytest.mark.parametrize("n", le.LENGTHS)
def test_float_factor_sweeps_are_the_sequential_sweep(K, n, d, dyadic):
    """cedar_amd_relax2_lines_op32 and _many_op32 (nrhs = 3, another qf and q per item, a fourth item that must keep its
    bits).  Every entry of the operator and of the factors is a small integer or a power of two, so the float copies are
    exact and the expected values are the FP64 reference's; item m equals the single call"""
    nrhs = 3
    items = items_of(le.dirichlet_case(n, "xy"[d], dyadic), nrhs + 1)
    case = items[0]
    assert np.array_equal(case.so.astype(np.float32), case.so) and np.array_equal(case.sor.astype(np.float32), case.sor)
    qf, q0 = np.stack([c.qf for c in items]), np.stack([c.q0 for c in items])
    for ud in (DOWN, UP):
        want = [le.sweep(c, ud) for c in items[:nrhs]]
        single = [c.q0.copy() for c in items[:nrhs]]
        for m in range(nrhs):
            assert K.relax2_lines_op32(case.so, items[m].qf, single[m], case.sor, d, ud) == 0
            assert np.array_equal(single[m], want[m]), (n, d, ud, m, first_difference(single[m], want[m]))
        got = q0.copy()
        assert K.relax2_lines_many_op32(case.so, qf, got, case.sor, d, ud, nrhs=nrhs) == 0
        for m in range(nrhs):
            assert np.array_equal(got[m], single[m]), (n, d, ud, m, first_difference(got[m], single[m]))
        assert np.array_equal(got[nrhs], q0[nrhs])


# ---------------------------------------------------------------- 4. the generic recurrence
@pytest.mark.parametrize("with_div", [False, True], ids=["nodiv", "div"])
@pytest.mark.parametrize("n", le.AFFINE_LENGTHS)
def test_affine_lines_is_the_sequential_recurrence(capi, n, with_div):
    """cedar_amd_affine_lines on device pointers: three lines with ld = n + 3 (so the lines are not 16-byte aligned),
    forward and backward, a in {-1, 0, +1}, div NULL or powers of two; the ld - n cells after each line keep their values"""
    # (a prototype of its own: the shared library object keeps the argument types other callers rely on)
    f = C.CFUNCTYPE(None, *([C.c_void_p] * 3 + [C.c_int] * 4))(("cedar_amd_affine_lines", capi.lib))
    y, a, div = le.make_affine(n, 5000 + n, with_div)
    nlines, ld = y.shape
    assert ld == n + 3 and nlines == 3
    da = capi.DeviceArray.from_numpy(a)
    dd = capi.DeviceArray.from_numpy(div) if with_div else None
    for reverse in (0, 1):
        want = le.affine_reference(y, a, div, n, reverse)
        dy = capi.DeviceArray.from_numpy(y)
        f(dy.ptr, da.ptr, dd.ptr if with_div else None, nlines, n, ld, reverse)
        capi.sync()
        got = dy.numpy()
        dy.free()
        assert np.array_equal(got[:, :n], want[:, :n]), (n, with_div, reverse, first_difference(got, want))
        assert np.array_equal(got[:, n:], y[:, n:])
        assert not np.array_equal(got, y) or n == 1
    da.free()
    if dd is not None:
        dd.free()


# ---------------------------------------------------------------- 5. factorisation, then the sweep on its factors
@pytest.mark.parametrize("d", ["x", "y"])
@pytest.mark.parametrize("n", le.SETUP_LENGTHS)
def test_setup_is_exact_and_the_sweep_on_its_factors_is_the_sequential_sweep(K, n, d):
    """BMG2_SymStd_SETUP_lines_x / _y on the operator with couplings 2**k and diagonal 2 * 2**k (2**k at the first
    unknown): pivots 2**k, multipliers -1, nothing else written; then the sweep with the factors it returned"""
    case, want_sor = le.setup_case(n, d)
    sor = np.zeros_like(want_sor)
    K.setup_lines2(case.so, sor, d)
    assert np.array_equal(sor, want_sor), first_difference(sor, want_sor)
    case = case._replace(sor=sor)
    for ud in (DOWN, UP):
        want = le.sweep(case, ud)
        got = case.q0.copy()
        K.relax_lines2(case.so, case.qf, got, sor, ud, d)
        assert np.array_equal(got, want), (n, d, ud, first_difference(got, want))
