"""Statement of the single-precision interpolation weights (cedar_amd_solver_use_fp32_interpolation)
on the CPU oracle: every level's P of an oracle hierarchy is rounded to float in place, which is what the switched
handle's transfers read.

The weights enter a cycle through the coarse-grid correction only, never through the residual, and R = P^T uses the same
rounded weights: the iteration keeps its fixed point and the preconditioner stays symmetric.  So the cycle counts of
`solve` V(2,1) and the iteration counts of pcg V(1,1) (pcg_statement.pcg) to 1e-10 are those of the FP64 weights, and every
history entry stays within a relative 1e-4 of the FP64 one (measured: at most 4.6e-6, the table below), except on
high_contrast7, where only equal counts and a final residual below the tolerance are asserted (measured 3.4e-4).

Right-hand sides: splitmix fields of seed 17 in [-1, 1] on the interior, x0 = 0.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import pcg_statement as ps
import problems as pb
from pyoracle import Oracle

TOL = 1e-10
HIST_RTOL = 1e-4

# name -> (operator, relaxation, solve cycles, measured history deviation of solve, pcg iterations)
TABLE = {
    "fe3": (lambda: pb.fe3(33, 33, 33), "point", 9, 4.0e-7, 8),
    "poisson3": (lambda: pb.poisson3(40, 33, 50), "point", 13, 1.1e-7, None),
    "dd3": (lambda: pb.diag_diffusion3(40, 33, 50, 1.0, 0.8, 1.3), "point", 18, 2.5e-9, 15),
    "vc9-point": (lambda: pb.varcoef9(129, 97), "point", 10, 7.2e-7, 8),
    "vc9-xy": (lambda: pb.varcoef9(129, 97), "line-xy", 9, 1.5e-6, 7),
    "an9-xy": (lambda: pb.aniso9(129, 97), "line-xy", 12, 4.6e-6, 9),
    "poisson2": (lambda: pb.poisson2(200, 130), "point", 11, 1.0e-6, None),
    "hc7": (lambda: ps.high_contrast7(24, 24, 24), "point", None, None, 15),
}


def rt(a):
    return a.astype(np.float32).astype(np.float64)


@pytest.fixture(scope="module")
def O():
    return Oracle()


@functools.lru_cache(maxsize=None)
def problem(name):
    so = TABLE[name][0]()
    g = so.shape[1:]
    b = pb.uniform(g, 17, -1, 1) * pb.interior_mask(g)
    so.setflags(write=False)
    b.setflags(write=False)
    return so, b


def round_weights(ml):
    """every level's P of the oracle hierarchy rounded to float, in place; returns the number of levels changed"""
    n, changed = C.c_size_t(), 0
    for l in range(ml.nlevels()):
        ptr = ml.o.L.orc_ml_level_array(ml.h, l, b"P", C.byref(n))
        if not ptr or n.value == 0:
            continue
        a = np.ctypeslib.as_array(ptr, shape=(n.value,))
        r = rt(a)
        changed += int(not np.array_equal(r, a))
        a[...] = r
    return changed


def hierarchy(O, name, rounded, **cycle):
    so, _ = problem(name)
    ml = O.ml_create(so, relax=TABLE[name][1], **cycle)
    if rounded:
        assert round_weights(ml) > 0  # the weights are not float-representable: the rounded cycle does differ
    return ml


def deviation(h, h0):
    assert len(h) == len(h0)
    return float(np.max(np.abs(h - h0) / np.abs(h0)))


@pytest.mark.parametrize("name", [k for k, v in TABLE.items() if v[2] is not None])
def test_solve_keeps_its_cycle_count_history_and_solution(O, name):
    so, b = problem(name)
    out = []
    for rounded in (False, True):
        ml = hierarchy(O, name, rounded, nrelax_pre=2, nrelax_post=1)
        x = np.zeros_like(b)
        h = ml.solve(b, x, maxiter=40, tol=TOL)
        ml.close()
        out.append((h, x))
    (h0, x0), (h1, x1) = out
    cycles = TABLE[name][2]
    print(name, "cycles", len(h0) - 1, len(h1) - 1, "history deviation", deviation(h1, h0), "x",
          np.max(np.abs(x1 - x0)) / np.max(np.abs(x0)))
    assert len(h0) - 1 == len(h1) - 1 == cycles
    assert h0[-1] < TOL and h1[-1] < TOL
    assert deviation(h1, h0) <= HIST_RTOL
    # the same fixed point: the two iterates differ by what is left of the error, far below 1e-12 of the solution
    assert np.max(np.abs(x1 - x0)) <= 1e-12 * np.max(np.abs(x0))


@pytest.mark.parametrize("name", [k for k, v in TABLE.items() if v[4] is not None])
def test_pcg_keeps_its_iteration_count_and_history(O, name):
    so, b = problem(name)
    out = []
    for rounded in (False, True):
        ml = hierarchy(O, name, rounded, nrelax_pre=1, nrelax_post=1)
        x = np.zeros_like(b)
        it, h = ps.pcg(O, so, b, x, ml=ml, max_iter=60, tol=TOL)
        ml.close()
        out.append((it, h))
    (it0, h0), (it1, h1) = out
    print(name, "iterations", it0, it1, "history deviation", deviation(h1, h0) if it0 == it1 else None)
    assert it0 == it1 == TABLE[name][4]
    assert h0[-1] < TOL and h1[-1] < TOL
    if name != "hc7":
        assert deviation(h1, h0) <= HIST_RTOL


def test_the_measured_deviations_leave_a_factor_of_twenty():
    worst = max(v[3] for v in TABLE.values() if v[3] is not None)
    assert worst == 4.6e-6 and HIST_RTOL >= 20 * worst
