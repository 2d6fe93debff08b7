"""Reference statement of the semidefinite solve (cedar_amd_solver_create_semidefinite, cedar_amd_solver_fcg_semidefinite)
in numpy, on the unchanged oracle.

The operator is symmetric positive semidefinite with the constants as null space (zero row sums: pure Neumann, fully
periodic).  Two rules make the multigrid cycle serve it:

  set-up   the coarsest matrix is assembled as always and the diagonal entry of its LAST unknown is doubled before the
           Cholesky factorisation;
  solve    the mean of the coarse solution is removed after the triangular solves.

The oracle's multilevel handle does not look at the factorisation's return value, so `ml_create` makes the handle for
the singular operator (its own factorisation breaks down) and overwrites the coarsest factor in place with the upper
Cholesky factor of A_c + a_nn e_n e_n^T, A_c assembled here from the handle's coarsest operator and factored in the
operation order of the oracle's own routines (DPOTF2 dense, DPBTF2 band), so that the factor has their bits.  For ibc != 0 the
oracle's coarse solve removes the mean already; for ibc == 0 it does not, which changes iterates by constants only:
histories agree to rounding and the final x is projected anyway.

On top: P v = v - mean_interior(v) with the correctly rounded mean, and fcg_semidefinite = fcg_statement.fcg on the
plain or the wrapped oracle with r0 and the final x projected and the cycle applied as P M P.  solve_reference is the dense zero-mean least-squares solution.
"""
import ctypes as C
import math

import numpy as np

import fcg_periodic_statement as fps
import fcg_statement as fs
import pcg_statement as ps
import problems as pb

inner = ps.inner


def per_of(nd, ibc):
    """(periodic_x, periodic_y, periodic_z) of a boundary code, 0 included"""
    return (0, 0, 0) if ibc == 0 else fps.per_of(nd, ibc)


def mean_interior(v):
    """the correctly rounded mean over the interior: math.fsum is exact, the division rounds once.  The device kernel
    carries its sum in two doubles and gives the same bits (tests/test_gpu_semidefinite.py)"""
    w = inner(v)
    return math.fsum(w.ravel().tolist()) / w.size


def project(v):
    """P v = v - mean_interior(v) on the interior, in place; ghosts untouched.  Returns the mean removed"""
    m = mean_interior(v)
    inner(v)[...] -= m
    return m


def assemble(A, ibc):
    """dense matrix of the level operator A (slots, [KK,] JJ, II) over the interior unknowns, i fastest: every coupling
    stored at an interior point, both of its ends taken through the wrap of the periodic directions; an end on the ghost
    layer of a non-periodic direction drops the coupling"""
    nd = A.ndim - 1
    per = per_of(nd, ibc)[:nd][::-1]  # array (slowest-first) order
    ext = tuple(n - 2 for n in A.shape[1:])
    N = int(np.prod(ext))
    offs = pb.slot_offsets(nd, A.shape[0])
    M = np.zeros((N, N))
    idx = np.arange(N).reshape(ext)
    P = np.indices(ext)

    def unknown(o):
        ok = np.ones(ext, dtype=bool)
        c = []
        for d in range(nd):
            q = P[d] + o[d]
            if per[d]:
                q = q % ext[d]
            else:
                ok &= (q >= 0) & (q < ext[d])
                q = np.clip(q, 0, ext[d] - 1)
            c.append(q)
        return idx[tuple(c)], ok

    for s in range(A.shape[0]):
        v = inner(A[s])
        a, oka = unknown(offs[s][0])
        b, okb = unknown(offs[s][1])
        ok = oka & okb
        if s == 0:
            np.add.at(M, (a[ok], b[ok]), v[ok])
        else:
            np.add.at(M, (a[ok], b[ok]), -v[ok])
            np.add.at(M, (b[ok], a[ok]), -v[ok])
    return M


def coarsest(ml):
    """(level index, operator) of the handle's coarsest level"""
    last = ml.nlevels() - 1
    return last, ml.array(last, "A")


def _potf2_upper(B):
    """DPOTF2 'U' in the reference-BLAS operation order the oracle and the device share (dot, sqrt, gemv, scal; sums in
    increasing row index, no fused multiply-add): the factor's bits, not only its value"""
    U = np.triu(B).copy()
    n = U.shape[0]
    for j in range(n):
        dot = 0.0
        for i in range(j):
            dot = dot + U[i, j] * U[i, j]
        ajj = U[j, j] - dot
        assert ajj > 0.0, j
        ajj = math.sqrt(ajj)
        U[j, j] = ajj
        if j + 1 < n:
            temp = np.zeros(n - j - 1)
            for i in range(j):
                temp = temp + U[i, j + 1:] * U[i, j]
            U[j, j + 1:] = (1.0 / ajj) * (U[j, j + 1:] + (-1.0) * temp)
    return U


def _pbtf2_upper(B, kd):
    """DPBTF2 'U' with bandwidth kd in its operation order (pivot, scaling, rank-one update of the trailing band block)"""
    W = np.triu(B).copy()
    n = W.shape[0]
    for j in range(n):
        ajj = W[j, j]
        assert ajj > 0.0, j
        ajj = math.sqrt(ajj)
        W[j, j] = ajj
        kn = min(kd, n - 1 - j)
        if kn > 0:
            x = (1.0 / ajj) * W[j, j + 1: j + 1 + kn]
            W[j, j + 1: j + 1 + kn] = x
            W[j + 1: j + 1 + kn, j + 1: j + 1 + kn] += np.triu(np.outer(x, -1.0 * x))
    return W


def bumped_factor(Ac, kd=None):
    """upper Cholesky factor of A_c with its last diagonal entry doubled, in the operation order of the coarsest set-up:
    the dense routine, or the band routine when a bandwidth is given"""
    B = Ac.copy()
    B[-1, -1] = B[-1, -1] + B[-1, -1]
    return _potf2_upper(B) if kd is None else _pbtf2_upper(B, kd)


def _band(U, kd, size):
    """U in LAPACK upper band storage AB(kd + 1 + i - j, j) = U(i, j) with ldab = kd + 1, flat"""
    N = U.shape[0]
    ldab = kd + 1
    assert size == ldab * N, (size, ldab, N)
    ab = np.zeros((N, ldab))  # ab[j, r] = AB(r + 1, j + 1)
    for j in range(N):
        lo = max(0, j - kd)
        ab[j, kd + lo - j: kd + 1] = U[lo: j + 1, j]
    assert np.all(np.triu(U, kd + 1) == 0)
    return ab.reshape(-1)


def ml_create(oracle, so, ibc, **kw):
    """the oracle's handle for the semidefinite operator so, its coarsest factor replaced in place.  Returns (ml, Ac):
    the handle and the assembled coarsest matrix (without the bump)"""
    ml = oracle.ml_create(so, ibc=ibc, **kw)
    nd = so.ndim - 1
    last, A = coarsest(ml)
    Ac = assemble(A, ibc)
    nx, ny, _ = ml.dims(last)
    kd = None if ibc != 0 else nx + 1 if nd == 2 else nx * (ny + 1) + 1
    U = bumped_factor(Ac, kd)
    n = C.c_size_t()
    ptr = oracle.L.orc_ml_level_array(ml.h, last, b"ABD", C.byref(n))
    dst = np.ctypeslib.as_array(ptr, shape=(n.value,))
    N = U.shape[0]
    if ibc != 0:
        assert n.value == N * N, (n.value, N)
        dst[:] = np.triu(U).T.reshape(-1)  # column-major, leading dimension N
    else:
        dst[:] = _band(U, kd, n.value)
    return ml, Ac


class Cycle:
    """the handle's cycle as fcg_statement wants it (ibc == 0) -- fcg_periodic_statement wraps it itself otherwise"""

    def __init__(self, ml):
        self.ml = ml

    def vcycle(self, z, r):
        self.ml.vcycle(z, r)


def apply_A(oracle, so, v, ibc):
    if ibc == 0:
        return ps.apply_A(oracle, so, v)
    return fps.apply_A(oracle, so, v, per_of(so.ndim - 1, ibc))


class ProjectedCycle:
    """the preconditioner P M P: r is projected (a copy) before the cycle and z after it.  In exact arithmetic the
    recurrence sees no difference (w = A p has no constant part); in floating point the rounding of w leaves a constant in
    r that never shrinks and that the cycle answers with a large smooth correction, and the constant the cycle leaves in
    z is cancellation noise in the next w.  Measured on the cases of tests/semidefinite_cases.py: z times
    (1 + 1.1e-16 U(-1,1)) plus a constant of 0.37 max|z| after every cycle moves the history entries above 1e-10 by
    4e-7 to 4e-6 of their value without the two projections, by 4e-11 to 3e-7 with z alone projected, and by 3e-14 to
    6e-13 with both"""

    def __init__(self, cycle):
        self.cycle = cycle

    def vcycle(self, z, r):
        rr = np.array(r)
        project(rr)
        self.cycle.vcycle(z, rr)
        project(z)


def fcg_semidefinite(oracle, so, b, x, ml, ibc, projected=True, **kw):
    """solves A x = P b with mean(x) = 0: x (interior) updated in place, returns (iterations, hist) with
    hist[0] = |P (b - A x0)|.  b is not written.  The loop is handed r0 = P (b - A x0) as its right-hand side and a zero
    start, so that it forms r0 - A 0 = r0 with exactly these bits, and its result is the correction to x0.  The multigrid
    preconditioner is P M P (ProjectedCycle); precon none / diag are taken as they are.  projected=False: the plain
    recurrence, r0 and the final x alone projected and the cycle as it is (the same in exact arithmetic)"""
    mask = pb.interior_mask(b.shape)
    x *= mask
    r0 = np.zeros_like(b)
    inner(r0)[...] = inner(b * mask - apply_A(oracle, so, x, ibc))
    project(r0)
    dx = np.zeros_like(x)
    per = per_of(so.ndim - 1, ibc)
    cycle = Cycle(ml) if ibc == 0 else fps.WrappedCycle(ml, per)
    it, hist = fs.fcg(oracle if ibc == 0 else fps.WrappedOracle(oracle, per), so, r0, dx,
                      ml=ProjectedCycle(cycle) if projected else cycle, **kw)
    inner(x)[...] += inner(dx)
    project(x)
    return it, hist


def stationary(oracle, so, b, x, ml, ibc, max_iter=50, tol=1e-8):
    """x += M (P b - A x) until |r| / |r0| < tol; returns (iterations, hist) with hist as fcg's"""
    bp = b * pb.interior_mask(b.shape)
    project(bp)
    if ibc != 0:
        return fps.stationary(oracle, so, bp, x, ml, ibc, max_iter=max_iter, tol=tol)

    def res():
        r = np.zeros_like(bp)
        inner(r)[...] = inner(bp - ps.apply_A(oracle, so, x))
        return r

    r = res()
    r0 = np.sqrt(ps.dot(r, r))
    hist = [r0]
    for _ in range(max_iter):
        z = np.zeros_like(r)
        ml.vcycle(z, r)
        inner(x)[...] += inner(z)
        r = res()
        hist.append(np.sqrt(ps.dot(r, r)) / r0)
        if not np.isfinite(hist[-1]) or hist[-1] < tol:
            break
    return len(hist) - 1, np.array(hist)


def true_residual(oracle, so, b, x, ibc):
    """|P b - A x|_2 over the interior"""
    bp = b * pb.interior_mask(b.shape)
    project(bp)
    return float(np.linalg.norm(inner(bp - apply_A(oracle, so, x * pb.interior_mask(x.shape), ibc))))


def solve_reference(so, b, ibc):
    """(x*, kappa): the zero-mean least-squares solution of A x = P b on the assembled level-0 matrix, as a level array
    with zero ghosts, and kappa = lambda_max / lambda_min+ of A"""
    A = assemble(so, ibc)
    bp = np.array(inner(b))
    bp -= bp.mean()
    y = np.linalg.lstsq(A, bp.reshape(-1), rcond=None)[0]
    y -= y.mean()
    x = np.zeros_like(b)
    inner(x)[...] = y.reshape(bp.shape)
    lam = np.linalg.eigvalsh(A)
    return x, float(lam[-1] / lam[1])


def kappa_plus(Ac):
    lam = np.linalg.eigvalsh(Ac)
    return float(lam[-1] / lam[1])
