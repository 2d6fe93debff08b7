"""Reference statement of flexible conjugate gradients on a periodic handle (cedar_amd_solver_fcg_periodic) in numpy.

It is fcg_statement.fcg itself with two changes, made by handing it two thin wrappers:

  A v   the oracle's matvec of a COPY of v whose periodic directions were wrapped first (problems.wrap3; a 2D array is
        wrapped as one plane), so the ghost layers of v never matter;
  M r   the oracle's periodic cycle from zero on a wrapped copy of r, the result masked to the interior.

Everything else -- the Polak-Ribiere beta formed as -((alpha * w.z) / rho), the stop tests, the breakdown rules, the
history -- is fcg_statement's.  `standard` runs the same loop with pcg_statement.pcg (beta = rho_new / rho_old), and
`stationary` is the defect-correction iteration x += M (b - A x) the periodic solve amounts to; both only serve the
comparison of iteration counts in tests/test_fcg_periodic_statement.py.
"""
import numpy as np

import fcg_statement as fs
import pcg_statement as ps
import problems as pb

inner = ps.inner


def per_of(nd, ibc):
    """(periodic_x, periodic_y, periodic_z) of a boundary code"""
    if nd == 2:
        return {1: (0, 1, 0), 2: (1, 0, 0), 3: (1, 1, 0)}[ibc]
    return pb.per3_of(ibc)


def wrap(a, per):
    """the periodic image into the ghost layers of a 2D or 3D array, in place"""
    pb.wrap3(a if a.ndim == 3 else a[None], per)
    return a


def masked(a):
    return a * pb.interior_mask(a.shape)


class WrappedOracle:
    """matvec2 / matvec3 of the oracle on a wrapped copy of the vector"""

    def __init__(self, oracle, per):
        self.oracle, self.per = oracle, per

    def matvec2(self, so, q, qf):
        self.oracle.matvec2(so, wrap(np.array(q), self.per), qf)

    def matvec3(self, so, q, qf):
        self.oracle.matvec3(so, wrap(np.array(q), self.per), qf)


class WrappedCycle:
    """the oracle's periodic cycle on a wrapped copy of r; z comes back with zero ghosts"""

    def __init__(self, ml, per):
        self.ml, self.per = ml, per

    def vcycle(self, z, r):
        wrap(z, self.per)  # zero stays zero; a second cycle of nmg > 1 finds its iterate consistent
        self.ml.vcycle(z, wrap(np.array(r), self.per))
        z *= pb.interior_mask(z.shape)


def apply_A(oracle, so, v, per):
    return ps.apply_A(WrappedOracle(oracle, per), so, v)


def fcg_periodic(oracle, so, b, x, ml, ibc, standard=False, **kw):
    """x (interior) updated in place; returns (iterations, hist).  ml: the oracle's handle made with the same ibc"""
    per = per_of(so.ndim - 1, ibc)
    bm = masked(b)
    x *= pb.interior_mask(x.shape)
    return (ps.pcg if standard else fs.fcg)(WrappedOracle(oracle, per), so, bm, x, ml=WrappedCycle(ml, per), **kw)


def stationary(oracle, so, b, x, ml, ibc, max_iter=50, tol=1e-8):
    """x += M (b - A x) until ||r|| / ||r0|| < tol; returns (iterations, hist) with hist as fcg's"""
    per = per_of(so.ndim - 1, ibc)
    M = WrappedCycle(ml, per)

    def res():
        r = np.zeros_like(b)
        inner(r)[...] = inner(b - apply_A(oracle, so, x, per))
        return r

    r = res()
    r0 = np.sqrt(ps.dot(r, r))
    hist = [r0]
    for k in range(max_iter):
        z = np.zeros_like(r)
        M.vcycle(z, r)
        inner(x)[...] += inner(z)
        r = res()
        hist.append(np.sqrt(ps.dot(r, r)) / r0)
        if hist[-1] < tol:
            break
    return len(hist) - 1, np.array(hist)


def true_residual(oracle, so, b, x, ibc):
    """||b - A x||_2 over the interior, A x through the wrapped matvec"""
    per = per_of(so.ndim - 1, ibc)
    return float(np.linalg.norm(inner(b - apply_A(oracle, so, x, per))))


def symmetry_defect(oracle, ml, g, ibc, nd):
    """|<Mu,v> - <u,Mv>| / |<Mu,v>| for two random fields"""
    per = per_of(nd, ibc)
    M = WrappedCycle(ml, per)
    u, v = ps.random_field(g, 31), ps.random_field(g, 37)
    mu, mv = np.zeros(g), np.zeros(g)
    M.vcycle(mu, u)
    M.vcycle(mv, v)
    a, c = ps.dot(mu, v), ps.dot(u, mv)
    return abs(a - c) / abs(a)
