"""Reference statement of the multigrid-preconditioned conjugate gradient (cedar_amd_solver_pcg) in numpy.

A p comes from the oracle's matvec (the C restatement of BMG{2,3}_SymStd_UTILS_matvec), M^-1 r from the oracle's
multilevel handle (nmg V-cycles started at zero), or from the diagonal / identity.  The loop, the stop tests and the
breakdown rules are those of the library: BoxMG's numbering, hist[0] = ||r0||_2, hist[i] = ||r_i||_2 / ||r0||_2.

Also the high-contrast 7-point operator of the issue (two-phase coefficients, contrast 1e6) and the A-norm.
"""
import numpy as np

import problems as pb


def inner(a):
    return a[tuple(slice(1, -1) for _ in a.shape)]


def dot(u, v):
    return float(np.dot(inner(u).ravel(), inner(v).ravel()))


def apply_A(oracle, so, v):
    out = np.zeros_like(v)
    (oracle.matvec2 if so.ndim == 3 else oracle.matvec3)(so, np.ascontiguousarray(v), out)
    return out


def a_norm(oracle, so, e):
    return np.sqrt(max(dot(e, apply_A(oracle, so, e)), 0.0))


def pcg(oracle, so, b, x, ml=None, precon="mg", max_iter=50, tol=1e-8, stop="rel_l2", nmg=1):
    """x updated in place; returns (iterations, hist)"""
    def M(r):
        if precon == "none":
            return r.copy()
        z = np.zeros_like(r)
        if precon == "diag":
            inner(z)[...] = inner(r) / inner(so[0])
            return z
        for _ in range(nmg):
            ml.vcycle(z, r)
        return z

    mnorm, rel = stop in ("abs_m", "rel_m"), stop in ("rel_l2", "rel_m")
    r = np.zeros_like(b)
    inner(r)[...] = inner(b - apply_A(oracle, so, x))
    z = M(r)
    rr, rho = dot(r, r), dot(r, z)
    r0, m0 = np.sqrt(rr), np.sqrt(max(rho, 0.0))
    hist = [r0]

    def stopped(rr, rz):
        v = np.sqrt(max(rz, 0.0)) if mnorm else np.sqrt(rr)
        return (v / (m0 if mnorm else r0) if rel else v) < tol

    if r0 == 0.0 or not rho > 0 or stopped(rr, rho):
        return 0, np.array(hist)
    p, beta, it = None, 0.0, 0
    for k in range(max_iter):
        p = z.copy() if k == 0 else z + beta * p  # z and p keep zero ghosts
        w = apply_A(oracle, so, p)
        sigma = dot(p, w)
        if not (sigma > 0 and np.isfinite(sigma)) or rho == 0:
            break
        alpha = rho / sigma
        inner(x)[...] += alpha * inner(p)
        inner(r)[...] -= alpha * inner(w)
        rr = dot(r, r)
        last = k + 1 == max_iter
        rz = rho
        if mnorm or not last:
            z = M(r)
            rz = dot(r, z)
        it = k + 1
        hist.append(np.sqrt(rr) / r0)
        if stopped(rr, rz):
            break
        beta = rz / rho if rho != 0 else 0.0
        rho = rz
    return it, np.array(hist)


def high_contrast7(nx, ny, nz, contrast=1e6, block=4, frac=0.3, seed=2024):
    """7-point diffusion with two-phase coefficients: blocks of block^3 points take kappa = contrast with probability
    `frac` (splitmix64 hash of the block index), 1 elsewhere; face coefficients are harmonic means; Dirichlet
    boundaries (the couplings to the ghost layer count in the diagonal and are not stored)"""
    g = (nz + 2, ny + 2, nx + 2)
    kk, jj, ii = np.meshgrid(*[np.arange(n) // block for n in g], indexing="ij")
    bid = (kk * 4096 + jj) * 4096 + ii
    kap = np.where(pb.splitmix64(bid.ravel(), seed).reshape(g) < frac, contrast, 1.0)
    # the ghost layer takes the coefficient of the point next to it
    kap[0], kap[-1] = kap[1], kap[-2]
    kap[:, 0], kap[:, -1] = kap[:, 1], kap[:, -2]
    kap[:, :, 0], kap[:, :, -1] = kap[:, :, 1], kap[:, :, -2]

    def hm(a, b):
        return 2.0 * a * b / (a + b)

    fx = hm(kap[:, :, 1:], kap[:, :, :-1])   # face between i-1 and i, stored at i (shape ..., II-1)
    fy = hm(kap[:, 1:, :], kap[:, :-1, :])
    fz = hm(kap[1:], kap[:-1])
    so = np.zeros((4,) + g)
    I, J, K = slice(1, nx + 1), slice(1, ny + 1), slice(1, nz + 1)
    so[pb.KP, K, J, I] = (fx[K, J, 0:nx] + fx[K, J, 1:nx + 1] + fy[K, 0:ny, I] + fy[K, 1:ny + 1, I]
                          + fz[0:nz, J, I] + fz[1:nz + 1, J, I])
    so[pb.KPW, K, J, 2:nx + 1] = fx[K, J, 1:nx]
    so[pb.KPS, K, 2:ny + 1, I] = fy[K, 1:ny, I]
    so[pb.KB, 2:nz + 1, J, I] = fz[1:nz, J, I]
    return so


def random_field(shape_g, seed):
    x = pb.uniform(shape_g, seed, -1.0, 1.0)
    return x * pb.interior_mask(shape_g)
