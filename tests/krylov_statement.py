"""Plain statement of the passes of one conjugate-gradient iteration (cedar_amd/csrc/krylov.hip), numpy only.

For given arrays and a scalar block each function returns what the pass must leave, in the rounding order the kernels'
header states (the library is built without FMA contraction, numpy does not fuse either):

  direction   p' = z + beta p (first: p' = z) on the whole array, ghost cells included; w = A p' on the interior through
              the oracle's matvec2 / matvec3; pn and w outside the interior as given
  update      x + alpha p, r - alpha w (alpha = 0: x and r as they are), z = r / diag
  the dots    exactly: on dyadic (small-integer) data as an integer sum, on real data as the correctly rounded sum of
              the exact products (error-free product splitting + math.fsum)
  the scalars set_alpha / set_rho of krylov.hip: alpha, beta, the rho hand-over, the breakdown flag, `first`, the three
              has_rz cases; rank-order combine as a left-to-right float sum (the same sequence of IEEE additions)

pcg_chained strings them together in the order of cedar_amd_solver_pcg (solver.cpp); tests/test_krylov_statement.py pins
it to tests/pcg_statement.py without a GPU.
"""
import math
import sys

import numpy as np

import pcg_statement as ps

RHO, SIGMA, ALPHA, BETA, RR, RZ, FLAG, NSC = 0, 1, 2, 3, 4, 5, 6, 8  # common.h PCG_*
DBL_MAX = sys.float_info.max
U = 2.0 ** -53  # unit roundoff of binary64

inner = ps.inner


# ---------------------------------------------------------------- arrays
def direction(oracle, so, z, p, pn, w, beta, first):
    """(pn', w'): p may be anything (NaN) when first"""
    pf = z.copy() if first else z + beta * p
    full = np.zeros_like(z)
    (oracle.matvec2 if so.ndim == 3 else oracle.matvec3)(np.ascontiguousarray(so), pf, full)
    pn2, w2 = pn.copy(), w.copy()
    inner(pn2)[...] = inner(pf)
    inner(w2)[...] = inner(full)
    return pn2, w2


def update(zmode, move, x, r, p, w, z, diag, alpha):
    """(x', r', z'); arrays a mode does not use may be None and come back as given"""
    x2 = None if x is None else x.copy()
    r2 = r.copy()
    z2 = None if z is None else z.copy()
    if move and alpha != 0.0:
        inner(x2)[...] = inner(x) + alpha * inner(p)
        inner(r2)[...] = inner(r) - alpha * inner(w)
    if zmode == 1:
        inner(z2)[...] = inner(r2) / inner(diag)
    return x2, r2, z2


def shell(z, p, pn, beta, first, boxes):
    """pn' = z + beta p on boxes (i0, j0, k0, ni, nj, nk), 0-based incl. ghost; 3D arrays"""
    pf = z.copy() if first else z + beta * p
    out = pn.copy()
    for i0, j0, k0, ni, nj, nk in boxes:
        s = (slice(k0, k0 + nk), slice(j0, j0 + nj), slice(i0, i0 + ni))
        out[s] = pf[s]
    return out


# ---------------------------------------------------------------- exact dots
def _scaled_ints(a, max_shift):
    for k in range(max_shift + 1):
        s = a * float(2 ** k)
        if np.array_equal(s, np.rint(s)):
            assert np.max(np.abs(s)) < 2 ** 20, "not small-integer data"
            return s.astype(np.int64), k
    raise AssertionError("not dyadic data: no power of two up to 2^%d makes it integral" % max_shift)


def exact_dot_dyadic(u, v, max_shift=16):
    """interior dot of dyadic rationals as integers: (total, sum_abs, shift) with u.v = total / 2^shift exactly.
    sum_abs < 2^53 means: every product and every partial sum of them, in any order, is an exact double."""
    a, ka = _scaled_ints(inner(u).ravel(), max_shift)
    b, kb = _scaled_ints(inner(v).ravel(), max_shift)
    t = a * b  # below 2^40 each, at most 2^21 terms: no int64 overflow
    assert t.size <= 2 ** 21
    return int(np.sum(t)), int(np.sum(np.abs(t))), ka + kb


def dyadic_value(total, shift):
    return math.ldexp(float(total), -shift)  # exact for |total| < 2^53


def _two_prod(a, b):
    """a * b = p + e exactly (Dekker / Veltkamp splitting; no overflow or underflow for moderate data)"""
    p = a * b
    c = 134217729.0 * a
    ah = c - (c - a)
    al = a - ah
    c = 134217729.0 * b
    bh = c - (c - b)
    bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def exact_dot_real(u, v):
    """(s, sum_abs, n): s the exact interior dot rounded once, sum_abs = sum |u_i v_i| (rounded), n the number of terms"""
    a, b = inner(u).ravel(), inner(v).ravel()
    p, e = _two_prod(a, b)
    return math.fsum(np.concatenate([p, e]).tolist()), math.fsum(np.abs(p).tolist()), a.size


def any_order_bound(n, sum_abs):
    """|fl-sum of n rounded products in ANY association - exact| <= gamma_n sum|t_i|: each term passes one product
    rounding and at most n - 1 additions, n U sum|t| to first order.  The factor 2 covers the higher-order terms of
    gamma_n = n U / (1 - n U) (n U < 2^-31 here) and the rounding of sum_abs itself -- a margin on the analysis, not a
    fitted tolerance."""
    return 2.0 * n * U * sum_abs


# ---------------------------------------------------------------- scalars
def set_alpha(sigma, sc):
    sc = np.array(sc, dtype=np.float64)
    rho = float(sc[RHO])
    ok = sigma > 0.0 and sigma <= DBL_MAX and rho != 0.0
    sc[SIGMA] = sigma
    sc[ALPHA] = rho / sigma if ok else 0.0
    if not ok:
        sc[FLAG] = 1.0
    return sc


def has_rz_of(zmode):
    return 0 if zmode == 3 else 2 if zmode == 0 else 1


def set_rho(rr, rz, has_rz, first, sc):
    sc = np.array(sc, dtype=np.float64)
    sc[RR] = rr
    if has_rz:
        rho = float(sc[RHO])
        sc[RZ] = rz
        sc[BETA] = 0.0 if first or rho == 0.0 else rz / rho
        sc[RHO] = rz
    return sc


def update_scalars(zmode, rr, rz, first, sc):
    """the second stage of pcg_update: zmode 0 takes r.z = r.r, zmode 3 stores r.r only"""
    h = has_rz_of(zmode)
    return set_rho(rr, rr if h == 2 else rz, h, first, sc)


def rank_sum(g, world, stride, t):
    v = float(g[t])
    for r in range(1, world):
        v += float(g[r * stride + t])
    return v


def rank_alpha(g, world, stride, sc):
    return set_alpha(rank_sum(g, world, stride, 0), sc)


def rank_rho(zmode, g, world, stride, first, sc):
    h = has_rz_of(zmode)
    rr = rank_sum(g, world, stride, 0)
    return set_rho(rr, rank_sum(g, world, stride, 1) if h == 1 else rr, h, first, sc)


# ---------------------------------------------------------------- the passes chained as cedar_amd_solver_pcg does
def pcg_chained(oracle, so, b, x, ml=None, precon="mg", max_iter=50, tol=1e-8, stop="rel_l2", nmg=1):
    """x updated in place; returns (iterations, hist).  Dots in floating point (np.dot), as tests/pcg_statement.py."""
    zm = {"none": 0, "diag": 1, "mg": 2}[precon]
    mnorm, rel = stop in ("abs_m", "rel_m"), stop in ("rel_l2", "rel_m")
    diag = so[0]

    def M(r):
        z = np.zeros_like(r)
        for _ in range(nmg):
            ml.vcycle(z, r)
        return z

    def dots(r, z):
        return ps.dot(r, r), (ps.dot(r, z) if z is not None else 0.0)

    sc = np.zeros(NSC)
    r = np.zeros_like(b)
    inner(r)[...] = inner(b - ps.apply_A(oracle, so, x))
    z = M(r) if zm == 2 else np.zeros_like(r) if zm == 1 else None
    _, r, z = update(zm, False, None, r, None, None, z, diag, 0.0)
    sc = update_scalars(zm, *dots(r, z), True, sc)
    r0, m0 = math.sqrt(sc[RR]), math.sqrt(max(sc[RZ], 0.0))
    hist = [r0]

    def stopped(sc):
        v = math.sqrt(max(sc[RZ], 0.0)) if mnorm else math.sqrt(sc[RR])
        return (v / (m0 if mnorm else r0) if rel else v) < tol

    if r0 == 0.0 or not sc[RZ] > 0 or stopped(sc):
        return 0, np.array(hist)
    pbuf = [np.zeros_like(b), np.zeros_like(b)]
    w = np.zeros_like(b)
    it = 0
    for k in range(max_iter):
        pold, pn = pbuf[(k + 1) & 1], pbuf[k & 1]
        pn, w = direction(oracle, so, r if zm == 0 else z, pold, pn, w, float(sc[BETA]), k == 0)
        pbuf[k & 1] = pn
        sc = set_alpha(ps.dot(pn, w), sc)
        zu = 3 if zm == 2 else zm
        xn, r, z = update(zu, True, x, r, pn, w, z, diag, float(sc[ALPHA]))
        x[...] = xn
        sc = update_scalars(zu, *dots(r, z if zu == 1 else None), False, sc)
        last = k + 1 == max_iter
        if zm == 2 and mnorm:
            z = M(r)
            sc = update_scalars(2, *dots(r, z), False, sc)
        if sc[FLAG] != 0:
            break
        it = k + 1
        hist.append(math.sqrt(sc[RR]) / r0)
        if stopped(sc):
            break
        if zm == 2 and not mnorm and not last:
            z = M(r)
            sc = update_scalars(2, *dots(r, z), False, sc)
    return it, np.array(hist)
