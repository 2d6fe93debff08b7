"""The interpolation weights of the cycle's grid transfers kept in single precision
(cedar_amd_solver_use_fp32_interpolation, the float instantiations of transferf.hip), single vector
and batch, 2D and 3D.

Promoting a float to double is exact, so a transfer kernel that reads a float copy of the weights and promotes on use does
the FP64 kernel's arithmetic on the weights rounded to float: sections 1 and 2 compare bit patterns, no tolerance.
Section 3 runs the real (unrounded) weights against an untouched FP64 handle: the weights enter the cycle through the
coarse-grid correction only, so counts are equal, histories agree to a relative 1e-4 (tests/test_ci32_statement.py has
the CPU statement and the measured 4.6e-6) and `solve` reaches the same solution to 1e-12 of max|x|.
"""
import functools

import numpy as np
import pytest

import pcg_statement as ps
import problems as pb

pytestmark = pytest.mark.gpu

SENTINEL = -1.2345678e300


def rt(a):
    return a.astype(np.float32).astype(np.float64)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def capi():
    from cedar_amd import capi
    assert capi.device_count() >= 1, "no GPU visible"
    return capi


@pytest.fixture(scope="module")
def K(capi):
    return capi.Kernels()


@pytest.fixture(scope="module")
def O():
    from pyoracle import Oracle
    return Oracle()


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for v in ("CEDAR_AMD_CI32_MIN_ROWS", "CEDAR_AMD_OP32_MIN_ROWS", "CEDAR_AMD_LINES_SMALL", "CEDAR_AMD_PSUM"):
        monkeypatch.delenv(v, raising=False)


# ---------------------------------------------------------------- 1. kernels, bit for bit
# Fine (nx, ny, nz); the coarse grid has nxc = (nx - 1) // 2 + 1 points a row.
# Float restrictions: a lane owns the coarse pair (ic, ic + 1), ic odd, so a row is ceil(nxc / 2) pairs; workgroups of 64
# lanes up to 64 pairs, else 128 (3D) or 128 / 256 (2D), one grid column of workgroups per 128 (256) pairs.
# interp_add3: one workgroup a fine row, a lane owns a fine pair, 64 / 128 / 256 lanes at IIF / 2 = (nx + 2) // 2 of
# <= 64, < 256, >= 256, lane loop beyond.  interp_add2 (float): 256 lanes, one per fine point i = 2 .. IIF.
#   (3,3,3) (4,5,3) (5,4,6) (9,3,3) (10,3,3)   odd and even extents -- the ghost column, row and plane that even extents
#                                              touch -- and coarse rows of 2, 2, 3, 5, 5 points: a lone pair, a pair and a
#                                              single, two pairs and a single
#   (127..130,3,3)                             interp_add3's 64 -> 128-lane step (IIF/2 = 64, 65, 65, 66); 32 | 33 pairs
#   (255..258,3,3)                             restrictions: 64 pairs | 65 pairs, the 64 -> 128-lane step
#   (511..514,3,3)                             interp_add3's 128 -> 256-lane step (IIF/2 = 256, 257, 257, 258); restrict3:
#                                              128 pairs | 129 pairs, the second workgroup of a row
#   (513,4,3) (1030,3,3)                       second and third trips of interp_add3's lane loop; 258 pairs: three workgroups
#   (40,33,50)                                 many rows
SHAPES3 = [(3, 3, 3), (4, 5, 3), (5, 4, 6), (9, 3, 3), (10, 3, 3), (127, 3, 3), (128, 3, 3), (129, 3, 3), (130, 3, 3),
           (255, 3, 3), (256, 3, 3), (257, 3, 3), (258, 3, 3), (511, 3, 3), (512, 3, 3), (513, 3, 3), (514, 3, 3),
           (513, 4, 3), (1030, 3, 3), (40, 33, 50)]
#   (3,3) (4,5) (9,3) (10,3)                   as in 3D
#   (255..258,3)                               restrict2: 64 | 65 pairs (64 -> 128 lanes); interp_add2: IIF - 1 = 256 | 257
#                                              points, the second workgroup of a row
#   (511..514,3)                               restrict2: 128 | 129 pairs (128 -> 256 lanes); interp_add2: 512 | 513 points
#   (1023,3) (1024,3) (1025,3) (1030,3)        restrict2: 256 | 257 pairs, the second workgroup of a row
#   (200,130)                                  many rows
SHAPES2 = [(3, 3), (4, 5), (9, 3), (10, 3), (255, 3), (256, 3), (257, 3), (258, 3), (511, 3), (512, 3), (513, 3), (514, 3),
           (1023, 3), (1024, 3), (1025, 3), (1030, 3), (200, 130)]
MANY_SHAPES3 = [(4, 5, 3), (10, 3, 3), (257, 3, 3), (513, 4, 3), (40, 33, 50)]
NRHS = [1, 3, 9]


@functools.lru_cache(maxsize=None)
def kernel_problem(shape, nst):
    """weights uniform in [-1, 1] (ghost cells included) and their rounding, an operator whose diagonal interp_add
    divides by, and max(NRHS) + 1 fine and coarse vectors with non-zero ghost cells"""
    g = tuple(n + 2 for n in shape[::-1])
    gc = pb.coarse_shape(g)
    nd = len(shape)
    seed = 4100 + 7 * sum(shape) + nst
    ci = pb.uniform((26 if nd == 3 else 8,) + gc, seed, -1, 1)
    so = pb.random_op(g, nst, seed + 1, zero_ghost=False)
    nitems = max(NRHS) + 1
    q = np.stack([pb.uniform(g, seed + 2 + 10 * m, -1, 1) for m in range(nitems)])
    res = np.stack([pb.uniform(g, seed + 3 + 10 * m, -1, 1) for m in range(nitems)])
    qc = np.stack([pb.uniform(gc, seed + 4 + 10 * m, -1, 1) for m in range(nitems)])
    ci_r = rt(ci)
    assert not np.array_equal(ci_r, ci)
    for a in (ci, ci_r, so, q, res, qc):
        a.setflags(write=False)
    return ci, ci_r, so, q, res, qc


@pytest.mark.parametrize("shape", SHAPES3, ids=str)
def test_restrict3_is_the_fp64_kernel_on_the_rounded_weights(K, shape):
    """cedar_amd_restrict3_ci32 on ci against BMG3_SymStd_restrict on rt(ci): every element of the coarse vector, == on the
    bit patterns; what the FP64 kernel leaves untouched (the ghost layer) keeps its sentinel"""
    ci, ci_r, _, q, _, qc = kernel_problem(shape, 14)
    want, got = np.full_like(qc[0], SENTINEL), np.full_like(qc[0], SENTINEL)
    K.restrict3(q[0].copy(), want, ci_r)
    assert K.restrict3_ci32(q[0].copy(), got, ci) == 0
    assert same_bits(got, want), (shape, np.max(np.abs(got - want)))
    m = pb.interior_mask(got.shape)
    assert np.all(got[~m] == SENTINEL) and not np.any(got[m] == SENTINEL)


@pytest.mark.parametrize("nst", [14, 4])
@pytest.mark.parametrize("shape", SHAPES3, ids=str)
def test_interp_add3_is_the_fp64_kernel_on_the_rounded_weights(K, shape, nst):
    """cedar_amd_interp_add3_ci32 against BMG3_SymStd_interp_add on rt(ci): x and the scaled residual, every element"""
    ci, ci_r, so, q, res, qc = kernel_problem(shape, nst)
    qw, rw, qg, rg = q[0].copy(), res[0].copy(), q[0].copy(), res[0].copy()
    K.interp_add3(qw, qc[0].copy(), so, rw, ci_r)
    assert K.interp_add3_ci32(qg, qc[0].copy(), so, rg, ci) == 0
    assert same_bits(qg, qw) and same_bits(rg, rw), (shape, nst)
    assert not np.array_equal(qg, q[0])
    if min(shape) >= 3:
        un = q[0].copy()  # the unrounded weights give other bits: the comparison can fail
        K.interp_add3(un, qc[0].copy(), so, res[0].copy(), ci)
        assert not same_bits(un, qw)


@pytest.mark.parametrize("shape", SHAPES2, ids=str)
def test_restrict2_is_the_fp64_kernel_on_the_rounded_weights(K, shape):
    ci, ci_r, _, q, _, qc = kernel_problem(shape, 5)
    want, got = np.full_like(qc[0], SENTINEL), np.full_like(qc[0], SENTINEL)
    K.restrict2(q[0].copy(), want, ci_r)
    assert K.restrict2_ci32(q[0].copy(), got, ci) == 0
    assert same_bits(got, want), (shape, np.max(np.abs(got - want)))
    m = pb.interior_mask(got.shape)
    assert np.all(got[~m] == SENTINEL) and not np.any(got[m] == SENTINEL)


@pytest.mark.parametrize("nst", [5, 3])
@pytest.mark.parametrize("shape", SHAPES2, ids=str)
def test_interp_add2_is_the_fp64_kernel_on_the_rounded_weights(K, shape, nst):
    ci, ci_r, so, q, res, qc = kernel_problem(shape, nst)
    qw, rw, qg, rg = q[0].copy(), res[0].copy(), q[0].copy(), res[0].copy()
    K.interp_add2(qw, qc[0].copy(), rw, so, ci_r)
    assert K.interp_add2_ci32(qg, qc[0].copy(), rg, so, ci) == 0
    assert same_bits(qg, qw) and same_bits(rg, rw), (shape, nst)
    assert not np.array_equal(qg, q[0])


@pytest.mark.parametrize("nrhs", NRHS)
@pytest.mark.parametrize("shape", MANY_SHAPES3, ids=str)
def test_many_items_are_the_single_call(K, shape, nrhs):
    """cedar_amd_restrict3_many_ci32 / _interp_add3_many_ci32: item m has the bits of the single call on item m alone (and
    so of the FP64 kernel on the rounded weights); the item beyond nrhs keeps its bits"""
    ci, ci_r, so, q, res, qc = kernel_problem(shape, 14)
    q, res, qc = (np.ascontiguousarray(a[:nrhs + 1]) for a in (q, res, qc))
    got = np.full_like(qc, SENTINEL)
    assert K.restrict3_many_ci32(q.copy(), got, ci, nrhs=nrhs) == 0
    for m in range(nrhs):
        one = np.full_like(qc[m], SENTINEL)
        assert K.restrict3_ci32(q[m].copy(), one, ci) == 0
        assert same_bits(got[m], one), (shape, nrhs, m)
    want = np.full_like(qc[0], SENTINEL)
    K.restrict3(q[nrhs - 1].copy(), want, ci_r)
    assert same_bits(got[nrhs - 1], want) and np.all(got[nrhs] == SENTINEL)

    qg, rg = q.copy(), res.copy()
    assert K.interp_add3_many_ci32(qg, qc.copy(), so, rg, ci, nrhs=nrhs) == 0
    for m in range(nrhs):
        q1, r1 = q[m].copy(), res[m].copy()
        assert K.interp_add3_ci32(q1, qc[m].copy(), so, r1, ci) == 0
        assert same_bits(qg[m], q1) and same_bits(rg[m], r1), (shape, nrhs, m)
    assert same_bits(qg[nrhs], q[nrhs]) and same_bits(rg[nrhs], res[nrhs]) and not np.array_equal(qg[:nrhs], q[:nrhs])


def test_kernel_entry_points_refuse_a_weight_that_overflows(K, capfd):
    """a weight of 1e39: non-zero, a message naming the call, outputs untouched; the same call on the weights given is served"""
    ci3, _, so3, q3, res3, qc3 = kernel_problem((9, 3, 3), 14)
    ci2, _, so2, q2, res2, qc2 = kernel_problem((9, 3), 5)
    big3, big2 = ci3.copy(), ci2.copy()
    big3[7, 1, 2, 2] = 1e39
    big2[3, 2, 2] = -1e39
    many = lambda a: np.ascontiguousarray(a[:3])
    calls = [
        ("cedar_amd_restrict2_ci32", big2, ci2, lambda w, o: K.restrict2_ci32(q2[0].copy(), o[0], w), [qc2[0]]),
        ("cedar_amd_interp_add2_ci32", big2, ci2, lambda w, o: K.interp_add2_ci32(o[0], qc2[0].copy(), o[1], so2, w), [q2[0], res2[0]]),
        ("cedar_amd_restrict3_many_ci32", big3, ci3, lambda w, o: K.restrict3_ci32(q3[0].copy(), o[0], w), [qc3[0]]),
        ("cedar_amd_interp_add3_many_ci32", big3, ci3, lambda w, o: K.interp_add3_ci32(o[0], qc3[0].copy(), so3, o[1], w), [q3[0], res3[0]]),
        ("cedar_amd_restrict3_many_ci32", big3, ci3, lambda w, o: K.restrict3_many_ci32(many(q3).copy(), o[0], w), [many(qc3)]),
        ("cedar_amd_interp_add3_many_ci32", big3, ci3,
         lambda w, o: K.interp_add3_many_ci32(o[0], many(qc3).copy(), so3, o[1], w), [many(q3), many(res3)]),
    ]
    for name, big, ci, call, init in calls:
        out = [a.copy() for a in init]
        capfd.readouterr()
        assert call(big, out) != 0, name
        err = capfd.readouterr().err
        assert name in err and "overflows single precision" in err, (name, err)
        assert all(same_bits(o, a) for o, a in zip(out, init)), name
        assert call(ci, out) == 0 and not all(np.array_equal(o, a) for o, a in zip(out, init)), name


# ---------------------------------------------------------------- 2. handles, still bit for bit
V11 = dict(nrelax_pre=1, nrelax_post=1)
V21 = dict(nrelax_pre=2, nrelax_post=1)
TOL = 1e-10
# name -> (operator, Solver arguments).  varcoef9(129,97): levels 129x97 and 65x49 run the transfer kernels, 33x25 and
# below the LDS-resident small-level kernels with their fused transfers; poisson2(200,130): 200x130 and 100x65 (100 > 64)
CASES = {
    "fe3": (lambda: pb.fe3(33, 33, 33), {}),
    "dd3": (lambda: pb.diag_diffusion3(40, 33, 50, 1.0, 0.8, 1.3), {}),  # a 7-point level 0 over 27-point levels
    "vc9-point": (lambda: pb.varcoef9(129, 97), {}),
    "vc9-xy": (lambda: pb.varcoef9(129, 97), dict(relax="line-xy")),
    "p2-x": (lambda: pb.poisson2(200, 130), dict(relax="line-x")),
    "vc9-f": (lambda: pb.varcoef9(129, 97), dict(cycle="f")),
    "fe3-f": (lambda: pb.fe3(33, 33, 33), dict(cycle="f")),
    "hc7": (lambda: ps.high_contrast7(24, 24, 24), {}),
    "poisson3": (lambda: pb.poisson3(40, 33, 50), {}),
    "an9-xy": (lambda: pb.aniso9(129, 97), dict(relax="line-xy")),
    "poisson2": (lambda: pb.poisson2(200, 130), {}),
}
NITEMS = 3


@functools.lru_cache(maxsize=None)
def solver_problem(name):
    """operator, Solver arguments, NITEMS right-hand sides (splitmix seeds 17, ...), NITEMS random interior vectors"""
    mk, kw = CASES[name]
    so = mk()
    g = so.shape[1:]
    m = pb.interior_mask(g)
    b = np.stack([pb.uniform(g, 17 + 100 * t, -1, 1) * m for t in range(NITEMS)])
    r = np.stack([pb.uniform(g, 23 + 100 * t, -1, 1) * m for t in range(NITEMS)])
    for a in (so, b, r):
        a.setflags(write=False)
    return so, kw, b, r


def is_small(s, l):
    return s.nd == 2 and max(s.dims(l)[:2]) <= 64  # the LDS-resident small-level kernels serve it: its transfers are fused


def pairs_served(s):
    return sum(1 for l in range(s.nlevels() - 1) if not is_small(s, l))


def mirror(A, B):
    """round B's weights on exactly the levels whose float copy A's transfers read: the coarse levels 1 .. n of the n
    pairs A counts (pairs are taken from the finest down: the fine levels the small-level kernels serve are the coarsest)"""
    n = A.fp32_interp_levels()
    for l in range(1, n + 1):
        B.set_array(l, "P", rt(B.array(l, "P")))
    return n


class Pair:
    """two handles on one operator; before(A, B) runs on both ahead of the switch, after(A, B) behind it"""

    def __init__(self, capi, name, cyc, before=None, after=None, **more):
        so, kw, self.b, self.r = solver_problem(name)
        kw = dict(kw, max_iter=30, tol=TOL, **cyc, **more)
        self.A, self.B = capi.Solver(so, **kw), capi.Solver(so, **kw)
        if before:
            before(self.A), before(self.B)
        self.n = self.A.use_fp32_interpolation(1)
        if after:
            after(self.A), after(self.B)
            self.n = self.A.use_fp32_interpolation(1)  # pairs whose fine level `after` moved off the small-level path
        assert self.n == self.A.fp32_interp_levels() and self.B.fp32_interp_levels() == 0
        assert mirror(self.A, self.B) == self.n

    def close(self):
        self.A.close(), self.B.close()

    def both(self, f):
        a, b = f(self.A), f(self.B)
        for u, v in zip(a, b):
            assert same_bits(np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64))
        return a

    def vcycles(self):
        def run(s):
            x = self.r[0].copy()
            s.vcycle(x, self.b[0])
            s.vcycle(x, self.b[0])
            return (x,)
        (x,) = self.both(run)
        assert not np.array_equal(x, self.r[0])
        return x

    def solve(self, converges=True):
        """converges=False: an F-cycle handle's solve starts every cycle from x = 0, and V(1,1) may need more than the 30
        cycles allowed; the bits are compared all the same"""
        def run(s):
            x = np.zeros_like(self.b[0])
            h = s.solve(self.b[0], x)
            return x, h
        x, h = self.both(run)
        assert len(h) > 2 and np.all(np.isfinite(h)) and (h[-1] < TOL or not converges)

    def cg(self, which):
        def run(s):
            x = np.zeros_like(self.b[0])
            h = getattr(s, which)(self.b[0], x, max_iter=40, tol=TOL)
            return x, h
        x, h = self.both(run)
        assert len(h) > 2 and h[-1] < TOL


def check_pair(capi, name, fcycle=False, before=None, after=None):
    p = Pair(capi, name, V11, before, after)
    try:
        assert p.n == pairs_served(p.A) >= 1
        p.vcycles()
        p.cg("fcg" if fcycle else "pcg")
    finally:
        p.close()
    p = Pair(capi, name, V21, before, after)
    try:
        p.vcycles()
        p.solve(converges=not fcycle)
        p.cg("fcg")
    finally:
        p.close()


@pytest.mark.parametrize("name", ["fe3", "dd3", "vc9-point", "vc9-xy", "p2-x"])
def test_switched_handle_is_the_fp64_handle_on_the_rounded_weights(capi, name):
    """two V-cycles from a random x, solve V(2,1), pcg V(1,1), fcg V(2,1): x, history and counts agree in every bit"""
    check_pair(capi, name)


@pytest.mark.parametrize("name", ["vc9-f", "fe3-f"])
def test_f_cycle_handles(capi, name):
    check_pair(capi, name, fcycle=True)


@pytest.mark.parametrize("order", ["operator-first", "interpolation-first"])
@pytest.mark.parametrize("name,switch", [("fe3", "use_fp32_operator_all"), ("dd3", "use_fp32_operator_all"),
                                         ("vc9-point", "use_fp32_operator_2d"), ("vc9-xy", "use_fp32_operator_lines")])
def test_composes_with_the_operator_switches(capi, name, switch, order):
    """the operator switch on both handles, before or after A's use_fp32_interpolation: each keeps its own count.  A 2D
    level that takes an operator copy leaves the small-level path, so its pair runs the transfer kernels: switched when the
    operator call came first (or on a repeated call), FP64 otherwise"""
    def op(s):
        assert getattr(s, switch)(1) == s.fp32_levels() >= 1
    kw = dict(before=op) if order == "operator-first" else dict(after=op)
    p = Pair(capi, name, V11, **kw)
    try:
        nl = p.A.nlevels() - 1
        assert p.n == (nl if switch != "use_fp32_operator_lines" else pairs_served(p.A))
        assert p.A.fp32_levels() == p.B.fp32_levels() >= 1
        p.vcycles()
        p.cg("pcg")
        p.solve(converges=False)
    finally:
        p.close()


@pytest.mark.parametrize("name", ["fe3", "vc9-point", "vc9-xy"])
def test_batch_handles(capi, name):
    """create_many handles with three right-hand sides: vcycle_many, solve_many, pcg_many"""
    p = Pair(capi, name, V11, max_rhs=NITEMS)
    try:
        assert p.n == pairs_served(p.A) >= 1

        def vc(s):
            x = p.r.copy()
            s.vcycle_many(x, p.b)
            s.vcycle_many(x, p.b)
            return (x,)

        def solve(s):
            x = np.zeros_like(p.b)
            rel, iters = s.solve_many(p.b, x)
            return [x, np.array(iters, dtype=np.float64)] + list(rel)

        def pcg(s):
            x = np.zeros_like(p.b)
            hist, iters = s.pcg_many(p.b, x, max_iter=40, tol=TOL)
            return [x, np.array(iters, dtype=np.float64)] + list(hist)

        (x,) = p.both(vc)
        assert not np.array_equal(x, p.r)
        out = p.both(solve)
        assert all(len(h) > 2 and h[-1] < 1e-6 for h in out[2:])
        out = p.both(pcg)
        assert all(h[-1] < TOL for h in out[2:])
        # item 0 of the batch against the single-vector cycle of the same handle
        x1 = p.r[0].copy()
        p.A.vcycle(x1, p.b[0])
        p.A.vcycle(x1, p.b[0])
        assert same_bits(x1, x[0])
    finally:
        p.close()


@pytest.mark.parametrize("name", ["fe3", "vc9-point", "vc9-xy"])
def test_counts_defaults_set_and_get(capi, name, monkeypatch, capfd):
    so, kw, b, r = solver_problem(name)
    kw = dict(kw, **V11)
    A, B = capi.Solver(so, **kw), capi.Solver(so, **kw)
    try:
        want = pairs_served(A)
        assert A.fp32_interp_levels() == 0
        assert A.use_fp32_interpolation() == 0  # the default: no level here has 128 (3D) / 1024 (2D) rows
        x0 = r[0].copy()
        B.vcycle(x0, b[0])
        xa = r[0].copy()
        A.vcycle(xa, b[0])
        assert same_bits(xa, x0)  # nothing reads a float copy until a pair is switched
        rows = A.dims(0)[1]
        assert A.use_fp32_interpolation(rows) == 1 and A.use_fp32_interpolation(rows + 1) == 1  # never switched back
        monkeypatch.setenv("CEDAR_AMD_CI32_MIN_ROWS", "1")
        assert A.use_fp32_interpolation() == want  # the override is read at the call
        monkeypatch.delenv("CEDAR_AMD_CI32_MIN_ROWS")
        assert A.use_fp32_interpolation(1) == want == A.fp32_interp_levels() and A.fp32_levels() == 0
        # get "P" returns the unrounded weights
        for l in range(1, want + 1):
            P = A.array(l, "P")
            assert same_bits(P, B.array(l, "P")) and not np.array_equal(rt(P), P)
        assert mirror(A, B) == want
        xa, xb = r[0].copy(), r[0].copy()
        A.vcycle(xa, b[0]), B.vcycle(xb, b[0])
        assert same_bits(xa, xb) and not same_bits(xa, x0)
        # set "P" with new weights rebuilds the copy
        P = A.array(1, "P")
        newP = P * (1.0 + 1e-3 * pb.uniform(P.shape, 77, -1, 1))
        A.set_array(1, "P", newP)
        B.set_array(1, "P", rt(newP))
        assert same_bits(A.array(1, "P"), newP)
        ya, yb = r[0].copy(), r[0].copy()
        A.vcycle(ya, b[0]), B.vcycle(yb, b[0])
        assert same_bits(ya, yb) and not same_bits(ya, xa)
        # a weight that overflows float: reported, the level's transfers read the FP64 weights again
        big = newP.copy()
        big.reshape(-1)[big.size // 2] = 1e39
        capfd.readouterr()
        A.set_array(1, "P", big)
        assert "overflows single precision" in capfd.readouterr().err
        assert A.fp32_interp_levels() == want - 1
        B.set_array(1, "P", big)
        za, zb = r[0].copy(), r[0].copy()
        A.vcycle(za, b[0]), B.vcycle(zb, b[0])
        assert same_bits(za, zb)
    finally:
        A.close(), B.close()


def test_refusals_leave_the_handle_unchanged(capi, capfd):
    """NULL handle, ibc != 0, 3D plane relaxation, negative min_rows, a weight finite in FP64 and not in float: -1, a
    message naming the call, no pair switched, the bits of vcycle's result unchanged"""
    who = "cedar_amd_solver_use_fp32_interpolation"
    capfd.readouterr()
    assert capi.lib.cedar_amd_solver_use_fp32_interpolation(None, 1) == -1
    assert who in capfd.readouterr().err
    assert capi.lib.cedar_amd_solver_fp32_interp_levels(None) == 0
    capfd.readouterr()

    def refused(s, b, x0, min_rows, word):
        xa = x0.copy()
        s.vcycle(xa, b)
        capfd.readouterr()
        assert s.use_fp32_interpolation(min_rows) == -1
        err = capfd.readouterr().err
        assert who in err and word in err and "unchanged" in err, err
        assert s.fp32_interp_levels() == 0
        xb = x0.copy()
        s.vcycle(xb, b)
        assert same_bits(xa, xb)

    so, _, b, r = solver_problem("fe3")
    s = capi.Solver(so, **V11)
    try:
        refused(s, b[0], r[0], -1, "negative")
        big = s.array(2, "P")
        big[3, 2, 2, 2] = 1e39
        s.set_array(2, "P", big)
        refused(s, b[0], r[0], 1, "overflows single precision")
    finally:
        s.close()
    so9 = pb.fe3(9, 9, 9)
    g = so9.shape[1:]
    s = capi.Solver(so9, relax="plane-xy", **V11)
    try:
        refused(s, pb.uniform(g, 17, -1, 1) * pb.interior_mask(g), pb.uniform(g, 23, -1, 1) * pb.interior_mask(g), 1, "plane")
    finally:
        s.close()
    per = (True, False)
    sop = pb.periodic_poisson2(16, 16, per)
    g = sop.shape[1:]
    s = capi.Solver(sop, ibc=pb.ibc_of(per), **V11)
    try:
        refused(s, pb.periodic_rhs2(16, 16, per), np.zeros(g), 1, "ibc")
    finally:
        s.close()


# ---------------------------------------------------------------- 3. real weights
HIST_RTOL = 1e-4


def true_rel_residual(O, so, b, x):
    r = pb.interior_mask(b.shape) * (b - ps.apply_A(O, so, x))
    return np.linalg.norm(r) / np.linalg.norm(b)


def close_hist(h1, h0):
    return len(h1) == len(h0) and np.all(np.abs(h1 - h0) <= HIST_RTOL * np.abs(h0))


@pytest.mark.parametrize("name", ["fe3", "poisson3", "dd3", "vc9-point", "vc9-xy", "an9-xy", "poisson2"])
def test_solve_on_the_real_weights(capi, O, name):
    """`solve` V(2,1) to 1e-10 against an untouched FP64 handle: equal cycle counts, histories within 1e-4, x within 1e-12 of
    max|x| (measured on the CPU statement: 1.5e-14), the true relative residual below the tolerance for both"""
    so, kw, b, _ = solver_problem(name)
    kw = dict(kw, max_iter=40, tol=TOL, **V21)
    out = []
    for switched in (False, True):
        s = capi.Solver(so, **kw)
        try:
            if switched:
                assert s.use_fp32_interpolation(1) == pairs_served(s) >= 1
            x = np.zeros_like(b[0])
            h = s.solve(b[0], x)
        finally:
            s.close()
        out.append((h, x))
    (h0, x0), (h1, x1) = out
    dev = np.max(np.abs(h1 - h0) / np.abs(h0)) if len(h0) == len(h1) else None
    print(name, "cycles", len(h0) - 1, len(h1) - 1, "history deviation", dev, "x", np.max(np.abs(x1 - x0)) / np.max(np.abs(x0)),
          "true residuals", true_rel_residual(O, so, b[0], x0), true_rel_residual(O, so, b[0], x1))
    assert len(h0) == len(h1) and h0[-1] < TOL and h1[-1] < TOL
    assert close_hist(h1, h0)
    assert np.max(np.abs(x1 - x0)) <= 1e-12 * np.max(np.abs(x0))
    assert true_rel_residual(O, so, b[0], x0) < TOL and true_rel_residual(O, so, b[0], x1) < TOL


@pytest.mark.parametrize("name", ["fe3", "dd3", "vc9-point", "vc9-xy", "an9-xy", "hc7"])
def test_pcg_on_the_real_weights(capi, O, name):
    """pcg V(1,1) to 1e-10 against an untouched FP64 handle: equal iteration counts, histories within 1e-4 (high_contrast7:
    counts and the final residual only), the true relative residual below the tolerance for both"""
    so, kw, b, _ = solver_problem(name)
    kw = dict(kw, **V11)
    out = []
    for switched in (False, True):
        s = capi.Solver(so, **kw)
        try:
            if switched:
                assert s.use_fp32_interpolation(1) == pairs_served(s) >= 1
            x = np.zeros_like(b[0])
            h = s.pcg(b[0], x, max_iter=60, tol=TOL)
        finally:
            s.close()
        out.append((h, x))
    (h0, x0), (h1, x1) = out
    dev = np.max(np.abs(h1 - h0) / np.abs(h0)) if len(h0) == len(h1) else None
    print(name, "iterations", len(h0) - 1, len(h1) - 1, "history deviation", dev,
          "true residuals", true_rel_residual(O, so, b[0], x0), true_rel_residual(O, so, b[0], x1))
    assert len(h0) == len(h1) and h0[-1] < TOL and h1[-1] < TOL
    if name != "hc7":
        assert close_hist(h1, h0)
    assert true_rel_residual(O, so, b[0], x0) < TOL and true_rel_residual(O, so, b[0], x1) < TOL
