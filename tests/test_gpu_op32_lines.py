"""The operator and the line factors of a 2D line-relaxed level kept in single precision
(cedar_amd_solver_use_fp32_operator_lines, the float instantiations of linesf.hip), single vector
and batch.

Promoting a float to double is exact, so a kernel that reads float copies and promotes on load does the FP64 kernel's
arithmetic on the operator and the factors rounded to float: sections 1 - 4 and 6 compare bit patterns, no tolerance.
Section 5 runs the real (unrounded) operator, where the switched handle's preconditioner differs from the FP64 one by a
relative 6e-8.

Measured on an MI355X (section 5, tol 1e-10; FP64 handle / handle after use_fp32_operator_lines(1); the true relative
residual is the oracle's matvec on the unrounded operator; the rounding bound of evaluating b - A x twice is 1.8e-13 for
aniso9, 2.0e-13 for poisson2, 6.3e-14, 5.9e-14 and 2.7e-13 for the three varcoef9 grids):
  aniso9(129,70, eps=0.1)
    line-x    pcg V(1,1) 12 / 12 iterations, 1.5566e-11 / 1.5566e-11;  fcg V(2,1) 9 / 9, 2.2173e-11 / 2.2173e-11;
              solve V(2,1) 11 / 11 cycles, 4.7267e-11 / 4.7268e-11
    line-y    pcg 33 / 33, 8.0958e-11 / 8.1012e-11;  fcg 27 / 27, 6.3067e-11 / 6.3067e-11;
              solve 101 / 101 cycles, 8.4267e-11 / 8.4267e-11
    line-xy   pcg 8 / 8, 6.6962e-11 / 6.6964e-11;  fcg 7 / 7, 2.6130e-11 / 2.6131e-11;  solve 10 / 10, 2.8177e-11 / 2.8179e-11
  poisson2(129,70) line-xy    pcg 7 / 7, 1.6607e-11 / 1.6607e-11;  fcg 6 / 6, 7.1872e-11 / 7.1872e-11;
                              solve 9 / 9, 2.4731e-11 / 2.4731e-11
  varcoef9(1030,40) line-x    pcg 8 / 8, 5.3776e-11 / 5.3776e-11;  fcg 8 / 8, 4.3979e-12 / 4.3979e-12;
                              solve 9 / 9, 6.3794e-11 / 6.3794e-11
  varcoef9(40,1030) line-y    pcg 8 / 8, 5.8648e-11 / 5.8648e-11;  fcg 7 / 7, 9.6161e-11 / 9.6161e-11;
                              solve 9 / 9, 5.3772e-11 / 5.3772e-11
  varcoef9(530,520) line-xy   pcg 7 / 7, 7.3249e-11 / 7.3249e-11;  fcg 7 / 7, 2.0489e-11 / 2.0489e-11;
                              solve 9 / 9, 1.7135e-11 / 1.7135e-11
(the right-hand sides are splitmix fields of seed 17 scaled to [-1, 1] on the interior, x0 = 0)
"""
import ctypes as C
import functools

import numpy as np
import pytest

import problems as pb

pytestmark = pytest.mark.gpu

DOWN, UP = 0, 1
KO, KW, KS, KSW, KNW = range(5)


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


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for v in ("CEDAR_AMD_LINE_BS", "CEDAR_AMD_LINE_PERM", "CEDAR_AMD_LINES_SMALL", "CEDAR_AMD_YLINES_TRANSPOSED",
              "CEDAR_AMD_OP32_MIN_ROWS"):
        monkeypatch.delenv(v, raising=False)


# ---------------------------------------------------------------- 1. kernels, bit for bit
# line length x lines (dir 1: the grid is lines x line length).  One workgroup per line, a lane owns 8 consecutive unknowns
# of a scan tile; 64 lanes up to 512 unknowns (factors read from the plain float image, one right-hand side per lane and
# pass), else 256 lanes on tiles of 2048 unknowns (factors from the scan-ordered float copy, right-hand sides by aligned
# quads of floats: passes of 2 x 256 quads, the grid points 1, 2 and the up to three after the last whole quad one by
# one).  A slot-row of the operator copy holds line length + 3 floats, padded to a multiple of 32.
#   (1,1), (2,3), (7,2)              degenerate sizes; one line: the second colour is empty
#   (28,5) .. (31,5)                 length + 3 = 31 .. 34: either side of the float slot-row padding
#   (511,4), (512,4), (513,4)        the 64 -> 256-lane step, where the permuted factor form and the quad path begin
#   (2047,3), (2048,3), (2049,3)     second scan tile with the carry; second right-hand-side pass (512 quads a pass)
#   (4100,2)                         third tile
#   (7400,2)                         66.7 KB of dynamic LDS: beyond the 64 KB a kernel gets without asking
#   (40,5001)                        2500 line workgroups in one colour launch
SHAPES = [(1, 1), (2, 3), (7, 2), (28, 5), (29, 5), (30, 5), (31, 5), (511, 4), (512, 4), (513, 4), (2047, 3), (2048, 3),
          (2049, 3), (4100, 2), (7400, 2), (40, 5001)]
MANY_SHAPES = [(31, 5), (513, 4), (2049, 3)]
NRHS = [1, 3, 9]


@functools.lru_cache(maxsize=None)
def kernel_problem(shape, nst, d):
    """operator, right-hand sides, starting vectors, the factors of the drop-in SETUP_lines_x / _y on the unrounded
    operator, and operator and factors rounded to float"""
    from cedar_amd import capi
    n, nlines = shape
    nx, ny = (n, nlines) if d == 0 else (nlines, n)
    g = (ny + 2, nx + 2)
    so = pb.random_op(g, nst, 871 + nst + 10 * d, zero_ghost=False)
    sor = np.zeros((2,) + g)
    capi.Kernels().setup_lines2(so, sor, "xy"[d])
    nitems = 4 if nx * ny > 100000 or shape not in MANY_SHAPES else max(NRHS) + 1  # one item beyond the largest batch
    qf = np.stack([pb.uniform(g, 872 + 17 * m, -1, 1) for m in range(nitems)])  # non-zero ghost cells
    q0 = np.stack([pb.uniform(g, 873 + 17 * m, -1, 1) for m in range(nitems)])
    so_r, sor_r = rt(so), rt(sor)
    assert not np.array_equal(so_r, so) and not np.array_equal(sor_r, sor)
    for a in (so, qf, q0, sor, so_r, sor_r):
        a.setflags(write=False)
    return so, qf, q0, sor, so_r, sor_r


@pytest.mark.parametrize("d", [0, 1], ids=["x", "y"])
@pytest.mark.parametrize("nst", [5, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_line_sweep_is_the_fp64_sweep_on_the_rounded_operator_and_factors(K, shape, nst, d):
    """cedar_amd_relax2_lines_op32 on (so, sor) against BMG2_SymStd_relax_lines_x / _y on (rt(so), rt(sor)): both
    directions, both updown, three sweeps in a row, every element of q (ghost cells included) with == on the bit patterns"""
    so, qf, q0, sor, so_r, sor_r = kernel_problem(shape, nst, d)
    for ud in (DOWN, UP):
        want, got = q0[0].copy(), q0[0].copy()
        for sweep in range(3):
            K.relax_lines2(so_r, qf[0], want, sor_r, ud, "xy"[d])
            assert K.relax2_lines_op32(so, qf[0], got, sor, d, ud) == 0
            assert same_bits(got, want), (shape, nst, d, ud, sweep, np.max(np.abs(got - want)))
        assert not np.array_equal(got, q0[0])


# ---------------------------------------------------------------- 2. batches
@pytest.mark.parametrize("nrhs", NRHS)
@pytest.mark.parametrize("d", [0, 1], ids=["x", "y"])
@pytest.mark.parametrize("nst", [5, 3])
@pytest.mark.parametrize("shape", MANY_SHAPES, ids=str)
def test_many_items_are_the_single_call(K, shape, nst, d, nrhs):
    """cedar_amd_relax2_lines_many_op32: item m has the bits of the single call on item m alone (and so of the FP64 kernel
    on the rounded arrays); the item beyond nrhs keeps its bits"""
    so, qf, q0, sor, so_r, sor_r = kernel_problem(shape, nst, d)
    qf, q0 = np.ascontiguousarray(qf[:nrhs + 1]), np.ascontiguousarray(q0[:nrhs + 1])
    for ud in (DOWN, UP):
        got = q0.copy()
        single = [q0[m].copy() for m in range(nrhs)]
        for sweep in range(2):
            assert K.relax2_lines_many_op32(so, qf, got, sor, d, ud, nrhs=nrhs) == 0
            for m in range(nrhs):
                assert K.relax2_lines_op32(so, qf[m], single[m], sor, d, ud) == 0
                assert same_bits(got[m], single[m]), (shape, nst, d, nrhs, ud, sweep, m)
        want = q0[nrhs - 1].copy()
        for sweep in range(2):
            K.relax_lines2(so_r, qf[nrhs - 1], want, sor_r, ud, "xy"[d])
        assert same_bits(got[nrhs - 1], want)
        assert same_bits(got[nrhs], q0[nrhs]) and not np.array_equal(got[:nrhs], q0[:nrhs])


# ---------------------------------------------------------------- 3. entry-point refusals
def test_kernel_entry_points_refuse_overflow_bad_nrhs_bad_nstncl_null_and_long_lines(capi, K, capfd):
    """an entry or a factor of 1e39, nrhs of 0 and 33, nstncl 4, a NULL array, a line beyond the LDS: -1, a message naming
    the call, q untouched"""
    for d in (0, 1):
        so, qf, q0, sor, _, _ = kernel_problem((31, 5), 5, d)
        big = so.copy()
        big[2, 3, 4] = 1e39
        bigf = sor.copy()
        bigf.reshape(-1)[3 * 33 + 5] = 1e39  # a pivot of the third line (lines of 31 unknowns: stride 33 either way)
        q1, qm = q0[0], np.ascontiguousarray(q0[:3])
        f1, fm = qf[0], np.ascontiguousarray(qf[:3])
        calls = [
            ("cedar_amd_relax2_lines_op32", q1, lambda a, s, o: K.relax2_lines_op32(a, f1, o, s, d, UP)),
            ("cedar_amd_relax2_lines_many_op32", qm, lambda a, s, o: K.relax2_lines_many_op32(a, fm, o, s, d, UP)),
        ]
        for name, init, call in calls:
            for a, s in ((big, sor), (so, bigf)):
                out = init.copy()
                capfd.readouterr()
                assert call(a, s, out) == -1
                err = capfd.readouterr().err
                assert name in err and "overflows single precision" in err, (name, err)
                assert same_bits(out, init), name
            assert call(so, sor, out) == 0 and not np.array_equal(out, init), name  # and the same call is served
        for nrhs in (0, 33):
            out = qm.copy()
            capfd.readouterr()
            assert K.relax2_lines_many_op32(so, fm, out, sor, d, UP, nrhs=nrhs) == -1
            err = capfd.readouterr().err
            assert "cedar_amd_relax2_lines_many_op32" in err and "nrhs" in err and same_bits(out, qm)
        lib = capi.lib
        JJ, II = (C.c_uint(v) for v in so.shape[1:])
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        out = q1.copy()
        capfd.readouterr()
        lib.cedar_amd_relax2_lines_op32.argtypes = [C.c_void_p] * 4 + [C.c_uint] * 2 + [C.c_int] * 3
        assert lib.cedar_amd_relax2_lines_op32(p(so), p(f1), p(out), p(sor), II, JJ, 4, d, UP) == -1
        assert "nstncl" in capfd.readouterr().err and same_bits(out, q1)
        assert lib.cedar_amd_relax2_lines_op32(p(so), None, p(out), p(sor), II, JJ, 5, d, UP) == -1
        assert "cedar_amd_relax2_lines_op32" in capfd.readouterr().err and same_bits(out, q1)
        assert lib.cedar_amd_relax2_lines_op32(p(so), p(f1), p(out), None, II, JJ, 5, d, UP) == -1
        assert "NULL" in capfd.readouterr().err and same_bits(out, q1)
        # a line of 20000 unknowns needs 180 KB of LDS
        g = (3, 20002) if d == 0 else (20002, 3)
        lo, lf = pb.random_op(g, 3, 881, zero_ghost=False), np.ones((2,) + g)
        lq = pb.uniform(g, 882, -1, 1)
        out = lq.copy()
        capfd.readouterr()
        assert K.relax2_lines_op32(lo, lq, out, lf, d, UP) == -1
        err = capfd.readouterr().err
        assert "cedar_amd_relax2_lines_op32" in err and "LDS" in err and same_bits(out, lq)


# ---------------------------------------------------------------- 4 - 6. the solver
V11 = dict(nrelax_pre=1, nrelax_post=1)
V21 = dict(nrelax_pre=2, nrelax_post=1)
NITEMS = 3
# name -> (operator, relaxation).  aniso9(129,70): levels 129x70 and 65x35 (65 > 64: not small), then LDS-sized ones;
# poisson2(129,70): a five-point level 0; varcoef9(1030,40) / (40,1030): lines of 1030 and 515 unknowns, so levels 0 and 1
# read the scan-ordered factor copy inside a handle; varcoef9(530,520): both scan-ordered copies on level 0, the plain
# float image from level 1 (265x260) on
CASES = {
    "an-x": (lambda: pb.aniso9(129, 70, eps=1e-1), "line-x"),
    "an-y": (lambda: pb.aniso9(129, 70, eps=1e-1), "line-y"),
    "an-xy": (lambda: pb.aniso9(129, 70, eps=1e-1), "line-xy"),
    "p5-xy": (lambda: pb.poisson2(129, 70), "line-xy"),
    "vc-x": (lambda: pb.varcoef9(1030, 40), "line-x"),
    "vc-y": (lambda: pb.varcoef9(40, 1030), "line-y"),
    "vc-xy": (lambda: pb.varcoef9(530, 520), "line-xy"),
}


@functools.lru_cache(maxsize=None)
def solver_problem(name):
    """operator, relaxation, NITEMS right-hand sides (splitmix seeds 17, ...), NITEMS random interior vectors"""
    mk, relax = CASES[name]
    so = mk()
    g = so.shape[1:]
    m = pb.interior_mask(g)
    b = np.stack([pb.uniform(g, 17 + 100 * t, -1, 1) * m for t in range(NITEMS)])
    r = np.stack([pb.uniform(g, 23 + 100 * t, -1, 1) * m for t in range(NITEMS)])
    assert not np.array_equal(rt(so), so)  # not float-representable: the rounded path can differ
    for a in (so, b, r):
        a.setflags(write=False)
    return so, relax, b, r


def smoothed(s):
    return s.nlevels() - 1


def is_small(s, l):
    return max(s.dims(l)[:2]) <= 64  # served by the LDS-resident small-level kernels: never switched, never counted


def levels_taken(s, min_rows):
    return sum(1 for l in range(smoothed(s)) if s.dims(l)[1] >= min_rows and not is_small(s, l))


def round_products(s, relax, a0=None):
    """replace A, SOR0 and (line-xy) SOR1 of every level by their float-rounded values (a0: level 0's A)"""
    for l in range(s.nlevels()):
        A = s.array(l, "A") if (l or a0 is None) else a0
        s.set_array(l, "A", rt(A))
        s.set_array(l, "SOR0", rt(s.array(l, "SOR0")))
        if relax == "line-xy":
            s.set_array(l, "SOR1", rt(s.array(l, "SOR1")))


def handle_outputs(h, cyc, sym, b, r):
    o = {}
    if cyc == "v":
        x = r.copy()
        h.vcycle(x, b)
        o["cycle"] = x
        if sym:  # (precondition refuses a cycle that is not symmetric)
            z = np.zeros_like(r)
            h.precondition(z, r)
            o["z"] = z
        x = np.zeros_like(b)
        o["cg_hist"] = (h.pcg if sym else h.fcg)(b, x, max_iter=12, tol=1e-10)
        o["cg_x"] = x
    else:
        x = np.zeros_like(b)
        o["solve_hist"] = h.solve(b, x)
        o["solve_x"] = x
    return o


@pytest.mark.parametrize("kw,all_levels", [(V11, True), (V21, False)], ids=["v11-all", "v21-level0"])
@pytest.mark.parametrize("name", list(CASES))
def test_cycle_on_rounded_products_is_bit_identical(capi, name, kw, all_levels):
    """two handles whose A, SOR0 and SOR1 are float-representable on every level; one calls
    use_fp32_operator_lines(min_rows), which returns the number of smoothed levels with that many rows that are not
    LDS-sized small levels (min_rows = 1: all of those; min_rows = level 0's rows: level 0 alone, level 1 left out).
    vcycle, precondition, the pcg history and iterate (fcg where the cycle is V(2,1)) do not differ in one bit, nor does
    an F-cycle solve's history and iterate"""
    so, relax, b, r = solver_problem(name)
    sym = kw["nrelax_pre"] == kw["nrelax_post"]
    for cyc in ("v", "f"):
        ref = capi.Solver(so, relax=relax, max_iter=4, tol=0.0, cycle=cyc, **kw)
        s = capi.Solver(so, relax=relax, max_iter=4, tol=0.0, cycle=cyc, **kw)
        assert s.array(0, "A").shape[0] == (3 if name == "p5-xy" else 5) and s.array(1, "A").shape[0] == 5
        round_products(ref, relax)
        round_products(s, relax)
        assert s.fp32_levels() == 0
        min_rows = 1 if all_levels else s.dims(0)[1]
        want_levels = levels_taken(s, min_rows)
        assert levels_taken(s, 1) >= 2
        assert want_levels == (levels_taken(s, 1) if all_levels else 1)
        assert s.use_fp32_operator_lines(min_rows) == want_levels == s.fp32_levels()
        want, got = handle_outputs(ref, cyc, sym, b[0], r[0]), handle_outputs(s, cyc, sym, b[0], r[0])
        ref.close()
        s.close()
        for key in want:
            assert same_bits(got[key], want[key]), (name, cyc, key)
        if cyc == "v":
            assert len(got["cg_hist"]) > 2 and got["cg_hist"][-1] < got["cg_hist"][0] and not np.array_equal(got["cycle"], r[0])
        else:
            assert len(got["solve_hist"]) == 5


@pytest.mark.parametrize("name,kw", [("an-xy", V21), ("p5-xy", V11), ("vc-x", V11), ("vc-y", V21), ("vc-xy", V11)],
                         ids=["an-xy-v21", "p5-xy-v11", "vc-x-v11", "vc-y-v21", "vc-xy-v11"])
def test_batched_cycle_on_rounded_products_is_bit_identical(capi, name, kw):
    """the same with create_many handles: vcycle_many on three items against the FP64 batch handle on the rounded
    products, and pcg_many (fcg_many for V(2,1)) item by item against the single switched handle"""
    so, relax, b, r = solver_problem(name)
    sym = kw["nrelax_pre"] == kw["nrelax_post"]
    ref, s = capi.Solver(so, relax=relax, max_rhs=4, **kw), capi.Solver(so, relax=relax, max_rhs=4, **kw)
    one = capi.Solver(so, relax=relax, **kw)
    for h in (ref, s, one):
        round_products(h, relax)
    assert s.use_fp32_operator_lines(1) == levels_taken(s, 1) == s.fp32_levels() >= 2
    assert one.use_fp32_operator_lines(1) == levels_taken(one, 1)
    want, got = r.copy(), r.copy()
    ref.vcycle_many(want, b)
    s.vcycle_many(got, b)
    assert same_bits(got, want) and not np.array_equal(got, r)
    x = np.zeros_like(b)
    hist, iters = (s.pcg_many if sym else s.fcg_many)(b, x, max_iter=8, tol=1e-10)
    xr = np.zeros_like(b)
    hist_r, iters_r = (ref.pcg_many if sym else ref.fcg_many)(b, xr, max_iter=8, tol=1e-10)
    assert iters == iters_r and same_bits(x, xr) and min(iters) > 2
    for m in range(NITEMS):
        x1 = r[m].copy()
        one.vcycle(x1, b[m])
        assert same_bits(got[m], x1), (name, m)
        x1 = np.zeros_like(b[m])
        h1 = (one.pcg if sym else one.fcg)(b[m], x1, max_iter=8, tol=1e-10)
        assert same_bits(hist[m], h1) and same_bits(x[m], x1), (name, m)
    for h in (ref, s, one):
        h.close()


# ---------------------------------------------------------------- 5. real operators
def abs_apply(so, x):
    """|A| |x| on the interior (the magnitudes of the terms b - A x sums), zero elsewhere"""
    a, v = np.abs(so), np.abs(x)
    out = np.zeros_like(x)
    c = (slice(1, -1), slice(1, -1))
    sh = lambda arr, dj, di: arr[1 + dj:arr.shape[0] - 1 + dj, 1 + di:arr.shape[1] - 1 + di]
    t = a[KO][c] * v[c] + a[KW][c] * sh(v, 0, -1) + sh(a[KW], 0, 1) * sh(v, 0, 1) + a[KS][c] * sh(v, -1, 0) \
        + sh(a[KS], 1, 0) * sh(v, 1, 0)
    if so.shape[0] == 5:
        t = t + a[KSW][c] * sh(v, -1, -1) + sh(a[KNW], 0, 1) * sh(v, -1, 1) + sh(a[KNW], 1, 0) * sh(v, 1, -1) \
            + sh(a[KSW], 1, 1) * sh(v, 1, 1)
    out[c] = t
    return out


def true_relres(O, so, b, x):
    ax = np.zeros_like(b)
    O.matvec2(so, np.ascontiguousarray(x), ax)
    m = pb.interior_mask(b.shape)
    return np.linalg.norm((b - ax)[m]) / np.linalg.norm(b[m])


def rounding_bound(so, b, x):
    """Library and oracle both evaluate b - A x in floating point: up to ten terms a point, so each entry carries an error
    of at most 11 u (|b| + |A| |x|), u = 2^-53, in either evaluation -- 22 u for the two"""
    m = pb.interior_mask(b.shape)
    return 22 * 2.0 ** -53 * np.linalg.norm((np.abs(b) + abs_apply(so, x))[m]) / np.linalg.norm(b[m])


@pytest.mark.parametrize("name", list(CASES))
def test_real_operator_converges_to_the_fp64_solution(capi, name):
    """the unrounded operator, FP64 handle against a handle after use_fp32_operator_lines(1): pcg (V(1,1)), fcg (V(2,1))
    and solve (V(2,1)) to 1e-10.  Both handles meet the stop test; the true relative residual (oracle matvec on the
    unrounded so) is within tol plus the rounding bound of evaluating b - A x twice; the iteration counts differ by at
    most one; the iterates differ"""
    from pyoracle import Oracle
    O = Oracle()
    so, relax, bb, _ = solver_problem(name)
    b = bb[0]
    tol = 1e-10
    for kind, kw in (("pcg", V11), ("fcg", V21), ("solve", V21)):
        # (max_iter 150: the plain V(2,1) cycle with y lines alone contracts slowly on the anisotropic operator, whose strong
        # coupling runs along x, and needs 101 cycles, FP64 or not -- checked beforehand with the CPU oracle, which takes 9 to
        # 11 cycles on the six other cases; the Krylov runs need fewer iterations than the plain cycle needs cycles)
        ref = capi.Solver(so, relax=relax, max_iter=150, tol=tol, **kw)
        s = capi.Solver(so, relax=relax, max_iter=150, tol=tol, **kw)
        assert s.use_fp32_operator_lines(1) == levels_taken(s, 1) >= 2 and ref.fp32_levels() == 0
        x_ref, x = np.zeros_like(b), np.zeros_like(b)
        if kind == "solve":
            h_ref, h = ref.solve(b, x_ref), s.solve(b, x)
        else:
            h_ref, h = getattr(ref, kind)(b, x_ref, max_iter=60, tol=tol), getattr(s, kind)(b, x, max_iter=60, tol=tol)
        rr_ref, rr = true_relres(O, so, b, x_ref), true_relres(O, so, b, x)
        bound = rounding_bound(so, b, x)
        print("%s %s: iterations fp64 %d, fp32-operator %d; last %.4e, %.4e; true relative residual %.4e, %.4e; bound %.3e"
              % (name, kind, len(h_ref) - 1, len(h) - 1, h_ref[-1], h[-1], rr_ref, rr, bound))
        ref.close()
        s.close()
        assert h_ref[-1] < tol and h[-1] < tol and len(h) - 1 < (150 if kind == "solve" else 60)
        assert rr <= tol + bound and rr_ref <= tol + bound
        assert abs(len(h) - len(h_ref)) <= 1
        assert not np.array_equal(x, x_ref)


# ---------------------------------------------------------------- 6. rules
@pytest.mark.parametrize("mk", [pb.varcoef9, pb.poisson2], ids=["nine-point", "five-point"])
def test_default_min_rows_takes_a_level_of_1024_rows(capi, mk):
    """min_rows = 0: the measured default switches a level with at least 1024 rows and leaves one
    with 1023 in FP64; the level below (35 x 512, not a small level) stays FP64 either way"""
    for ny, want in ((1024, 1), (1023, 0)):
        s = capi.Solver(mk(70, ny), relax="line-xy", **V11)
        assert smoothed(s) >= 2 and s.dims(1)[1] < 1024 and not is_small(s, 0) and not is_small(s, 1)
        assert s.use_fp32_operator_lines(0) == want == s.fp32_levels()
        assert s.use_fp32_operator_lines(ny) == 1  # an explicit min_rows switches level 0 in both cases
        s.close()


def test_min_rows_env_overrides_the_default(capi, monkeypatch):
    """CEDAR_AMD_OP32_MIN_ROWS, read at the call, stands in for min_rows = 0; an explicit min_rows wins over it"""
    so, relax, b, r = solver_problem("vc-xy")
    s = capi.Solver(so, relax=relax, **V11)
    assert s.use_fp32_operator_lines(0) == 0  # 520 rows: below the default
    monkeypatch.setenv("CEDAR_AMD_OP32_MIN_ROWS", "500")
    assert s.use_fp32_operator_lines(0) == 1 == levels_taken(s, 500)
    monkeypatch.setenv("CEDAR_AMD_OP32_MIN_ROWS", "200")
    assert s.use_fp32_operator_lines(0) == 2 == levels_taken(s, 200)
    assert s.use_fp32_operator_lines(100) == 3 == levels_taken(s, 100)
    s.close()


def test_repetition_is_idempotent_never_switches_back_and_never_counts_small_levels(capi):
    so, relax, b, r = solver_problem("vc-xy")
    s = capi.Solver(so, relax=relax, **V11)
    n200 = levels_taken(s, 200)
    assert s.use_fp32_operator_lines(200) == n200 == 2
    z1 = np.zeros_like(r[0])
    s.precondition(z1, r[0])
    assert s.use_fp32_operator_lines(200) == n200 and s.use_fp32_operator_lines(5000) == n200
    z2 = np.zeros_like(r[0])
    s.precondition(z2, r[0])
    assert same_bits(z1, z2)
    # min_rows = 1: every level of more than 64 x 64 unknowns, and none of the LDS-sized ones below them
    nsmall = sum(1 for l in range(smoothed(s)) if is_small(s, l))
    assert nsmall >= 1 and s.use_fp32_operator_lines(1) == smoothed(s) - nsmall == s.use_fp32_operator_lines(1)
    s.close()
    # a handle whose smoothed levels are all small switches nothing
    t = capi.Solver(pb.varcoef9(40, 30), relax="line-xy", **V11)
    assert smoothed(t) >= 2 and t.use_fp32_operator_lines(1) == 0 == t.fp32_levels()
    t.close()


@pytest.mark.parametrize("name", ["an-xy", "vc-x", "vc-y"])
def test_set_after_the_switch_rebuilds_the_float_copies(capi, capfd, name):
    """cedar_amd_solver_set("A" | "SOR0" | "SOR1") on a switched level: the bits of a fresh handle built on those arrays
    and switched, and of a plain FP64 handle on the rounded products; an A with an entry of 1e39 is reported and the
    level reads FP64 again"""
    so, relax, b, r = solver_problem(name)
    r = r[0]
    facs = ["SOR0", "SOR1"] if relax == "line-xy" else ["SOR0"]
    a_new = rt(so * pb.uniform(so.shape, 861, 0.97, 1.03))
    s = capi.Solver(so, relax=relax, **V11)
    round_products(s, relax)
    n = s.use_fp32_operator_lines(1)
    assert n == levels_taken(s, 1) >= 2
    fac_new = {f: rt(s.array(0, f) * 0.98) for f in facs}
    z_old = np.zeros_like(r)
    s.precondition(z_old, r)
    s.set_array(0, "A", a_new)
    for f in facs:
        s.set_array(0, f, fac_new[f])
    fresh, plain = capi.Solver(so, relax=relax, **V11), capi.Solver(so, relax=relax, **V11)
    for h in (fresh, plain):
        round_products(h, relax, a0=a_new)
        for f in facs:
            h.set_array(0, f, fac_new[f])
    assert fresh.use_fp32_operator_lines(1) == n
    z, z_fresh, z_plain = np.zeros_like(r), np.zeros_like(r), np.zeros_like(r)
    s.precondition(z, r)
    fresh.precondition(z_fresh, r)
    plain.precondition(z_plain, r)
    assert same_bits(z, z_fresh) and same_bits(z, z_plain) and not np.array_equal(z, z_old)
    big = a_new.copy()
    big[1, 5, 6] = 1e39
    capfd.readouterr()
    s.set_array(0, "A", big)
    assert "overflows single precision" in capfd.readouterr().err
    assert s.fp32_levels() == n - 1
    plain.set_array(0, "A", big)
    s.precondition(z, r)
    plain.precondition(z_plain, r)
    assert same_bits(z, z_plain)
    # and an overflowing factor on the next level
    bigf = s.array(1, facs[-1]).copy()
    nx1, ny1 = s.dims(1)[:2]
    ld = nx1 + 2 if relax == "line-x" else ny1 + 2  # x factors are SOR(II,JJ,2), y factors SOR(JJ,II,2)
    bigf.reshape(-1)[3 * ld + 5] = 1e39  # a pivot of the third line
    capfd.readouterr()
    s.set_array(1, facs[-1], bigf)
    assert "overflows single precision" in capfd.readouterr().err
    assert s.fp32_levels() == n - 2
    plain.set_array(1, facs[-1], bigf)
    s.precondition(z, r)
    plain.precondition(z_plain, r)
    assert same_bits(z, z_plain)
    for h in (s, fresh, plain):
        h.close()


def test_refusals_leave_the_handle_as_it_was(capi, capfd, monkeypatch):
    """NULL handle, 3D handle, point relaxation, ibc = 2, y lines without transposed arrays, min_rows = -1, an entry of
    1e39: -1, a message, fp32_levels() == 0 and the next cycle's bits unchanged"""
    so2, b2 = pb.varcoef9(140, 90), pb.rhs2(140, 90)

    def refused(s, text, b, min_rows=1):
        def run():
            x = np.zeros_like(b)
            return [s.solve(b, x), x]
        before = run()
        capfd.readouterr()
        rc = s.use_fp32_operator_lines(min_rows)
        err = capfd.readouterr().err
        assert rc == -1 and "cedar_amd_solver_use_fp32_operator_lines" in err and text in err, (text, err)
        assert s.fp32_levels() == 0
        assert all(same_bits(a, c) for a, c in zip(before, run())), text
        s.close()

    refused(capi.Solver(pb.poisson3(9, 9, 9), max_iter=2, **V11), "3D handles", pb.rhs3(9, 9, 9))
    refused(capi.Solver(so2, relax="point", max_iter=2, **V11), "cedar_amd_solver_use_fp32_operator_2d", b2)
    per = (True, False)
    refused(capi.Solver(pb.periodic_poisson2(16, 16, per), relax="line-x", max_iter=2, ibc=pb.ibc_of(per), **V11), "periodic",
            pb.periodic_rhs2(16, 16, per))
    assert pb.ibc_of(per) == 2
    monkeypatch.setenv("CEDAR_AMD_YLINES_TRANSPOSED", "0")
    refused(capi.Solver(so2, relax="line-xy", max_iter=2), "CEDAR_AMD_YLINES_TRANSPOSED", b2)
    refused(capi.Solver(so2, relax="line-y", max_iter=2), "CEDAR_AMD_YLINES_TRANSPOSED", b2)
    ok = capi.Solver(so2, relax="line-x", max_iter=2)  # x lines keep no transposed arrays and are served
    assert ok.use_fp32_operator_lines(1) == levels_taken(ok, 1) >= 1
    ok.close()
    monkeypatch.delenv("CEDAR_AMD_YLINES_TRANSPOSED")
    refused(capi.Solver(so2, relax="line-xy", max_iter=2), "min_rows", b2, min_rows=-1)
    refused(capi.Solver(so2, relax="line-y", max_rhs=4, max_iter=2), "min_rows", b2, min_rows=-1)
    big = so2.copy()
    big[1, 9, 9] = 1e39
    refused(capi.Solver(big, relax="line-xy", max_iter=1), "overflows single precision", b2)
    capfd.readouterr()
    assert capi.lib.cedar_amd_solver_use_fp32_operator_lines(None, 1) == -1
    assert "NULL solver handle" in capfd.readouterr().err
