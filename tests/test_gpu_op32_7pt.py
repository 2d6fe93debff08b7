"""The 7-point operator of the cycle kept in single precision (cedar_amd_solver_use_fp32_operator_all, the float view of
op7f.hip), single vector and batch.

Promoting a float to double is exact, so a kernel that reads the float copy and promotes on load does the FP64 kernel's
arithmetic on the operator rounded to float: sections 1, 2, 4 and 6 compare bit patterns, no tolerance.  Section 5 runs
the real (unrounded) operator, where the switched handle's preconditioner differs from the FP64 one by a relative 6e-8.

Measured on an MI355X (section 5, tol 1e-10; FP64 handle / handle after use_fp32_operator_all(1); the true relative
residual is the oracle's matvec on the unrounded operator):
  diag_diffusion3(40,33,50; 1, .8, 1.3)  pcg V(1,1) 15 / 15 iterations, 4.6255e-11 / 4.6255e-11;  fcg V(2,1) 12 / 12,
                                         1.7278e-11 / 1.7278e-11;  solve V(2,1) 18 / 18 cycles, 8.0171e-11 / 8.0171e-11
  poisson3(65,65,65)                     pcg 10 / 10, 4.1876e-11 / 4.1876e-11;  fcg 9 / 9, 6.9470e-12 / 6.9470e-12;
                                         solve 11 / 11 cycles, 3.6163e-11 / 3.6163e-11
  high_contrast7(24,24,24)               pcg 15 / 15, 6.0962e-11 / 5.1700e-11;  fcg 14 / 14, 9.5585e-11 / 9.4920e-11;
                                         solve 75 / 75 cycles, 8.5217e-11 / 8.7273e-11 (true 8.8004e-11: within the
                                         rounding bound of evaluating b - A x twice, 4.96e-10)
(the right-hand sides here are splitmix fields of seed 17 scaled to [-1, 1] on the interior, x0 = 0)
"""
import ctypes as C
import functools

import numpy as np
import pytest

import problems as pb
import pcg_statement as ps

pytestmark = pytest.mark.gpu

DOWN, UP = 0, 1

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


# ---------------------------------------------------------------- 1. kernels, bit for bit
# nx x ny x nz.  The launchers of op7f.hip take one workgroup per grid row and step only in the workgroup size: the sweep
# has 64 / 128 / 256 lanes for up to 64 / 128 / more colour points (ceil(nx / 2)) of a row, the residual for up to
# 64 / 128 / more points (nx).
#   (1,1,1), (2,3,2)        the smallest grids: one point, and rows with one point of a colour
#   (30,9,6), (31,9,6)      II = 32 / 33: either side of the float row padding, even and odd row length
#   (63..65,5,4)            residual 64 -> 128 lanes at nx = 64 | 65
#   (127,5,4), (129,5,4)    sweep 64 -> 128 lanes (64 | 65 colour points); residual 128 -> 256 lanes (128 | 129 points)
#   (256,4,3), (257,4,3)    sweep 128 -> 256 lanes (128 | 129 colour points); residual lane loop: second trip at 257
#   (513,4,3)               sweep lane loop: second trip (257 colour points on 256 lanes)
#   (1030,3,3)              rows beyond 1024 points are served: sweep third trip, residual fifth
#   (40,33,50)              1650 rows: more workgroups than one wave of them on the card, all three extents different
# There is no row loop: a workgroup serves one row.
SHAPES = [(1, 1, 1), (2, 3, 2), (30, 9, 6), (31, 9, 6), (63, 5, 4), (64, 5, 4), (65, 5, 4), (127, 5, 4), (129, 5, 4),
          (256, 4, 3), (257, 4, 3), (513, 4, 3), (1030, 3, 3), (40, 33, 50)]
NRHS = [1, 3, 9]
MANY_SHAPES = SHAPES


@functools.lru_cache(maxsize=None)
def kernel_problem(shape):
    nx, ny, nz = shape
    g = (nz + 2, ny + 2, nx + 2)
    so = pb.random_op(g, 4, 741, zero_ghost=False)
    sor = np.zeros((2,) + g)
    from pyoracle import Oracle
    Oracle().setup_recip3(so, sor)
    n = max(NRHS) + 1  # one item beyond the largest batch
    qf = np.stack([pb.uniform(g, 742 + 17 * m, -1, 1) for m in range(n)])  # non-zero ghost cells
    q0 = np.stack([pb.uniform(g, 743 + 17 * m, -1, 1) for m in range(n)])
    so_r, sor_r = rt(so), rt(sor)
    assert not np.array_equal(so_r, so) and not np.array_equal(sor_r, sor)
    for a in (so, qf, q0, sor, so_r, sor_r):
        a.setflags(write=False)
    return so, qf, q0, sor, so_r, sor_r


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_relax_is_the_fp64_sweep_on_the_rounded_operator(K, shape):
    """cedar_amd_relax7_gs_op32 on (so, sor) against BMG3_SymStd_relax_GS on (rt(so), rt(sor)): both directions, three
    sweeps in a row, every element of q (ghost cells included) with == on the bit patterns"""
    so, qf, q0, sor, so_r, sor_r = kernel_problem(shape)
    for ud in (DOWN, UP):
        want, got = q0[0].copy(), q0[0].copy()
        for sweep in range(3):
            K.relax3(so_r, qf[0], want, sor_r, ud)
            assert K.relax7_op32(so, qf[0], got, sor, ud) == 0
            assert same_bits(got, want), (shape, ud, sweep, np.max(np.abs(got - want)))
        assert not np.array_equal(got, q0[0])


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_residual_is_the_fp64_residual_on_the_rounded_operator(K, shape):
    """cedar_amd_residual7_op32 against BMG3_SymStd_residual on rt(so) into a sentinel-filled array: every element of
    res, everything outside the interior untouched"""
    so, qf, q0, sor, so_r, sor_r = kernel_problem(shape)
    sentinel = pb.uniform(q0[0].shape, 744, -1, 1)
    want, got = sentinel.copy(), sentinel.copy()
    K.residual3(so_r, qf[0], q0[0], want)
    assert K.residual7_op32(so, qf[0], q0[0], got) == 0
    assert same_bits(got, want), (shape, np.max(np.abs(got - want)))
    m = ~pb.interior_mask(q0[0].shape)
    assert same_bits(got[m], sentinel[m]) and not np.array_equal(got, sentinel)


@pytest.mark.parametrize("nrhs", NRHS)
@pytest.mark.parametrize("shape", MANY_SHAPES, ids=str)
def test_relax_many_items_are_the_single_call_and_the_fp64_batched_sweep(K, shape, nrhs):
    """cedar_amd_relax7_gs_many_op32: item m equals cedar_amd_relax7_gs_op32 on item m alone and
    cedar_amd_relax3_gs_many on the rounded arrays; the item beyond nrhs keeps its bits.  Both directions, three sweeps"""
    so, qf, q0, sor, so_r, sor_r = kernel_problem(shape)
    qf, q0 = np.ascontiguousarray(qf[:nrhs + 1]), np.ascontiguousarray(q0[:nrhs + 1])
    for ud in (DOWN, UP):
        want, got = q0.copy(), q0.copy()
        single = [q0[m].copy() for m in range(nrhs)]
        for sweep in range(3):
            K.relax3_many(so_r, qf, want, sor_r, ud, nrhs=nrhs)
            assert K.relax7_many_op32(so, qf, got, sor, ud, nrhs=nrhs) == 0
            assert same_bits(got, want), (shape, nrhs, ud, sweep, np.max(np.abs(got - want)))
            for m in range(nrhs):
                assert K.relax7_op32(so, qf[m], single[m], sor, ud) == 0
                assert same_bits(got[m], single[m]), (shape, nrhs, ud, sweep, m)
        assert same_bits(got[nrhs], q0[nrhs]) and not np.array_equal(got[:nrhs], q0[:nrhs])


@pytest.mark.parametrize("nrhs", NRHS)
@pytest.mark.parametrize("shape", MANY_SHAPES, ids=str)
def test_residual_many_items_are_the_single_call_and_the_fp64_batched_residual(K, shape, nrhs):
    """cedar_amd_residual7_many_op32 against cedar_amd_residual3_many on rt(so) and, per item, against
    cedar_amd_residual7_op32; ghost cells and the item beyond nrhs keep the sentinel's bits"""
    so, qf, q0, sor, so_r, sor_r = kernel_problem(shape)
    qf, q0 = np.ascontiguousarray(qf[:nrhs + 1]), np.ascontiguousarray(q0[:nrhs + 1])
    sentinel = np.stack([pb.uniform(q0.shape[1:], 745 + m, -1, 1) for m in range(nrhs + 1)])
    want, got = sentinel.copy(), sentinel.copy()
    K.residual3_many(so_r, qf, q0, want, nrhs=nrhs)
    assert K.residual7_many_op32(so, qf, q0, got, nrhs=nrhs) == 0
    assert same_bits(got, want), (shape, nrhs, np.max(np.abs(got - want)))
    ghost = ~pb.interior_mask(q0.shape[1:])
    for m in range(nrhs):
        one = sentinel[m].copy()
        assert K.residual7_op32(so, qf[m], q0[m], one) == 0
        assert same_bits(got[m], one), (shape, nrhs, m)
        assert same_bits(got[m][ghost], sentinel[m][ghost]) and not np.array_equal(got[m], sentinel[m])
    assert same_bits(got[nrhs], sentinel[nrhs])


# ---------------------------------------------------------------- 2. entry-point refusals
def test_kernel_entry_points_refuse_overflow_and_bad_nrhs(capi, K, capfd):
    """an entry of 1e39, nrhs of 0 and 33, a NULL array: -1, a message naming the call, outputs untouched"""
    so, qf, q0, sor, _, _ = kernel_problem((31, 9, 6))
    big = so.copy()
    big[2, 3, 4, 7] = 1e39
    q1, qm = q0[0], np.ascontiguousarray(q0[:3])
    f1, fm = qf[0], np.ascontiguousarray(qf[:3])
    calls = [
        ("cedar_amd_relax7_gs_op32", q1, lambda a, o: K.relax7_op32(a, f1, o, sor, UP)),
        ("cedar_amd_residual7_op32", q1, lambda a, o: K.residual7_op32(a, f1, q1, o)),
        ("cedar_amd_relax7_gs_many_op32", qm, lambda a, o: K.relax7_many_op32(a, fm, o, sor, UP)),
        ("cedar_amd_residual7_many_op32", qm, lambda a, o: K.residual7_many_op32(a, fm, qm, o)),
    ]
    for name, init, call in calls:
        out = init.copy()
        capfd.readouterr()
        assert call(big, out) == -1
        err = capfd.readouterr().err
        assert name in err and "overflows single precision" in err, (name, err)
        assert same_bits(out, init), name
        assert call(so, out) == 0 and not np.array_equal(out, init), name  # and the same call is served on so
    for nrhs in (0, 33):
        out = qm.copy()
        capfd.readouterr()
        assert K.relax7_many_op32(so, fm, out, sor, UP, nrhs=nrhs) == -1
        err = capfd.readouterr().err
        assert "cedar_amd_relax7_gs_many_op32" in err and "nrhs" in err and same_bits(out, qm)
        assert K.residual7_many_op32(so, fm, qm, out, nrhs=nrhs) == -1
        err = capfd.readouterr().err
        assert "cedar_amd_residual7_many_op32" in err and "nrhs" in err and same_bits(out, qm)
    # a NULL array
    lib = capi.lib
    II, JJ, KK = (C.c_uint(v) for v in (33, 11, 8))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    out = q1.copy()
    capfd.readouterr()
    lib.cedar_amd_relax7_gs_op32.argtypes = [C.c_void_p] * 4 + [C.c_uint] * 3 + [C.c_int]
    lib.cedar_amd_residual7_op32.argtypes = [C.c_void_p] * 4 + [C.c_uint] * 3
    assert lib.cedar_amd_relax7_gs_op32(p(so), None, p(out), p(sor), II, JJ, KK, UP) == -1
    assert "cedar_amd_relax7_gs_op32" in capfd.readouterr().err and same_bits(out, q1)
    assert lib.cedar_amd_residual7_op32(None, p(f1), p(q1), p(out), II, JJ, KK) == -1
    assert "cedar_amd_residual7_op32" in capfd.readouterr().err and same_bits(out, q1)


# ---------------------------------------------------------------- 3 - 6. the solver
V11 = dict(relax="point", nrelax_pre=1, nrelax_post=1)
V21 = dict(relax="point", nrelax_pre=2, nrelax_post=1)
NITEMS = 3


@functools.lru_cache(maxsize=None)
def solver_problem(name):
    """operator, NITEMS right-hand sides (splitmix seeds 17, ...), NITEMS random interior vectors"""
    so = {"dd": lambda: pb.diag_diffusion3(40, 33, 50, 1.0, 0.8, 1.3), "p65": lambda: pb.poisson3(65, 65, 65),
          "hc": lambda: ps.high_contrast7(24, 24, 24)}[name]()
    g = so.shape[1:]
    m = pb.interior_mask(g)
    b = np.stack([pb.uniform(g, 17 + 100 * t, -1, 1) * m for t in range(NITEMS)])
    r = np.stack([pb.uniform(g, 23 + 100 * t, -1, 1) * m for t in range(NITEMS)])
    assert not np.array_equal(rt(so), so)  # not float-representable: the rounded path can differ
    for a in (so, b, r):
        a.setflags(write=False)
    return so, b, r


def smoothed(s):
    return s.nlevels() - 1


def round_products(s, a0=None):
    """replace A and SOR0 of every level by their float-rounded values (a0: level 0's A instead of what it holds)"""
    for l in range(s.nlevels()):
        A = s.array(l, "A") if (l or a0 is None) else a0
        s.set_array(l, "A", rt(A))
        s.set_array(l, "SOR0", rt(s.array(l, "SOR0")))


ROUNDED_CASES = [("dd", V21), ("p65", V11)]


@pytest.mark.parametrize("name,kw", ROUNDED_CASES, ids=["dd-v21", "p65-v11"])
def test_cycle_on_rounded_products_is_bit_identical(capi, monkeypatch, name, kw):
    """two handles whose A and SOR0 are float-representable on every level; one calls use_fp32_operator_all(1), which
    returns the number of smoothed levels, level 0 included.  vcycle, precondition, the pcg history and iterate (fcg
    where the cycle is V(2,1), which pcg refuses) do not differ in one bit, nor does an F-cycle solve's history.
    CEDAR_AMD_PSUM=0: the 27-point levels below run the reference order on both handles."""
    so, b, r = solver_problem(name)
    monkeypatch.setenv("CEDAR_AMD_PSUM", "0")
    monkeypatch.delenv("CEDAR_AMD_FRUN", raising=False)
    sym = kw["nrelax_pre"] == kw["nrelax_post"]
    for cyc in ("v", "f"):
        ref, s = capi.Solver(so, max_iter=4, tol=0.0, cycle=cyc, **kw), capi.Solver(so, max_iter=4, tol=0.0, cycle=cyc, **kw)
        assert s.array(0, "A").shape[0] == 4 and smoothed(s) >= 2
        round_products(ref)
        round_products(s)
        assert s.fp32_levels() == 0
        assert s.use_fp32_operator_all(1) == smoothed(s) == s.fp32_levels()
        outs = []
        for h in (ref, s):
            o = {}
            if cyc == "v":
                x = r[0].copy()
                h.vcycle(x, b[0])
                o["cycle"] = x
                z = np.zeros_like(r[0])
                h.precondition(z, r[0])
                o["z"] = z
                x = np.zeros_like(b[0])
                o["cg_hist"] = (h.pcg if sym else h.fcg)(b[0], x, max_iter=30, tol=1e-10)
                o["cg_x"] = x
            else:
                x = np.zeros_like(b[0])
                o["solve_hist"] = h.solve(b[0], x)
                o["solve_x"] = x
            outs.append(o)
        ref.close()
        s.close()
        want, got = outs
        for key in want:
            assert same_bits(got[key], want[key]), (name, cyc, key)
        if cyc == "v":
            assert len(got["cg_hist"]) > 2 and got["cg_hist"][-1] < 1e-10 and not np.array_equal(got["cycle"], r[0])
        else:
            assert len(got["solve_hist"]) == 5


@pytest.mark.parametrize("name,kw", ROUNDED_CASES, ids=["dd-v21", "p65-v11"])
def test_batched_cycle_on_rounded_products_is_bit_identical(capi, monkeypatch, name, kw):
    """the same with create_many handles: vcycle_many on three items against the FP64 batch handle on the rounded
    products, and pcg_many (fcg_many for V(2,1)) item by item against the single switched handle"""
    so, b, r = solver_problem(name)
    monkeypatch.setenv("CEDAR_AMD_PSUM", "0")
    monkeypatch.delenv("CEDAR_AMD_FRUN", raising=False)
    sym = kw["nrelax_pre"] == kw["nrelax_post"]
    ref, s, one = capi.Solver(so, max_rhs=4, **kw), capi.Solver(so, max_rhs=4, **kw), capi.Solver(so, **kw)
    for h in (ref, s, one):
        round_products(h)
    assert s.use_fp32_operator_all(1) == smoothed(s) == s.fp32_levels()
    assert one.use_fp32_operator_all(1) == smoothed(one)
    want, got = r.copy(), r.copy()
    ref.vcycle_many(want, b)
    s.vcycle_many(got, b)
    assert same_bits(got, want) and not np.array_equal(got, r)
    x = np.zeros_like(b)
    hist, iters = (s.pcg_many if sym else s.fcg_many)(b, x, max_iter=30, tol=1e-10)
    xr = np.zeros_like(b)
    hist_r, iters_r = (ref.pcg_many if sym else ref.fcg_many)(b, xr, max_iter=30, tol=1e-10)
    assert iters == iters_r and same_bits(x, xr) and min(iters) > 2
    for m in range(NITEMS):
        x1 = r[m].copy()
        one.vcycle(x1, b[m])
        assert same_bits(got[m], x1), (name, m)
        x1 = np.zeros_like(b[m])
        h1 = (one.pcg if sym else one.fcg)(b[m], x1, max_iter=30, tol=1e-10)
        assert same_bits(hist[m], h1) and same_bits(x[m], x1), (name, m)
    # nrhs == 1 on the batch handle: the single-vector float kernels
    x1, xm = r[0].copy(), r[:1].copy()
    one.vcycle(x1, b[0])
    s.vcycle_many(xm, b[:1])
    assert same_bits(xm[0], x1)
    for h in (ref, s, one):
        h.close()


def test_the_existing_calls_leave_the_7_point_level_alone(capi, monkeypatch):
    """on a 7-point handle use_fp32_operator(1) returns the number of smoothed 27-point levels and level 0 stays FP64
    (its cycle has the bits of a handle whose coarse levels alone are rounded); _all(1) then returns one more, and a
    second _all(1) the same; use_fp32_operator_many likewise on a batch handle; _all(0) leaves level 0 to its default"""
    so, b, r = solver_problem("dd")
    monkeypatch.setenv("CEDAR_AMD_PSUM", "0")
    s, ref = capi.Solver(so, **V11), capi.Solver(so, **V11)
    for h in (s, ref):  # the 27-point levels' products float-representable on both, level 0 as it is
        for l in range(1, h.nlevels()):
            h.set_array(l, "A", rt(h.array(l, "A")))
            h.set_array(l, "SOR0", rt(h.array(l, "SOR0")))
    n27 = smoothed(s) - 1
    assert n27 >= 1 and s.use_fp32_operator(1) == n27 == s.fp32_levels()
    z27 = np.zeros_like(r[0])
    s.precondition(z27, r[0])
    z_ref = np.zeros_like(r[0])  # FP64 kernels throughout: equal only if level 0 of s still reads the unrounded FP64 A
    ref.precondition(z_ref, r[0])
    assert same_bits(z27, z_ref)
    assert s.use_fp32_operator_all(1) == n27 + 1 == s.fp32_levels()
    assert s.use_fp32_operator_all(1) == n27 + 1
    assert s.use_fp32_operator(1) == n27 + 1  # the count includes the 7-point level; nothing switches back
    z = np.zeros_like(r[0])
    s.precondition(z, r[0])
    assert not np.array_equal(z, z27)
    m = capi.Solver(so, max_rhs=4, **V11)
    assert m.use_fp32_operator_many(1) == n27 and m.use_fp32_operator_all(1) == n27 + 1 == m.use_fp32_operator_all(1)
    d = capi.Solver(so, **V11)
    n_default = d.use_fp32_operator_all(0)
    assert n_default == d.fp32_levels() and 0 <= n_default <= n27 + 1
    for h in (s, ref, m, d):
        h.close()


def test_default_min_rows_takes_a_7_point_level_of_128_rows(capi, monkeypatch):
    """min_rows = 0: the measured default switches a 7-point level 0 with at least 128 rows and
    leaves one with 127 in FP64; the 27-point level below (64 rows) is under its own default of 128 either way, and the
    older call switches nothing on such a handle"""
    monkeypatch.delenv("CEDAR_AMD_OP32_MIN_ROWS", raising=False)
    for ny, want in ((128, 1), (127, 0)):
        s = capi.Solver(pb.diag_diffusion3(9, ny, 9, 1.0, 0.8, 1.3), **V11)
        assert smoothed(s) >= 2 and s.dims(1)[1] < 128
        assert s.use_fp32_operator(0) == 0
        assert s.use_fp32_operator_all(0) == want == s.fp32_levels()
        assert s.use_fp32_operator_all(ny) == 1  # an explicit min_rows switches it in both cases
        s.close()


def true_relres(O, so, b, x):
    ax = np.zeros_like(b)
    O.matvec3(so, np.ascontiguousarray(x), ax)
    m = pb.interior_mask(b.shape)
    return np.linalg.norm((b - ax)[m]) / np.linalg.norm(b[m])


@pytest.mark.parametrize("name", ["dd", "p65", "hc"])
def test_real_operator_converges_to_the_fp64_solution(capi, name):
    """the unrounded operator, FP64 handle against a handle after use_fp32_operator_all(1): pcg (V(1,1)) and fcg (V(2,1))
    to 1e-10 reach a true relative residual (oracle matvec on the unrounded so) below 1e-10 within one iteration of the
    FP64 handle's count, with an x that differs in some bit; solve (V(2,1)) takes the same number of cycles +-1 and
    reports the FP64 residual"""
    from pyoracle import Oracle
    O = Oracle()
    so, bb, _ = solver_problem(name)
    b = bb[0]
    tol = 1e-10
    for kind, kw in (("pcg", V11), ("fcg", V21)):
        # (max_iter 100: the plain cycle needs some 65 iterations on the high-contrast operator, FP64 or not)
        ref, s = capi.Solver(so, max_iter=100, tol=tol, **kw), capi.Solver(so, max_iter=100, tol=tol, **kw)
        assert s.use_fp32_operator_all(1) == smoothed(s) and ref.fp32_levels() == 0
        x_ref, x = np.zeros_like(b), np.zeros_like(b)
        h_ref, h = getattr(ref, kind)(b, x_ref, max_iter=50, tol=tol), getattr(s, kind)(b, x, max_iter=50, tol=tol)
        rr_ref, rr = true_relres(O, so, b, x_ref), true_relres(O, so, b, x)
        print("%s %s: iterations fp64 %d, fp32-operator %d; true relative residual %.4e, %.4e"
              % (name, kind, len(h_ref) - 1, len(h) - 1, rr_ref, rr))
        assert h[-1] < tol and rr < tol
        assert abs((len(h) - 1) - (len(h_ref) - 1)) <= 1
        assert not np.array_equal(x, x_ref)
        if kind == "fcg":
            x_ref, x = np.zeros_like(b), np.zeros_like(b)
            c_ref, c = ref.solve(b, x_ref), s.solve(b, x)
            rr = true_relres(O, so, b, x)
            print("%s solve: cycles fp64 %d, fp32-operator %d; last relative residual %.4e, %.4e; true %.4e"
                  % (name, len(c_ref) - 1, len(c) - 1, c_ref[-1], c[-1], rr))
            assert c_ref[-1] < tol and c[-1] < tol and len(c) - 1 < 100 and abs(len(c) - len(c_ref)) <= 1
            # the reported residual is the FP64 operator's.  Library and oracle both evaluate b - A x in floating point,
            # eight terms a point, each with an error of at most 8 u (|b| + |A| |x|) per entry, u = 2^-53, and |A| |x| <=
            # 2 diag |x| for these diagonally dominant operators; the two norms' own rounding is below 1e-9 relative
            m = pb.interior_mask(b.shape)
            bound = 16 * 2.0 ** -53 * np.linalg.norm((np.abs(b) + 2 * so[0] * np.abs(x))[m]) / np.linalg.norm(b[m])
            print("%s solve: reported - true = %.3e, rounding bound of the two evaluations %.3e" % (name, c[-1] - rr, bound))
            assert abs(c[-1] - rr) <= bound + 1e-9 * rr
        ref.close()
        s.close()


def test_set_after_the_switch_rebuilds_the_float_copy(capi, capfd):
    """cedar_amd_solver_set("A") on the switched level 0: the bits of a fresh handle built on that A and switched, and of
    a plain FP64 handle on the rounded products; an A with an entry of 1e39 is reported and level 0 runs FP64 again"""
    so, b, r = solver_problem("dd")
    r = r[0]
    a_new = rt(so * pb.uniform(so.shape, 761, 0.97, 1.03))
    s = capi.Solver(so, **V11)
    round_products(s)
    n = s.use_fp32_operator_all(1)
    assert n == smoothed(s)
    z_old = np.zeros_like(r)
    s.precondition(z_old, r)
    s.set_array(0, "A", a_new)
    fresh = capi.Solver(so, **V11)
    round_products(fresh, a0=a_new)
    assert fresh.use_fp32_operator_all(1) == n
    plain = capi.Solver(so, **V11)
    round_products(plain, a0=a_new)
    z, z_fresh, z_plain = np.zeros_like(r), np.zeros_like(r), np.zeros_like(r)
    s.precondition(z, r)
    fresh.precondition(z_fresh, r)
    plain.precondition(z_plain, r)
    assert same_bits(z, z_fresh) and same_bits(z, z_plain) and not np.array_equal(z, z_old)
    # overflow: level 0 goes back to FP64 and reads the new array as it is
    big = a_new.copy()
    big[1, 5, 6, 7] = 1e39
    capfd.readouterr()
    s.set_array(0, "A", big)
    assert "overflows single precision" in capfd.readouterr().err
    assert s.fp32_levels() == n - 1
    plain.set_array(0, "A", big)
    s.precondition(z, r)
    plain.precondition(z_plain, r)
    assert same_bits(z, z_plain)
    for h in (s, fresh, plain):
        h.close()


def test_refusals_leave_the_handle_as_it_was(capi, capfd):
    """NULL handle, 2D handle, ibc != 0, plane relaxation, min_rows = -1, an overflowing entry: -1, a message,
    fp32_levels() == 0 and the next cycle's bits unchanged"""
    import cases
    so3, b3 = pb.poisson3(17, 17, 17), pb.rhs3(17, 17, 17)

    def refused(s, text, b, min_rows=1):
        def run():
            x = np.zeros_like(b)
            return [s.solve(b, x), x]
        before = run()
        capfd.readouterr()
        rc = s.use_fp32_operator_all(min_rows)
        err = capfd.readouterr().err
        assert rc == -1 and "cedar_amd_solver_use_fp32_operator_all" in err and text in err, (text, err)
        assert s.fp32_levels() == 0
        assert all(same_bits(a, c) for a, c in zip(before, run())), text
        s.close()

    refused(capi.Solver(pb.varcoef9(40, 30), max_iter=3), "2D", pb.rhs2(40, 30))
    mk_op, mk_rhs, st = cases.SOLVES_PER3["perrand27_y_24x32x20_v21"]
    refused(capi.Solver(mk_op(), max_iter=3, **st), "periodic", mk_rhs())
    refused(capi.Solver(so3, relax="plane-xy", max_iter=2), "plane relaxation", b3)
    refused(capi.Solver(so3, max_iter=3, **V11), "min_rows", b3, min_rows=-1)
    refused(capi.Solver(so3, max_rhs=4, max_iter=3, **V11), "min_rows", b3, min_rows=-1)
    big = so3.copy()
    big[1, 9, 9, 9] = 1e39
    refused(capi.Solver(big, max_iter=1, **V11), "overflows single precision", b3)
    capfd.readouterr()
    assert capi.lib.cedar_amd_solver_use_fp32_operator_all(None, 1) == -1
    assert "NULL solver handle" in capfd.readouterr().err
