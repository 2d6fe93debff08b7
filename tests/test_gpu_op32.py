"""The 27-point operator of the cycle kept in single precision (cedar_amd_solver_use_fp32_operator, the float view of
relax3d.hip / relax3d_psum.hip).

Promoting a float to double is exact, so a kernel that reads the float copy and promotes on load does the FP64 kernel's
arithmetic on the operator rounded to float: sections 1, 2 and 4 compare bit patterns, no tolerance.  Section 3 runs
the real (unrounded) operator, where the switched handle differs from the FP64 one by a 6e-8 relative perturbation of
the preconditioner, and checks what that may and may not move.

Measured on an MI355X (section 3, tol 1e-10, V(1,1); FP64 handle / switched handle):
  40x33x50:  pcg 8 / 8 iterations, true relative residual 3.937e-11 / 3.937e-11;  solve 10 / 10 cycles
  65^3:      pcg 8 / 8 iterations, true relative residual 8.495e-11 / 8.495e-11;  solve 10 / 10 cycles
"""
import ctypes as C
import functools

import numpy as np
import pytest

import cases
import problems as pb

pytestmark = pytest.mark.gpu


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
# nx x ny x nz: every launcher width (64 / 128 / 256 / 512 lanes) on either side of its step, the float row padding
# (II = 32: no pad; II = 33: 31 pad floats), an odd last pair, and 37x18x11: at least four runs at frun 2 and 4 with a
# short last run (nF = 9)
SHAPES = [(30, 9, 6), (31, 9, 6), (61, 16, 5), (127, 9, 6), (129, 9, 6), (257, 8, 5), (513, 8, 5), (40, 33, 50), (37, 18, 11)]


@functools.lru_cache(maxsize=None)
def kernel_problem(shape):
    nx, ny, nz = shape
    g = (nz + 2, ny + 2, nx + 2)
    so = pb.random_op(g, 14, 141, zero_ghost=False)
    qf, q0 = pb.uniform(g, 142, -1, 1), pb.uniform(g, 143, -1, 1)
    sor = np.zeros((2,) + g)
    from pyoracle import Oracle
    Oracle().setup_recip3(so, sor)
    for a in (so, qf, q0, sor):
        a.setflags(write=False)
    return so, qf, q0, sor


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_relax_reference_order_is_the_fp64_sweep_on_the_rounded_operator(K, monkeypatch, shape):
    """cedar_amd_relax3_gs_op32(frun = 0) against BMG3_SymStd_relax_GS on (rt(so), rt(sor)): both directions, three
    sweeps in a row, every element of q (ghost cells included) with == on the bit patterns.  CEDAR_AMD_FRUN unset (row
    kernels at these sizes) and 2 (the plane-fused kernel wherever a plane has four runs)."""
    so, qf, q0, sor = kernel_problem(shape)
    so_r, sor_r = rt(so), rt(sor)
    assert not np.array_equal(so_r, so)
    for frun_env in (None, "2"):
        if frun_env is None:
            monkeypatch.delenv("CEDAR_AMD_FRUN", raising=False)
        else:
            monkeypatch.setenv("CEDAR_AMD_FRUN", frun_env)
        for ud in (0, 1):
            want, got = q0.copy(), q0.copy()
            for sweep in range(3):
                K.relax3(so_r, qf, want, sor_r, ud)
                assert K.relax3_op32(so, qf, got, sor, ud, 0) == 0
                assert same_bits(got, want), (shape, frun_env, ud, sweep, np.max(np.abs(got - want)))
            assert not np.array_equal(got, q0)


@pytest.mark.parametrize("frun", [2, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_relax_partial_sums_are_the_fp64_partial_sum_sweep_on_the_rounded_operator(K, monkeypatch, shape, frun):
    """cedar_amd_relax3_gs_op32(frun) against cedar_amd_relax3_gs_psum on the rounded arrays with the same run length
    (CEDAR_AMD_FRUN): bit for bit, both directions, three sweeps; where the level cannot take partial sums (fewer than
    four runs, rows above 512 points) both fall back to the reference order and still agree"""
    so, qf, q0, sor = kernel_problem(shape)
    so_r, sor_r = rt(so), rt(sor)
    monkeypatch.setenv("CEDAR_AMD_FRUN", str(frun))
    nx, ny, nz = shape
    took_want = 1 if (ny >= 4 * frun and (nx + 1) // 2 <= 256) else 0
    for ud in (0, 1):
        want, got = q0.copy(), q0.copy()
        for sweep in range(3):
            assert K.relax3_psum(so_r, qf, want, sor_r, ud) == took_want
            assert K.relax3_op32(so, qf, got, sor, ud, frun) == took_want
            assert same_bits(got, want), (shape, frun, ud, sweep, np.max(np.abs(got - want)))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_residual_is_the_fp64_residual_on_the_rounded_operator(K, shape):
    """cedar_amd_residual3_op32 against BMG3_SymStd_residual on rt(so): every element of res, ghost cells untouched"""
    so, qf, q0, sor = kernel_problem(shape)
    sentinel = pb.uniform(q0.shape, 144, -1, 1)
    want, got = sentinel.copy(), sentinel.copy()
    K.residual3(rt(so), qf, q0, want)
    assert K.residual3_op32(so, qf, q0, got) == 0
    assert same_bits(got, want), (shape, np.max(np.abs(got - want)))
    m = ~pb.interior_mask(q0.shape)
    assert same_bits(got[m], sentinel[m]) and not np.array_equal(got, sentinel)


# ---------------------------------------------------------------- 2 - 4. the solver
SOLVER_CASES = ["fe27_40x33x50_v21", "fe27_65_v21"]
V11 = dict(relax="point", nrelax_pre=1, nrelax_post=1)


@functools.lru_cache(maxsize=None)
def solver_problem(name):
    mk_op, mk_rhs, _ = cases.SOLVES[name]
    so, b = mk_op(), mk_rhs()
    r = pb.uniform(b.shape, 151, -1, 1) * pb.interior_mask(b.shape)
    for a in (so, b, r):
        a.setflags(write=False)
    return so, b, r


def smoothed27(s):
    """levels that are smoothed (all but the coarsest) and hold a 27-point operator"""
    return [l for l in range(s.nlevels() - 1) if s.array(l, "A").shape[0] == 14]


def round_products(s, a0=None):
    """replace A and SOR0 of every level by their float-rounded values (a0: level 0's A instead of what it holds)"""
    for l in range(s.nlevels()):
        A = s.array(l, "A") if (l or a0 is None) else a0
        s.set_array(l, "A", rt(A))
        s.set_array(l, "SOR0", rt(s.array(l, "SOR0")))


def outputs(s, b, r, capi, with_pcg=True):
    """what sections 2 and 4 compare: precondition, pcg (history, iterate), solve (history)"""
    out = {}
    if with_pcg:
        z = np.zeros_like(r)
        s.precondition(z, r)
        out["z"] = z
        x = np.zeros_like(b)
        out["pcg_hist"] = s.pcg(b, x, max_iter=30, tol=1e-10)
        out["pcg_x"] = x
    x = np.zeros_like(b)
    out["solve_hist"] = s.solve(b, x)
    return out


# Tolerance of the solves in the test below.  Rounding SOR0 by itself makes it differ from the reciprocal of the rounded
# diagonal by a relative 2^-24 = 6e-8, so the sweep's fixed point is no longer the solution of A: the plain solve of the
# FP64 handle stagnates at a relative residual of the order 6e-8 * n^2 (the diagonal against the operator on a smooth
# error; 1e-4 and 2.5e-4 at n = 40 and 65), while the switched handle's defect-correction form does not.  Cycle counts
# are comparable above that level: 1e-3.
SOLVE_TOL = 1e-3


@pytest.mark.parametrize("psum", ["0", "1"])
@pytest.mark.parametrize("name", SOLVER_CASES, ids=str)
def test_cycle_on_rounded_products_is_bit_identical(capi, monkeypatch, name, psum):
    """two handles whose A and SOR0 are float-representable on every level; one switches every smoothed 27-point
    level.  precondition, the pcg history / iterate / count and the solve cycle count must not differ in one bit --
    reference order (CEDAR_AMD_PSUM=0) and partial sums with runs of two rows; V-cycles, and F-cycles in solve; once with
    min_rows = level 0's ny, so that only level 0 switches."""
    so, b, r = solver_problem(name)
    monkeypatch.setenv("CEDAR_AMD_PSUM", psum)
    if psum == "1":
        monkeypatch.setenv("CEDAR_AMD_FRUN", "2")
    else:
        monkeypatch.delenv("CEDAR_AMD_FRUN", raising=False)
    ny0 = so.shape[2] - 2
    for kw, min_rows in ((V11, 1), (V11, ny0), (dict(relax="point", nrelax_pre=2, nrelax_post=1, cycle="f"), 1)):
        vcyc = kw.get("cycle", "v") == "v"
        maxit = 25 if vcyc else 4
        ref, s = capi.Solver(so, max_iter=maxit, tol=SOLVE_TOL, **kw), capi.Solver(so, max_iter=maxit, tol=SOLVE_TOL, **kw)
        round_products(ref)
        round_products(s)
        want_levels = [l for l in smoothed27(s) if s.dims(l)[1] >= min_rows]
        assert len(want_levels) >= (1 if min_rows > 1 else 2)
        assert s.fp32_levels() == 0
        assert s.use_fp32_operator(min_rows) == len(want_levels) == s.fp32_levels()
        assert s.use_fp32_operator(min_rows) == len(want_levels)  # idempotent
        want, got = outputs(ref, b, r, capi, vcyc), outputs(s, b, r, capi, vcyc)
        if vcyc:
            assert same_bits(got["z"], want["z"]) and np.any(got["z"] != 0), (name, psum, min_rows)
            assert len(got["pcg_hist"]) == len(want["pcg_hist"]) > 2 and same_bits(got["pcg_hist"], want["pcg_hist"])
            assert same_bits(got["pcg_x"], want["pcg_x"])
            # defect correction computes the same iterates in another order of additions: the count, not the bits
            assert len(got["solve_hist"]) == len(want["solve_hist"]) > 2
            assert got["solve_hist"][-1] < SOLVE_TOL and want["solve_hist"][-1] < SOLVE_TOL
        else:  # every F-cycle starts from x = 0: the plain form is kept, and the histories are identical
            assert len(got["solve_hist"]) == len(want["solve_hist"]) and same_bits(got["solve_hist"], want["solve_hist"])
        ref.close()
        s.close()


def true_relres(K, so, b, x):
    ax = np.zeros_like(b)
    K.matvec3(so, x, ax)
    m = pb.interior_mask(b.shape)
    return np.linalg.norm((b - ax)[m]) / np.linalg.norm(b[m])


@pytest.mark.parametrize("name", SOLVER_CASES, ids=str)
def test_real_operator_converges_to_the_fp64_solution(capi, K, name):
    """the unrounded operator.  The switched handle's preconditioner differs from the FP64 one (the float path is taken),
    by a relative 6e-8: pcg to 1e-10 needs at most one iteration more (a count moves only when a residual sits at the
    threshold) and reaches a true FP64 residual within a factor two of max(tol, the FP64 handle's); solve to 1e-10 meets
    the tolerance in at most one cycle more -- without the defect-correction form it would stagnate near 6e-8 * cond."""
    so, b, r = solver_problem(name)
    tol = 1e-10
    ref, s = capi.Solver(so, max_iter=30, tol=tol, **V11), capi.Solver(so, max_iter=30, tol=tol, **V11)
    assert s.use_fp32_operator(1) == len(smoothed27(s)) >= 2
    z_ref, z = np.zeros_like(r), np.zeros_like(r)
    ref.precondition(z_ref, r)
    s.precondition(z, r)
    assert not np.array_equal(z, z_ref)
    x_ref, x = np.zeros_like(b), np.zeros_like(b)
    h_ref, h = ref.pcg(b, x_ref, max_iter=50, tol=tol), s.pcg(b, x, max_iter=50, tol=tol)
    rr_ref, rr = true_relres(K, so, b, x_ref), true_relres(K, so, b, x)
    print("%s pcg: iterations fp64 %d, fp32-operator %d; true relative residual %.3e, %.3e" % (name, len(h_ref) - 1, len(h) - 1, rr_ref, rr))
    assert h_ref[-1] < tol and h[-1] < tol
    assert len(h) - 1 <= len(h_ref) - 1 + 1
    assert rr <= 2 * max(tol, rr_ref)
    x_ref, x = np.zeros_like(b), np.zeros_like(b)
    c_ref, c = ref.solve(b, x_ref), s.solve(b, x)
    print("%s solve: cycles fp64 %d, fp32-operator %d; last relative residual %.3e, %.3e" % (name, len(c_ref) - 1, len(c) - 1, c_ref[-1], c[-1]))
    assert c_ref[-1] < tol and c[-1] < tol
    assert len(c) - 1 <= len(c_ref) - 1 + 1
    assert true_relres(K, so, b, x) <= 2 * max(tol, true_relres(K, so, b, x_ref))
    ref.close()
    s.close()


def test_set_after_the_switch_rebuilds_the_float_copy(capi):
    """cedar_amd_solver_set("A") on a switched level: precondition equals, bit for bit, a fresh handle prepared with
    that A before its switch"""
    so, b, r = solver_problem("fe27_40x33x50_v21")
    a_new = rt(so * pb.uniform(so.shape, 161, 0.97, 1.03))
    s = capi.Solver(so, **V11)
    round_products(s)
    assert s.use_fp32_operator(1) >= 2
    z_old = np.zeros_like(r)
    s.precondition(z_old, r)
    s.set_array(0, "A", a_new)
    fresh = capi.Solver(so, **V11)
    round_products(fresh, a0=a_new)
    fresh.use_fp32_operator(1)
    plain = capi.Solver(so, **V11)
    round_products(plain, a0=a_new)
    z, z_fresh, z_plain = np.zeros_like(r), np.zeros_like(r), np.zeros_like(r)
    s.precondition(z, r)
    fresh.precondition(z_fresh, r)
    plain.precondition(z_plain, r)
    assert same_bits(z, z_fresh) and same_bits(z, z_plain) and not np.array_equal(z, z_old)
    for h in (s, fresh, plain):
        h.close()


# ---------------------------------------------------------------- 5. refusals
def test_refusals_leave_the_handle_as_it_was(capi, capfd):
    """argument checks that return before any launch: -1, a print_error message, fp32_levels() == 0, and the next
    precondition / solve has the bits from before the call"""
    so3, b3 = pb.fe3(17, 17, 17), pb.rhs3(17, 17, 17)
    r3 = pb.uniform(b3.shape, 171, -1, 1) * pb.interior_mask(b3.shape)

    def refused(s, text, run):
        before = run(s)
        capfd.readouterr()
        rc = s.use_fp32_operator(1)
        err = capfd.readouterr().err
        assert rc == -1 and "cedar_amd_solver_use_fp32_operator" in err and text in err, (text, err)
        assert s.fp32_levels() == 0
        after = run(s)
        assert all(same_bits(a, c) for a, c in zip(before, after)), text
        s.close()

    def run_solve(b):
        def run(s):
            x = np.zeros_like(b)
            return [s.solve(b, x), x]
        return run

    def run_precondition(s):
        z = np.zeros_like(r3)
        s.precondition(z, r3)
        return [z]

    refused(capi.Solver(pb.varcoef9(40, 30), max_iter=3), "2D", run_solve(pb.rhs2(40, 30)))
    mk_op, mk_rhs, st = cases.SOLVES_PER3["perrand27_y_24x32x20_v21"]
    refused(capi.Solver(mk_op(), max_iter=3, **st), "periodic", run_solve(mk_rhs()))
    refused(capi.Solver(so3, relax="plane-xy", max_iter=2), "plane relaxation", run_solve(b3))
    refused(capi.Solver(so3, max_rhs=4, **V11), "cedar_amd_solver_create_many", run_precondition)
    big = so3.copy()
    big[3, 9, 9, 9] = 1e39
    refused(capi.Solver(big, **V11), "overflows single precision", run_precondition)
    # the NULL handle
    capfd.readouterr()
    capi.lib.cedar_amd_solver_use_fp32_operator.argtypes = [C.c_void_p, C.c_int]
    assert capi.lib.cedar_amd_solver_use_fp32_operator(None, 1) == -1
    assert "NULL solver handle" in capfd.readouterr().err
    assert capi.lib.cedar_amd_solver_fp32_levels(None) == 0


def test_kernel_entry_points_refuse_an_overflowing_entry(K, capfd):
    so, qf, q0, sor = kernel_problem((30, 9, 6))
    big = so.copy()
    big[5, 3, 4, 7] = -1e39
    got = q0.copy()
    capfd.readouterr()
    assert K.relax3_op32(big, qf, got, sor, 1, 0) == -1
    assert "overflows single precision" in capfd.readouterr().err and same_bits(got, q0)
    res = q0.copy()
    assert K.residual3_op32(big, qf, q0, res) == -1
    assert "overflows single precision" in capfd.readouterr().err and same_bits(res, q0)
