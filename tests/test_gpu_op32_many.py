"""The single-precision 27-point operator on a batch of right-hand sides (cedar_amd_solver_use_fp32_operator_many, the
float view of many3d.hip).

Promoting a float to double is exact, so a batched kernel that reads the float copy and promotes on load does the FP64
batched kernel's arithmetic on the operator rounded to float: sections 1, 2 and 4 compare bit patterns, no tolerance.
Section 3 runs the real (unrounded) operator with the margins test_gpu_op32.py uses for the single-vector switch --
section 2 shows that item m of the batch has that call's bits, so the same margins hold per item.

Measured on an MI355X (section 3, tol 1e-10, V(1,1), three right-hand sides; FP64 batch handle / switched batch handle):
  40x33x50:  pcg_many 8 / 8 iterations on every item, true relative residuals 3.937e-11, 7.971e-12, 7.841e-12 on both;
             solve_many 10, 9, 9 / 10, 9, 9 cycles
  65^3:      pcg_many 8 / 8 iterations on every item, true relative residuals 8.495e-11, 1.472e-11, 1.221e-11 on both;
             solve_many 10, 9, 9 / 10, 9, 9 cycles
"""
import ctypes as C
import functools

import numpy as np
import pytest

import cases
import problems as pb

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
# nx x ny x nz: the float row padding (II = 32: none; II = 33: 31 pad floats and an odd last pair), either side of every
# launcher step (sweep 64 / 128 / 256 / 512 lanes; residual 64 / 128 / 256 lanes, 513: two trips of 256), and exactly 512
# pairs, the last shape served
SHAPES = [(30, 9, 6), (31, 9, 6), (127, 9, 6), (129, 9, 6), (255, 8, 5), (257, 8, 5), (513, 8, 5), (1024, 4, 3)]
NRHS = [1, 3, 5]  # three items or more: the two LDS rows xch[m & 1] are reused


@functools.lru_cache(maxsize=None)
def kernel_problem(shape):
    nx, ny, nz = shape
    g = (nz + 2, ny + 2, nx + 2)
    so = pb.random_op(g, 14, 241, zero_ghost=False)
    sor = np.zeros((2,) + g)
    from pyoracle import Oracle
    Oracle().setup_recip3(so, sor)
    qf = np.stack([pb.uniform(g, 242 + 17 * m, -1, 1) for m in range(max(NRHS))])
    q0 = np.stack([pb.uniform(g, 243 + 17 * m, -1, 1) for m in range(max(NRHS))])
    for a in (so, qf, q0, sor):
        a.setflags(write=False)
    return so, qf, q0, sor


@pytest.mark.parametrize("nrhs", NRHS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_relax_many_is_the_fp64_batched_sweep_on_the_rounded_operator(K, shape, nrhs):
    """cedar_amd_relax3_gs_many_op32 on (so, sor) against cedar_amd_relax3_gs_many on (rt(so), rt(sor)): both
    directions, three sweeps in a row, every element of every item (ghost cells included); and item m against the
    single-vector cedar_amd_relax3_gs_op32(frun = 0) on item m alone"""
    so, qf, q0, sor = kernel_problem(shape)
    so_r, sor_r = rt(so), rt(sor)
    assert not np.array_equal(so_r, so)
    qf, q0 = np.ascontiguousarray(qf[:nrhs]), np.ascontiguousarray(q0[:nrhs])
    for ud in (DOWN, UP):
        want, got = q0.copy(), q0.copy()
        single = [q0[m].copy() for m in range(nrhs)]
        for sweep in range(3):
            K.relax3_many(so_r, qf, want, sor_r, ud)
            assert K.relax3_many_op32(so, qf, got, sor, ud) == 0
            assert same_bits(got, want), (shape, nrhs, ud, sweep, np.max(np.abs(got - want)))
            for m in range(nrhs):
                assert K.relax3_op32(so, qf[m], single[m], sor, ud, 0) == 0
                assert same_bits(got[m], single[m]), (shape, nrhs, ud, sweep, m)
        assert not np.array_equal(got, q0)


@pytest.mark.parametrize("nrhs", NRHS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_residual_many_is_the_fp64_batched_residual_on_the_rounded_operator(K, shape, nrhs):
    """cedar_amd_residual3_many_op32 against cedar_amd_residual3_many on rt(so) and, per item, against
    cedar_amd_residual3_op32: every element of res, ghost cells untouched"""
    so, qf, q0, sor = kernel_problem(shape)
    qf, q0 = np.ascontiguousarray(qf[:nrhs]), np.ascontiguousarray(q0[:nrhs])
    sentinel = np.stack([pb.uniform(q0.shape[1:], 244 + m, -1, 1) for m in range(nrhs)])
    want, got = sentinel.copy(), sentinel.copy()
    K.residual3_many(rt(so), qf, q0, want)
    assert K.residual3_many_op32(so, qf, q0, got) == 0
    assert same_bits(got, want), (shape, nrhs, np.max(np.abs(got - want)))
    ghost = ~pb.interior_mask(q0.shape[1:])
    for m in range(nrhs):
        one = sentinel[m].copy()
        assert K.residual3_op32(so, qf[m], q0[m], one) == 0
        assert same_bits(got[m], one), (shape, nrhs, m)
        assert same_bits(got[m][ghost], sentinel[m][ghost]) and not np.array_equal(got[m], sentinel[m])


@pytest.mark.parametrize("shape", [(129, 9, 6), (513, 8, 5)], ids=str)
def test_items_of_the_float_batch_do_not_see_each_other(K, shape):
    """item 1's q and qf replaced: items 0 and 2 keep their bits, sweep (both directions) and residual"""
    so, qf, q0, sor = kernel_problem(shape)
    qf, q0 = np.ascontiguousarray(qf[:3]), np.ascontiguousarray(q0[:3])
    qf2, q2 = qf.copy(), q0.copy()
    qf2[1] = pb.uniform(qf.shape[1:], 251, -1e3, 1e3)
    q2[1] = pb.uniform(qf.shape[1:], 252, -1e3, 1e3)

    def run(f, q):
        out = []
        for ud in (DOWN, UP):
            a = q.copy()
            assert K.relax3_many_op32(so, f, a, sor, ud) == 0
            out.append(a)
        r = np.zeros_like(q)
        assert K.residual3_many_op32(so, f, q, r) == 0
        return out + [r]

    for a, c in zip(run(qf, q0), run(qf2, q2)):
        assert same_bits(a[0], c[0]) and same_bits(a[2], c[2]) and not np.array_equal(a[1], c[1])


# ---------------------------------------------------------------- 2 - 4. the solver
SOLVER_CASES = ["fe27_40x33x50_v21", "fe27_65_v21"]
V11 = dict(relax="point", nrelax_pre=1, nrelax_post=1)
NITEMS = 3


@functools.lru_cache(maxsize=None)
def solver_problem(name):
    """operator, NITEMS distinct right-hand sides, NITEMS random interior vectors"""
    mk_op, mk_rhs, _ = cases.SOLVES[name]
    so, b0 = mk_op(), mk_rhs()
    m = pb.interior_mask(b0.shape)
    b = np.stack([b0] + [pb.uniform(b0.shape, 4242 + t, -1, 1) * m * np.max(np.abs(b0)) for t in range(1, NITEMS)])
    r = np.stack([pb.uniform(b0.shape, 261 + t, -1, 1) * m for t in range(NITEMS)])
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


def batch_outputs(s, b, r):
    """vcycle_many on random x, b; pcg_many (x, history rows, counts); solve_many (x, rel rows)"""
    out = {}
    x = r.copy()
    s.vcycle_many(x, b)
    out["cycle"] = x
    x = np.zeros_like(b)
    hist, iters = s.pcg_many(b, x, max_iter=30, tol=1e-10)
    out["pcg_x"], out["pcg_hist"], out["pcg_iters"] = x, hist, iters
    x = np.zeros_like(b)
    rel, _ = s.solve_many(b, x)
    out["solve_x"], out["solve_rel"] = x, rel
    return out


SOLVE_CYCLES = 4  # solve / solve_many with tol = 0: exactly this many cycles, every rel entry compared


@pytest.mark.parametrize("name", SOLVER_CASES, ids=str)
def test_batched_cycle_on_rounded_products_is_bit_identical(capi, monkeypatch, name):
    """two batch handles whose A and SOR0 are float-representable on every level; one switches.  vcycle_many, pcg_many
    (x, history rows, counts) and solve_many must not differ in one bit -- with every smoothed 27-point level switched
    and with level 0 alone.  Under CEDAR_AMD_PSUM=0 item m of each equals the single-vector switched handle on item m
    alone: the cycle, pcg, and solve (x and every rel entry: both are the same defect-correction recurrence)."""
    so, b, r = solver_problem(name)
    monkeypatch.setenv("CEDAR_AMD_PSUM", "0")
    monkeypatch.delenv("CEDAR_AMD_FRUN", raising=False)
    kw = dict(max_iter=SOLVE_CYCLES, tol=0.0, **V11)
    ny0 = so.shape[2] - 2
    for min_rows in (1, ny0):
        ref, s = capi.Solver(so, max_rhs=4, **kw), capi.Solver(so, max_rhs=4, **kw)
        assert s.max_rhs() == 4
        round_products(ref)
        round_products(s)
        want_levels = [l for l in smoothed27(s) if s.dims(l)[1] >= min_rows]
        assert len(want_levels) >= (1 if min_rows > 1 else 2)
        assert s.fp32_levels() == 0
        assert s.use_fp32_operator_many(min_rows) == len(want_levels) == s.fp32_levels()
        assert s.use_fp32_operator_many(min_rows) == len(want_levels)  # idempotent
        want, got = batch_outputs(ref, b, r), batch_outputs(s, b, r)
        ref.close()
        s.close()
        assert same_bits(got["cycle"], want["cycle"]) and not np.array_equal(got["cycle"], r), (name, min_rows)
        assert got["pcg_iters"] == want["pcg_iters"] and min(got["pcg_iters"]) > 2
        assert same_bits(got["pcg_x"], want["pcg_x"])
        for m in range(NITEMS):
            assert same_bits(got["pcg_hist"][m], want["pcg_hist"][m]), (name, min_rows, m)
            # the plain solve_many of the FP64 handle adds in another order than defect correction: same cycle count
            assert len(got["solve_rel"][m]) == len(want["solve_rel"][m]) == SOLVE_CYCLES + 1
        one = capi.Solver(so, **kw)
        round_products(one)
        assert one.use_fp32_operator(min_rows) == len(want_levels)
        for m in range(NITEMS):
            x = r[m].copy()
            one.vcycle(x, b[m])
            assert same_bits(got["cycle"][m], x), (name, min_rows, m)
            x = np.zeros_like(b[m])
            h = one.pcg(b[m], x, max_iter=30, tol=1e-10)
            assert same_bits(got["pcg_hist"][m], h) and same_bits(got["pcg_x"][m], x), (name, min_rows, m)
            x = np.zeros_like(b[m])
            rel = one.solve(b[m], x)
            assert len(rel) == SOLVE_CYCLES + 1 and same_bits(got["solve_rel"][m], rel), (name, min_rows, m, got["solve_rel"][m], rel)
            assert same_bits(got["solve_x"][m], x), (name, min_rows, m)
        one.close()


@pytest.mark.parametrize("name", SOLVER_CASES, ids=str)
def test_one_item_on_a_switched_batch_handle_is_the_plain_switched_handle(capi, monkeypatch, name):
    """default environment (partial-sum sweeps where the level takes them): the single-vector entry points and
    nrhs == 1 of the batched ones run the single-vector float kernels"""
    so, b, r = solver_problem(name)
    monkeypatch.delenv("CEDAR_AMD_PSUM", raising=False)
    monkeypatch.delenv("CEDAR_AMD_FRUN", raising=False)
    s, one = capi.Solver(so, max_rhs=4, **V11), capi.Solver(so, **V11)
    assert s.use_fp32_operator_many(1) == one.use_fp32_operator(1) >= 2
    z, z1 = np.zeros_like(r[0]), np.zeros_like(r[0])
    s.precondition(z, r[0])
    one.precondition(z1, r[0])
    assert same_bits(z, z1) and np.any(z != 0)
    x, x1 = np.zeros_like(b[0]), np.zeros_like(b[0])
    h, h1 = s.pcg(b[0], x, max_iter=30, tol=1e-10), one.pcg(b[0], x1, max_iter=30, tol=1e-10)
    assert same_bits(h, h1) and same_bits(x, x1) and len(h) > 2
    xm = np.zeros_like(b[:1])
    hm, _ = s.pcg_many(b[:1], xm, max_iter=30, tol=1e-10)
    assert same_bits(hm[0], h1) and same_bits(xm[0], x1)
    xm = r[:1].copy()
    x1 = r[0].copy()
    s.vcycle_many(xm, b[:1])
    one.vcycle(x1, b[0])
    assert same_bits(xm[0], x1)
    s.close()
    one.close()


# ---------------------------------------------------------------- 3. the real (unrounded) operator
def true_relres(K, so, b, x):
    ax = np.zeros_like(b)
    K.matvec3(so, x, ax)
    m = pb.interior_mask(b.shape)
    return np.linalg.norm((b - ax)[m]) / np.linalg.norm(b[m])


@pytest.mark.parametrize("name", SOLVER_CASES, ids=str)
def test_real_operator_converges_to_the_fp64_solution_per_item(capi, K, name):
    """an FP64 batch handle against a switched one, tol 1e-10: the batched cycle differs (the float path is taken);
    pcg_many meets tol on every item in at most one iteration more, with a true FP64 relative residual (matvec3 on the
    operator given) of at most 2 max(tol, the FP64 handle's); solve_many meets tol in at most one cycle more."""
    so, b, r = solver_problem(name)
    tol = 1e-10
    kw = dict(max_iter=30, tol=tol, max_rhs=4, **V11)
    ref, s = capi.Solver(so, **kw), capi.Solver(so, **kw)
    assert s.use_fp32_operator_many(1) == len(smoothed27(s)) >= 2
    z_ref, z = r.copy(), r.copy()
    ref.vcycle_many(z_ref, b)
    s.vcycle_many(z, b)
    assert not np.array_equal(z, z_ref)
    x_ref, x = np.zeros_like(b), np.zeros_like(b)
    (h_ref, it_ref), (h, it) = ref.pcg_many(b, x_ref, max_iter=50, tol=tol), s.pcg_many(b, x, max_iter=50, tol=tol)
    for m in range(NITEMS):
        rr_ref, rr = true_relres(K, so, b[m], x_ref[m]), true_relres(K, so, b[m], x[m])
        print("%s item %d pcg_many: iterations fp64 %d, fp32-operator %d; true relative residual %.3e, %.3e"
              % (name, m, it_ref[m], it[m], rr_ref, rr))
        assert h_ref[m][-1] < tol and h[m][-1] < tol
        assert it[m] <= it_ref[m] + 1
        assert rr <= 2 * max(tol, rr_ref)
    x_ref, x = np.zeros_like(b), np.zeros_like(b)
    (c_ref, n_ref), (c, n) = ref.solve_many(b, x_ref), s.solve_many(b, x)
    for m in range(NITEMS):
        print("%s item %d solve_many: cycles fp64 %d, fp32-operator %d; relative residual there %.3e, %.3e"
              % (name, m, n_ref[m], n[m], c_ref[m][n_ref[m]], c[m][n[m]]))
        assert c_ref[m][n_ref[m]] < tol and c[m][n[m]] < tol
        assert n[m] <= n_ref[m] + 1
    ref.close()
    s.close()


# ---------------------------------------------------------------- 4. set after the switch
def test_set_after_the_switch_rebuilds_the_float_copy_of_a_batch_handle(capi):
    """cedar_amd_solver_set("A") on a switched level of a batch handle: vcycle_many equals, bit for bit, a fresh batch
    handle prepared with that A before its switch"""
    so, b, r = solver_problem("fe27_40x33x50_v21")
    a_new = rt(so * pb.uniform(so.shape, 271, 0.97, 1.03))
    s = capi.Solver(so, max_rhs=4, **V11)
    round_products(s)
    assert s.use_fp32_operator_many(1) >= 2
    x_old = r.copy()
    s.vcycle_many(x_old, b)
    s.set_array(0, "A", a_new)
    fresh = capi.Solver(so, max_rhs=4, **V11)
    round_products(fresh, a0=a_new)
    assert fresh.use_fp32_operator_many(1) == s.fp32_levels()
    x, x_fresh = r.copy(), r.copy()
    s.vcycle_many(x, b)
    fresh.vcycle_many(x_fresh, b)
    assert same_bits(x, x_fresh) and not np.array_equal(x, x_old)
    s.close()
    fresh.close()


# ---------------------------------------------------------------- 5. refusals and forwarding
def test_one_right_hand_side_forwards_to_the_single_call(capi):
    so, b, r = solver_problem("fe27_40x33x50_v21")
    a, c = capi.Solver(so, **V11), capi.Solver(so, **V11)
    assert a.max_rhs() == 1
    n = c.use_fp32_operator(1)
    assert a.use_fp32_operator_many(1) == n == a.fp32_levels() >= 2
    assert a.use_fp32_operator_many(1) == n
    z, z1 = np.zeros_like(r[0]), np.zeros_like(r[0])
    a.precondition(z, r[0])
    c.precondition(z1, r[0])
    assert same_bits(z, z1) and np.any(z != 0)
    a.close()
    c.close()


def test_refusals_leave_the_batch_handle_as_it_was(capi, capfd):
    """-1, a print_error message, fp32_levels() == 0, and the next cycle has the bits from before the call"""
    so3, b3 = pb.fe3(17, 17, 17), pb.rhs3(17, 17, 17)
    m3 = pb.interior_mask(b3.shape)
    bm = np.stack([b3, pb.uniform(b3.shape, 281, -1, 1) * m3])
    xm = np.stack([pb.uniform(b3.shape, 282 + t, -1, 1) for t in range(2)])

    def refused(s, text, run, min_rows=1):
        before = run(s)
        capfd.readouterr()
        rc = s.use_fp32_operator_many(min_rows)
        err = capfd.readouterr().err
        assert rc == -1 and "cedar_amd_solver_use_fp32_operator" in err and text in err, (text, err)
        assert s.fp32_levels() == 0
        after = run(s)
        assert all(same_bits(a, c) for a, c in zip(before, after)), text
        s.close()

    def run_cycle_many(x0, b):
        def run(s):
            x = x0.copy()
            s.vcycle_many(x, b)
            return [x]
        return run

    def run_solve(b):
        def run(s):
            x = np.zeros_like(b)
            return [s.solve(b, x), x]
        return run

    so2, b2 = pb.varcoef9(40, 30), pb.rhs2(40, 30)
    s2 = capi.Solver(so2, max_iter=3, max_rhs=4)
    assert s2.max_rhs() == 4
    refused(s2, "2D", run_cycle_many(np.stack([b2 * 0.5, b2 * 0.25]), np.stack([b2, 2 * b2])))
    # a periodic or plane-relaxation handle holds one right-hand side whatever was asked for: the forwarded call refuses
    mk_op, mk_rhs, st = cases.SOLVES_PER3["perrand27_y_24x32x20_v21"]
    sp = capi.Solver(mk_op(), max_iter=3, max_rhs=4, **st)
    assert sp.max_rhs() == 1
    refused(sp, "periodic", run_solve(mk_rhs()))
    spl = capi.Solver(so3, relax="plane-xy", max_iter=2, max_rhs=4)
    assert spl.max_rhs() == 1
    refused(spl, "plane relaxation", run_solve(b3))
    refused(capi.Solver(so3, max_rhs=4, **V11), "min_rows must not be negative", run_cycle_many(xm, bm), min_rows=-1)
    big = so3.copy()
    big[3, 9, 9, 9] = 1e39
    refused(capi.Solver(big, max_rhs=4, **V11), "overflows single precision", run_cycle_many(xm, bm))
    capfd.readouterr()
    capi.lib.cedar_amd_solver_use_fp32_operator_many.argtypes = [C.c_void_p, C.c_int]
    assert capi.lib.cedar_amd_solver_use_fp32_operator_many(None, 1) == -1
    err = capfd.readouterr().err
    assert "NULL solver handle" in err and "cedar_amd_solver_use_fp32_operator_many" in err


def test_kernel_entry_points_refuse(K, capfd):
    """nrhs 0 and 33, a NULL array, rows of 1025 points, an overflowing entry: -1, a message, q / res untouched"""
    so, qf, q0, sor = kernel_problem((30, 9, 6))
    qf, q0 = np.ascontiguousarray(qf[:3]), np.ascontiguousarray(q0[:3])
    big = so.copy()
    big[5, 3, 4, 7] = -1e39
    g_long = (5, 6, 1027)
    so_long, v_long = np.ones((14,) + g_long), np.ones((2,) + g_long)
    sor_long = np.ones((2,) + g_long)

    def check(call, text):
        capfd.readouterr()
        rc, arr, arr0 = call()
        err = capfd.readouterr().err
        assert rc == -1 and "_many_op32" in err and text in err, (text, rc, err)
        assert same_bits(arr, arr0), text

    for nrhs in (0, 33):
        got = q0.copy()
        check(lambda: (K.relax3_many_op32(so, qf, got, sor, UP, nrhs=nrhs), got, q0), "nrhs must be 1 .. 32")
        check(lambda: (K.residual3_many_op32(so, qf, q0, got, nrhs=nrhs), got, q0), "nrhs must be 1 .. 32")
    got = q0.copy()
    check(lambda: (K.relax3_many_op32(so, None, got, sor, UP), got, q0), "NULL")
    check(lambda: (K.residual3_many_op32(None, qf, q0, got), got, q0), "NULL")
    got_long = v_long.copy()
    check(lambda: (K.relax3_many_op32(so_long, v_long, got_long, sor_long, UP), got_long, v_long), "1024 points")
    check(lambda: (K.residual3_many_op32(so_long, v_long, v_long, got_long), got_long, v_long), "1024 points")
    check(lambda: (K.relax3_many_op32(big, qf, got, sor, DOWN), got, q0), "overflows single precision")
    check(lambda: (K.residual3_many_op32(big, qf, q0, got), got, q0), "overflows single precision")
