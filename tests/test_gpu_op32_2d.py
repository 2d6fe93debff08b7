"""The operator of a 2D point-relaxed level kept in single precision (cedar_amd_solver_use_fp32_operator_2d, the float view
of op2f.hip), single vector and batch.

Promoting a float to double is exact, so a kernel that reads the float copy and promotes on load does the FP64 kernel's
arithmetic on the operator rounded to float: sections 1 - 4 and 6 compare bit patterns, no tolerance.  Section 5 runs
the real (unrounded) operator, where the switched handle's preconditioner differs from the FP64 one by a relative 6e-8.

Measured on an MI355X (section 5, tol 1e-10; FP64 handle / handle after use_fp32_operator_2d(1); the true relative
residual is the oracle's matvec on the unrounded operator; the rounding bound of evaluating b - A x twice is 2.2e-13,
1.8e-13 and 2.0e-13 for the three operators):
  varcoef9(150,140)         pcg V(1,1) 8 / 8 iterations, 7.5761e-11 / 7.5761e-11;  fcg V(2,1) 8 / 8, 1.2001e-11 / 1.2001e-11;
                            solve V(2,1) 9 / 9 cycles, 6.9798e-11 / 6.9798e-11
  aniso9(129,70, eps=0.1)   pcg 34 / 34, 7.9950e-11 / 7.9949e-11;  fcg 28 / 28, 5.5840e-11 / 5.5840e-11;
                            solve 101 / 101 cycles, 9.0028e-11 / 9.0028e-11
  poisson2(129,70)          pcg 12 / 12, 3.1548e-11 / 3.1548e-11;  fcg 9 / 9, 6.2475e-11 / 6.2476e-11;
                            solve 14 / 14 cycles, 2.2456e-11 / 2.2455e-11
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
    for v in ("CEDAR_AMD_FRUN2", "CEDAR_AMD_PSUM", "CEDAR_AMD_OP32_MIN_ROWS"):
        monkeypatch.delenv(v, raising=False)


# ---------------------------------------------------------------- 1. kernels, bit for bit
# nx x ny.  The launchers of op2f.hip step as those of relax2d.hip do.  Nine-point sweep: one workgroup per row, a lane per
# pair of points, 64 lanes for up to 64 pairs (ceil(nx / 2)), else 256 lanes walking the row in chunks of 256 pairs with
# one carried value between chunks.  Nine-point residual: 64 lanes below 256 pairs (nx / 2), else 256, lanes loop.  The
# five-point kernels take a point per lane of 256-lane workgroups along the row.  A slot-row of the copy holds nx + 3
# floats (one float of lead), padded to a multiple of 32.
#   (1,1), (2,3)                  one point; rows with one point of a colour
#   (28,9), (29,9), (30,9), (31,9) nx + 3 = 31 .. 34: either side of the float row padding, even and odd row length
#   (127,6), (128,6), (129,6)     64 | 64 | 65 pairs: the 64 -> 256-lane step of the sweep
#   (511,4), (512,4), (513,4)     the residual's 64 -> 256-lane step (255 | 256 pairs); the sweep's second chunk with the
#                                 carried value at 257 pairs (513); the five-point kernels' second and third workgroup
#   (1030,3)                      third chunk, walked downwards for DOWN and upwards for UP
#   (40,5001)                     2500 row workgroups per launch: more than the card holds at once
SHAPES = [(1, 1), (2, 3), (28, 9), (29, 9), (30, 9), (31, 9), (127, 6), (128, 6), (129, 6), (511, 4), (512, 4), (513, 4),
          (1030, 3), (40, 5001)]
# 2. band-fused and partial-sum sweeps: at least 8 runs (ny >= 8 frun) and more than 64 pairs; the odd row counts give a
# short last run, (258,33) a second chunk inside the band walk
BAND_SHAPES = [(130, 16), (130, 17), (131, 19), (258, 33)]
NRHS = [1, 3, 9]


@functools.lru_cache(maxsize=None)
def kernel_problem(shape, nst):
    nx, ny = shape
    g = (ny + 2, nx + 2)
    so = pb.random_op(g, nst, 841 + nst, zero_ghost=False)
    sor = np.zeros((2,) + g)
    from pyoracle import Oracle
    Oracle().setup_recip2(so, sor)
    n = max(NRHS) + 1  # one item beyond the largest batch
    if nx * ny > 100000:
        n = 4
    qf = np.stack([pb.uniform(g, 842 + 17 * m, -1, 1) for m in range(n)])  # non-zero ghost cells
    q0 = np.stack([pb.uniform(g, 843 + 17 * m, -1, 1) for m in range(n)])
    so_r, sor_r = rt(so), rt(sor)
    assert not np.array_equal(so_r, so) and not np.array_equal(sor_r, sor)
    for a in (so, qf, q0, sor, so_r, sor_r):
        a.setflags(write=False)
    return so, qf, q0, sor, so_r, sor_r


@pytest.mark.parametrize("nst", [5, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_relax_is_the_fp64_sweep_on_the_rounded_operator(K, shape, nst):
    """cedar_amd_relax2_gs_op32 on (so, sor) against BMG2_SymStd_relax_GS on (rt(so), rt(sor)): both directions, three
    sweeps in a row, every element of q (ghost cells included) with == on the bit patterns"""
    so, qf, q0, sor, so_r, sor_r = kernel_problem(shape, nst)
    for ud in (DOWN, UP):
        want, got = q0[0].copy(), q0[0].copy()
        for sweep in range(3):
            K.relax2(so_r, qf[0], want, sor_r, ud)
            assert K.relax2_op32(so, qf[0], got, sor, ud) == 0
            assert same_bits(got, want), (shape, nst, ud, sweep, np.max(np.abs(got - want)))
        assert not np.array_equal(got, q0[0])


@pytest.mark.parametrize("nst", [5, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_residual_is_the_fp64_residual_on_the_rounded_operator(K, shape, nst):
    """cedar_amd_residual2_op32 against BMG2_SymStd_residual on rt(so) into a sentinel-filled array: every element of
    res, everything outside the interior untouched"""
    so, qf, q0, sor, so_r, sor_r = kernel_problem(shape, nst)
    sentinel = pb.uniform(q0[0].shape, 844, -1, 1)
    want, got = sentinel.copy(), sentinel.copy()
    K.residual2(so_r, qf[0], q0[0], want)
    assert K.residual2_op32(so, qf[0], q0[0], got) == 0
    assert same_bits(got, want), (shape, nst, np.max(np.abs(got - want)))
    m = ~pb.interior_mask(q0[0].shape)
    assert same_bits(got[m], sentinel[m]) and not np.array_equal(got, sentinel)


# ---------------------------------------------------------------- 2. band-fused and partial-sum sweeps
@pytest.mark.parametrize("shape", BAND_SHAPES, ids=str)
def test_band_fused_sweep_is_the_fp64_one_on_the_rounded_operator(K, monkeypatch, shape):
    """CEDAR_AMD_FRUN2=2: both calls run the band-fused launch plus the rows between runs"""
    monkeypatch.setenv("CEDAR_AMD_FRUN2", "2")
    so, qf, q0, sor, so_r, sor_r = kernel_problem(shape, 5)
    for ud in (DOWN, UP):
        want, got = q0[0].copy(), q0[0].copy()
        for sweep in range(3):
            K.relax2(so_r, qf[0], want, sor_r, ud)
            assert K.relax2_op32(so, qf[0], got, sor, ud) == 0
            assert same_bits(got, want), (shape, ud, sweep, np.max(np.abs(got - want)))
    monkeypatch.delenv("CEDAR_AMD_FRUN2")
    two = q0[0].copy()  # and the band-fused order has the bits of the two row-class launches
    for sweep in range(3):
        K.relax2_op32(so, qf[0], two, sor, UP)
    assert same_bits(two, got)


@pytest.mark.parametrize("shape,frun", [(s, 2) for s in BAND_SHAPES] + [((130, 40), 4)], ids=str)
def test_partial_sum_sweep_is_its_fp64_self_on_the_rounded_operator(K, monkeypatch, shape, frun):
    """cedar_amd_relax2_gs_psum_op32 against cedar_amd_relax2_gs_psum on the rounded arrays at the same run length: both
    return 1, every bit equal (the partial-sum sweep is not bit-faithful to the reference order, it is to itself)"""
    monkeypatch.setenv("CEDAR_AMD_FRUN2", str(frun))
    so, qf, q0, sor, so_r, sor_r = kernel_problem(shape, 5)
    for ud in (DOWN, UP):
        want, got, ref = q0[0].copy(), q0[0].copy(), q0[0].copy()
        for sweep in range(3):
            assert K.relax2_psum(so_r, qf[0], want, sor_r, ud) == 1
            assert K.relax2_psum_op32(so, qf[0], got, sor, ud) == 1
            assert same_bits(got, want), (shape, ud, sweep, np.max(np.abs(got - want)))
            K.relax2_op32(so, qf[0], ref, sor, ud)
        assert not np.array_equal(got, ref) and np.max(np.abs(got - ref)) < 1e-12  # another order of additions, really


def test_partial_sum_sweep_at_the_lds_limit(K, monkeypatch):
    """(4350,16) and (4351,16): two T rows of II doubles fit 68 KB at II = 4352 and not at 4353.  The first runs the
    partial-sum sweep (returns 1), the second returns 0 and is the reference-order sweep"""
    monkeypatch.setenv("CEDAR_AMD_FRUN2", "2")
    for shape, took in (((4350, 16), 1), ((4351, 16), 0)):
        so, qf, q0, sor, so_r, sor_r = kernel_problem(shape, 5)
        for ud in (DOWN, UP):
            want, got = q0[0].copy(), q0[0].copy()
            assert K.relax2_psum(so_r, qf[0], want, sor_r, ud) == took
            assert K.relax2_psum_op32(so, qf[0], got, sor, ud) == took
            assert same_bits(got, want), (shape, ud)
            if not took:
                ref = q0[0].copy()
                assert K.relax2_op32(so, qf[0], ref, sor, ud) == 0
                assert same_bits(got, ref)


def test_partial_sum_sweep_with_too_few_pairs_is_the_reference_order(K, monkeypatch):
    """(100,40): 50 pairs a row, so the call returns 0 and equals relax2_op32"""
    monkeypatch.setenv("CEDAR_AMD_FRUN2", "2")
    so, qf, q0, sor, so_r, sor_r = kernel_problem((100, 40), 5)
    for ud in (DOWN, UP):
        got, ref, want = q0[0].copy(), q0[0].copy(), q0[0].copy()
        assert K.relax2_psum_op32(so, qf[0], got, sor, ud) == 0
        assert K.relax2_op32(so, qf[0], ref, sor, ud) == 0
        K.relax2(so_r, qf[0], want, sor_r, ud)
        assert same_bits(got, ref) and same_bits(got, want)


# ---------------------------------------------------------------- 3. batches
MANY_CASES = [(s, 5, None) for s in SHAPES] + [(s, 3, None) for s in SHAPES] + [(s, 5, 2) for s in BAND_SHAPES]


@pytest.mark.parametrize("nrhs", NRHS)
@pytest.mark.parametrize("shape,nst,frun", MANY_CASES, ids=str)
def test_many_items_are_the_single_call_and_the_fp64_kernels(K, monkeypatch, shape, nst, frun, nrhs):
    """cedar_amd_relax2_gs_many_op32 / cedar_amd_residual2_many_op32: item m equals the single _op32 call on item m alone
    and BMG2_SymStd_relax_GS / _residual on the rounded arrays; the item beyond nrhs keeps its bits.  frun: with
    CEDAR_AMD_FRUN2 set, the band-fused launch on a batch"""
    if frun:
        monkeypatch.setenv("CEDAR_AMD_FRUN2", str(frun))
    so, qf, q0, sor, so_r, sor_r = kernel_problem(shape, nst)
    if nrhs + 1 > q0.shape[0]:
        nrhs = q0.shape[0] - 1  # (the largest grid keeps fewer items)
    qf, q0 = np.ascontiguousarray(qf[:nrhs + 1]), np.ascontiguousarray(q0[:nrhs + 1])
    for ud in (DOWN, UP):
        got = q0.copy()
        single = [q0[m].copy() for m in range(nrhs)]
        want = [q0[m].copy() for m in range(nrhs)]
        for sweep in range(2):
            assert K.relax2_many_op32(so, qf, got, sor, ud, nrhs=nrhs) == 0
            for m in range(nrhs):
                assert K.relax2_op32(so, qf[m], single[m], sor, ud) == 0
                K.relax2(so_r, qf[m], want[m], sor_r, ud)
                assert same_bits(got[m], single[m]) and same_bits(got[m], want[m]), (shape, nst, nrhs, ud, sweep, m)
        assert same_bits(got[nrhs], q0[nrhs]) and not np.array_equal(got[:nrhs], q0[:nrhs])
    sentinel = np.stack([pb.uniform(q0.shape[1:], 845 + m, -1, 1) for m in range(nrhs + 1)])
    got = sentinel.copy()
    assert K.residual2_many_op32(so, qf, q0, got, nrhs=nrhs) == 0
    ghost = ~pb.interior_mask(q0.shape[1:])
    for m in range(nrhs):
        one, want = sentinel[m].copy(), sentinel[m].copy()
        assert K.residual2_op32(so, qf[m], q0[m], one) == 0
        K.residual2(so_r, qf[m], q0[m], want)
        assert same_bits(got[m], one) and same_bits(got[m], want), (shape, nst, nrhs, m)
        assert same_bits(got[m][ghost], sentinel[m][ghost]) and not np.array_equal(got[m], sentinel[m])
    assert same_bits(got[nrhs], sentinel[nrhs])


def test_kernel_entry_points_refuse_overflow_bad_nrhs_bad_nstncl_and_null(capi, K, capfd):
    """an entry of 1e39, nrhs of 0 and 33, nstncl 4, a NULL array: -1, a message naming the call, outputs untouched"""
    so, qf, q0, sor, _, _ = kernel_problem((31, 9), 5)
    big = so.copy()
    big[2, 3, 7] = 1e39
    q1, qm = q0[0], np.ascontiguousarray(q0[:3])
    f1, fm = qf[0], np.ascontiguousarray(qf[:3])
    calls = [
        ("cedar_amd_relax2_gs_op32", q1, lambda a, o: K.relax2_op32(a, f1, o, sor, UP), 0),
        ("cedar_amd_relax2_gs_psum_op32", q1, lambda a, o: K.relax2_psum_op32(a, f1, o, sor, UP), 0),
        ("cedar_amd_residual2_op32", q1, lambda a, o: K.residual2_op32(a, f1, q1, o), 0),
        ("cedar_amd_relax2_gs_many_op32", qm, lambda a, o: K.relax2_many_op32(a, fm, o, sor, UP), 0),
        ("cedar_amd_residual2_many_op32", qm, lambda a, o: K.residual2_many_op32(a, fm, qm, o), 0),
    ]
    for name, init, call, rc in calls:
        out = init.copy()
        capfd.readouterr()
        assert call(big, out) == -1
        err = capfd.readouterr().err
        assert name in err and "overflows single precision" in err, (name, err)
        assert same_bits(out, init), name
        assert call(so, out) == rc and not np.array_equal(out, init), name  # and the same call is served on so
    for nrhs in (0, 33):
        out = qm.copy()
        capfd.readouterr()
        assert K.relax2_many_op32(so, fm, out, sor, UP, nrhs=nrhs) == -1
        err = capfd.readouterr().err
        assert "cedar_amd_relax2_gs_many_op32" in err and "nrhs" in err and same_bits(out, qm)
        assert K.residual2_many_op32(so, fm, qm, out, nrhs=nrhs) == -1
        err = capfd.readouterr().err
        assert "cedar_amd_residual2_many_op32" in err and "nrhs" in err and same_bits(out, qm)
    lib = capi.lib
    II, JJ = C.c_uint(33), C.c_uint(11)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    out = q1.copy()
    capfd.readouterr()
    lib.cedar_amd_relax2_gs_op32.argtypes = [C.c_void_p] * 4 + [C.c_uint] * 2 + [C.c_int] * 2
    lib.cedar_amd_residual2_op32.argtypes = [C.c_void_p] * 4 + [C.c_uint] * 2 + [C.c_int]
    assert lib.cedar_amd_relax2_gs_op32(p(so), p(f1), p(out), p(sor), II, JJ, 4, UP) == -1
    assert "nstncl" in capfd.readouterr().err and same_bits(out, q1)
    assert lib.cedar_amd_relax2_gs_op32(p(so), None, p(out), p(sor), II, JJ, 5, UP) == -1
    assert "cedar_amd_relax2_gs_op32" in capfd.readouterr().err and same_bits(out, q1)
    assert lib.cedar_amd_residual2_op32(None, p(f1), p(q1), p(out), II, JJ, 5) == -1
    assert "cedar_amd_residual2_op32" in capfd.readouterr().err and same_bits(out, q1)


# ---------------------------------------------------------------- 4 - 6. the solver
V11 = dict(relax="point", nrelax_pre=1, nrelax_post=1)
V21 = dict(relax="point", nrelax_pre=2, nrelax_post=1)
NITEMS = 3


@functools.lru_cache(maxsize=None)
def solver_problem(name):
    """operator, NITEMS right-hand sides (splitmix seeds 17, ...), NITEMS random interior vectors"""
    so = {"vc": lambda: pb.varcoef9(150, 140), "an": lambda: pb.aniso9(129, 70, eps=1e-1),
          "p5": lambda: pb.poisson2(129, 70)}[name]()
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


def levels_with_rows(s, min_rows):
    return sum(1 for l in range(smoothed(s)) if s.dims(l)[1] >= min_rows)


def round_products(s, a0=None):
    """replace A and SOR0 of every level by their float-rounded values (a0: level 0's A instead of what it holds)"""
    for l in range(s.nlevels()):
        A = s.array(l, "A") if (l or a0 is None) else a0
        s.set_array(l, "A", rt(A))
        s.set_array(l, "SOR0", rt(s.array(l, "SOR0")))


def handle_outputs(h, cyc, sym, b, r):
    o = {}
    if cyc == "v":
        x = r.copy()
        h.vcycle(x, b)
        o["cycle"] = x
        z = np.zeros_like(r)
        h.precondition(z, r)
        o["z"] = z
        x = np.zeros_like(b)
        o["cg_hist"] = (h.pcg if sym else h.fcg)(b, x, max_iter=40, tol=1e-10)
        o["cg_x"] = x
    else:
        x = np.zeros_like(b)
        o["solve_hist"] = h.solve(b, x)
        o["solve_x"] = x
    return o


ROUNDED_CASES = [("vc", V21, 1, None), ("vc", V11, 65, None), ("p5", V11, 1, None), ("p5", V21, 65, None), ("vc", V21, 1, 2)]


@pytest.mark.parametrize("name,kw,min_rows,frun", ROUNDED_CASES, ids=["vc-v21-1", "vc-v11-65", "p5-v11-1", "p5-v21-65", "vc-v21-psum"])
def test_cycle_on_rounded_products_is_bit_identical(capi, monkeypatch, name, kw, min_rows, frun):
    """two handles whose A and SOR0 are float-representable on every level; one calls use_fp32_operator_2d(min_rows),
    which returns the number of smoothed levels with that many rows (min_rows = 1: all, the LDS-sized small ones
    included, which then run the row kernels).  vcycle, precondition, the pcg history and iterate (fcg where the cycle is
    V(2,1)) do not differ in one bit, nor does an F-cycle solve's history.  varcoef9(150,140): levels 150x140, 75x70 and
    small ones; poisson2(129,70): a five-point level 0 and a nine-point level 1 of 65x35 (65 > 64: not small).
    frun: CEDAR_AMD_FRUN2, with which level 0 of varcoef9 runs the partial-sum sweep on both handles"""
    so, b, r = solver_problem(name)
    if frun:
        monkeypatch.setenv("CEDAR_AMD_FRUN2", str(frun))
    sym = kw["nrelax_pre"] == kw["nrelax_post"]
    for cyc in ("v", "f"):
        ref, s = capi.Solver(so, max_iter=4, tol=0.0, cycle=cyc, **kw), capi.Solver(so, max_iter=4, tol=0.0, cycle=cyc, **kw)
        assert s.array(0, "A").shape[0] == (3 if name == "p5" else 5) and s.array(1, "A").shape[0] == 5 and smoothed(s) >= 3
        round_products(ref)
        round_products(s)
        assert s.fp32_levels() == 0
        want_levels = levels_with_rows(s, min_rows)
        assert 0 < want_levels and (want_levels == smoothed(s)) == (min_rows == 1)
        assert s.use_fp32_operator_2d(min_rows) == want_levels == s.fp32_levels()
        want, got = handle_outputs(ref, cyc, sym, b[0], r[0]), handle_outputs(s, cyc, sym, b[0], r[0])
        ref.close()
        s.close()
        for key in want:
            assert same_bits(got[key], want[key]), (name, cyc, key)
        if cyc == "v":
            assert len(got["cg_hist"]) > 2 and got["cg_hist"][-1] < 1e-10 and not np.array_equal(got["cycle"], r[0])
        else:
            assert len(got["solve_hist"]) == 5


@pytest.mark.parametrize("name,kw", [("vc", V21), ("p5", V11)], ids=["vc-v21", "p5-v11"])
def test_batched_cycle_on_rounded_products_is_bit_identical(capi, name, kw):
    """the same with create_many handles: vcycle_many on three items against the FP64 batch handle on the rounded
    products, and pcg_many (fcg_many for V(2,1)) item by item against the single switched handle"""
    so, b, r = solver_problem(name)
    sym = kw["nrelax_pre"] == kw["nrelax_post"]
    ref, s, one = capi.Solver(so, max_rhs=4, **kw), capi.Solver(so, max_rhs=4, **kw), capi.Solver(so, **kw)
    for h in (ref, s, one):
        round_products(h)
    assert s.use_fp32_operator_2d(1) == smoothed(s) == s.fp32_levels()
    assert one.use_fp32_operator_2d(1) == smoothed(one)
    want, got = r.copy(), r.copy()
    ref.vcycle_many(want, b)
    s.vcycle_many(got, b)
    assert same_bits(got, want) and not np.array_equal(got, r)
    x = np.zeros_like(b)
    hist, iters = (s.pcg_many if sym else s.fcg_many)(b, x, max_iter=40, tol=1e-10)
    xr = np.zeros_like(b)
    hist_r, iters_r = (ref.pcg_many if sym else ref.fcg_many)(b, xr, max_iter=40, tol=1e-10)
    assert iters == iters_r and same_bits(x, xr) and min(iters) > 2
    for m in range(NITEMS):
        x1 = r[m].copy()
        one.vcycle(x1, b[m])
        assert same_bits(got[m], x1), (name, m)
        x1 = np.zeros_like(b[m])
        h1 = (one.pcg if sym else one.fcg)(b[m], x1, max_iter=40, tol=1e-10)
        assert same_bits(hist[m], h1) and same_bits(x[m], x1), (name, m)
    # nrhs == 1 on the batch handle
    x1, xm = r[0].copy(), r[:1].copy()
    one.vcycle(x1, b[0])
    s.vcycle_many(xm, b[:1])
    assert same_bits(xm[0], x1)
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


@pytest.mark.parametrize("name", ["vc", "an", "p5"])
def test_real_operator_converges_to_the_fp64_solution(capi, name):
    """the unrounded operator, FP64 handle against a handle after use_fp32_operator_2d(1): pcg (V(1,1)), fcg (V(2,1)) and
    solve (V(2,1)) to 1e-10.  Both handles meet the stop test; the true relative residual (oracle matvec on the unrounded
    so) is within tol plus the rounding bound of evaluating b - A x twice; the switched handle takes the FP64 handle's
    number of iterations, or one more"""
    from pyoracle import Oracle
    O = Oracle()
    so, bb, _ = solver_problem(name)
    b = bb[0]
    tol = 1e-10
    for kind, kw in (("pcg", V11), ("fcg", V21), ("solve", V21)):
        # (max_iter 150: the plain V(2,1) cycle with point relaxation contracts by 0.78 on the anisotropic operator and needs
        # some 95 cycles, FP64 or not -- checked beforehand with the CPU oracle; the Krylov runs need 34 at most)
        ref, s = capi.Solver(so, max_iter=150, tol=tol, **kw), capi.Solver(so, max_iter=150, tol=tol, **kw)
        assert s.use_fp32_operator_2d(1) == smoothed(s) and ref.fp32_levels() == 0
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
    with 1023 in FP64; the level below (512 rows) stays FP64 either way"""
    for ny, want in ((1024, 1), (1023, 0)):
        s = capi.Solver(mk(9, ny), **V11)
        assert smoothed(s) >= 2 and s.dims(1)[1] < 1024
        assert s.use_fp32_operator_2d(0) == want == s.fp32_levels()
        assert s.use_fp32_operator_2d(ny) == 1  # an explicit min_rows switches level 0 in both cases
        s.close()


def test_min_rows_env_overrides_the_default(capi, monkeypatch):
    """CEDAR_AMD_OP32_MIN_ROWS, read at the call, stands in for min_rows = 0; an explicit min_rows wins over it"""
    so, b, r = solver_problem("vc")
    s = capi.Solver(so, **V11)
    assert s.use_fp32_operator_2d(0) == 0  # 140 rows: far below the default
    monkeypatch.setenv("CEDAR_AMD_OP32_MIN_ROWS", "100")
    assert s.use_fp32_operator_2d(0) == 1 == levels_with_rows(s, 100)
    monkeypatch.setenv("CEDAR_AMD_OP32_MIN_ROWS", "70")
    assert s.use_fp32_operator_2d(0) == 2 == levels_with_rows(s, 70)
    assert s.use_fp32_operator_2d(1) == smoothed(s)
    s.close()


def test_repetition_is_idempotent_and_never_switches_back(capi):
    so, b, r = solver_problem("vc")
    s = capi.Solver(so, **V11)
    n65 = levels_with_rows(s, 65)
    assert s.use_fp32_operator_2d(65) == n65 == 2
    z1 = np.zeros_like(r[0])
    s.precondition(z1, r[0])
    assert s.use_fp32_operator_2d(65) == n65 and s.use_fp32_operator_2d(1000) == n65
    z2 = np.zeros_like(r[0])
    s.precondition(z2, r[0])
    assert same_bits(z1, z2)
    assert s.use_fp32_operator_2d(1) == smoothed(s) == s.use_fp32_operator_2d(1)
    s.close()


def test_set_after_the_switch_rebuilds_the_float_copy(capi, capfd):
    """cedar_amd_solver_set("A" | "SOR0") on a switched level: the bits of a fresh handle built on those arrays and
    switched, and of a plain FP64 handle on the rounded products; an A with an entry of 1e39 is reported and the level
    reads FP64 again"""
    so, b, r = solver_problem("vc")
    r = r[0]
    a_new = rt(so * pb.uniform(so.shape, 861, 0.97, 1.03))
    s = capi.Solver(so, **V11)
    round_products(s)
    n = s.use_fp32_operator_2d(1)
    assert n == smoothed(s)
    sor_new = rt(s.array(0, "SOR0") * 0.98)
    z_old = np.zeros_like(r)
    s.precondition(z_old, r)
    s.set_array(0, "A", a_new)
    s.set_array(0, "SOR0", sor_new)
    fresh = capi.Solver(so, **V11)
    round_products(fresh, a0=a_new)
    fresh.set_array(0, "SOR0", sor_new)
    assert fresh.use_fp32_operator_2d(1) == n
    plain = capi.Solver(so, **V11)
    round_products(plain, a0=a_new)
    plain.set_array(0, "SOR0", sor_new)
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
    for h in (s, fresh, plain):
        h.close()


def test_refusals_leave_the_handle_as_it_was(capi, capfd):
    """NULL handle, 3D handle, ibc = 2, line-x relaxation, min_rows = -1, an entry of 1e39: -1, a message,
    fp32_levels() == 0 and the next cycle's bits unchanged"""
    so2, b2 = pb.varcoef9(40, 30), pb.rhs2(40, 30)

    def refused(s, text, b, min_rows=1):
        def run():
            x = np.zeros_like(b)
            return [s.solve(b, x), x]
        before = run()
        capfd.readouterr()
        rc = s.use_fp32_operator_2d(min_rows)
        err = capfd.readouterr().err
        assert rc == -1 and "cedar_amd_solver_use_fp32_operator_2d" in err and text in err, (text, err)
        assert s.fp32_levels() == 0
        assert all(same_bits(a, c) for a, c in zip(before, run())), text
        s.close()

    refused(capi.Solver(pb.poisson3(9, 9, 9), max_iter=2, **V11), "cedar_amd_solver_use_fp32_operator_all", pb.rhs3(9, 9, 9))
    per = (True, False)
    refused(capi.Solver(pb.periodic_poisson2(16, 16, per), max_iter=2, ibc=pb.ibc_of(per), **V11), "periodic",
            pb.periodic_rhs2(16, 16, per))
    assert pb.ibc_of(per) == 2
    refused(capi.Solver(so2, relax="line-x", max_iter=2), "line relaxation", b2)
    refused(capi.Solver(so2, max_iter=2, **V11), "min_rows", b2, min_rows=-1)
    refused(capi.Solver(so2, max_rhs=4, max_iter=2, **V11), "min_rows", b2, min_rows=-1)
    big = so2.copy()
    big[1, 9, 9] = 1e39
    refused(capi.Solver(big, max_iter=1, **V11), "overflows single precision", b2)
    capfd.readouterr()
    assert capi.lib.cedar_amd_solver_use_fp32_operator_2d(None, 1) == -1
    assert "NULL solver handle" in capfd.readouterr().err
