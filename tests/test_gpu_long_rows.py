"""3D kernels on rows longer than one workgroup pass, against the oracle.

Every 3D launcher picks its kernel from the row length: nx itself (7-point residual / matvec: 64, 128 or 256 lanes,
steps at nx 64|65 and 255|256, a strided trip from nx 257), the column pairs of interp_add ((nx + 2) / 2: steps at nx
127|128 and 509|510, a second trip from nx 512), or npairs = (nx + 1) / 2 of the 27-point row kernels (64, 128, 256 and
512 lanes: steps at nx 128|129, 256|257, 512|513 and 1024|1025).  Past the last step a kernel walks its row in several
trips (residual27_rows<256> from nx 513, a third trip from 1025), another kernel is launched (relax27_colour, eight
whole colours, from nx 1025) or the single-vector path runs item by item (many3d.hip).  The shapes below sit on both
sides of every one of these steps with ny and nz tiny, odd and even; (1540, 3, 4) gives the 256-lane kernels a fourth
trip.

Tolerances are those of tests/test_gpu_kernels.py: bit-identical for recip / relax / residual / matvec / interpolation
set-up / restrict / interp_add (reference operation order, -ffp-contract=off), 1e-13 of max-abs for the Galerkin product
(different association); solver histories rtol 1e-10 / atol 1e-14 and x to 1e-12 (test_27pt_256_cubed_history_vs_oracle).
"""
import ctypes as C

import numpy as np
import pytest

import cases
import problems as pb
from test_gpu_kernels import check
from test_oracle_periodic3d import EXACT as EXACT_PER3

pytestmark = pytest.mark.gpu

DOWN, UP = 0, 1

SHAPES27 = [(513, 6, 5), (600, 9, 8), (1023, 4, 5), (1024, 5, 4), (1025, 4, 5), (1030, 5, 4), (1540, 3, 4),
            # the steps the list above does not straddle: 64|65 and 128|129 pairs, interp_add's 127|128, 509|510, 511|512
            (127, 4, 5), (128, 5, 4), (129, 4, 5), (256, 5, 4), (257, 4, 5), (509, 5, 4), (510, 4, 5), (511, 5, 4), (512, 4, 5)]
SHAPES7 = [(65, 5, 4), (255, 4, 5), (256, 5, 4), (257, 4, 5), (513, 5, 6), (600, 6, 5), (1030, 4, 5),
           # 64 points (one 64-lane pass), interp_add's steps
           (64, 4, 5), (127, 5, 4), (128, 4, 5), (509, 4, 5), (510, 5, 4), (511, 4, 5), (512, 5, 4)]
CASES = [("l_%dx%dx%d_27" % s, s[0], s[1], s[2], 14) for s in SHAPES27] + [("l_%dx%dx%d_7" % s, s[0], s[1], s[2], 4) for s in SHAPES7]


@pytest.fixture(scope="module")
def capi():
    from cedar_amd import capi
    assert capi.device_count() >= 1, "no GPU visible"
    return capi


@pytest.fixture(scope="module")
def K(capi):
    return capi.Kernels()


def _grid(shape):
    nx, ny, nz = shape
    return (nz + 2, ny + 2, nx + 2)


def _ghosts(g):
    return ~pb.interior_mask(g)


# ------------------------------------------------------------------ 1. every kernel of the suite
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_kernel_suite_vs_oracle(K, oracle, case):
    got, want = cases.kernel_suite_3d(K, case), cases.kernel_suite_3d(oracle, case)
    assert set(got) == set(want)
    for k in want:
        check(f"{case[0]}/{k}", got[k], want[k])


def _ghost_suite(impl, case, ci):
    """relax (two sweeps, both directions), residual, restrict and interp_add on an operator whose ghost entries are
    not zero, vectors with non-zero ghost cells; ci: interpolation weights (the oracle's, for both sides)"""
    name, nx, ny, nz, nst = case
    sd = cases._seed(name) + 1000
    g = _grid((nx, ny, nz))
    gc = pb.coarse_shape(g)
    so = pb.random_op(g, nst, sd, zero_ghost=False)
    qf, q0 = pb.uniform(g, sd + 1, -1, 1), pb.uniform(g, sd + 2, -1, 1)
    sor = np.zeros((2,) + g)
    impl.setup_recip3(so, sor)
    out = {"q0": q0}
    for ud in (DOWN, UP):
        q = q0.copy()
        impl.relax3(so, qf, q, sor, ud)
        impl.relax3(so, qf, q, sor, ud)
        out[f"relax{ud}"] = q
    r0 = pb.uniform(g, sd + 3, -1, 1)
    r = r0.copy()
    impl.residual3(so, qf, q0, r)
    out["residual"], out["r0"] = r, r0
    qc = pb.uniform(gc, sd + 4, -1, 1)
    impl.restrict3(q0, qc, ci)
    out["restrict"] = qc
    qcx = pb.uniform(gc, sd + 5, -1, 1) * pb.interior_mask(gc)
    q, res = q0.copy(), qf.copy()
    impl.interp_add3(q, qcx, so, res, ci)
    out["interp_add_q"], out["interp_add_res"] = q, res
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_kernels_with_nonzero_ghosts_vs_oracle(K, oracle, case):
    """kernel_suite_3d zeroes the operator's ghost entries; here they are random, as are the ghost cells of q and qf:
    a lane of a later trip that reads one column too far, or the ghost column through the wrong slot, shows.  relax and
    residual leave every ghost cell of the vector they write as it was."""
    name, nx, ny, nz, nst = case
    g = _grid((nx, ny, nz))
    so = pb.random_op(g, nst, cases._seed(name) + 1000, zero_ghost=False)
    ci = np.zeros((26,) + pb.coarse_shape(g))
    oracle.setup_interp3(so, ci)
    got, want = _ghost_suite(K, case, ci), _ghost_suite(oracle, case, ci)
    for k in ("relax0", "relax1", "residual", "restrict", "interp_add_q", "interp_add_res"):
        assert np.array_equal(got[k], want[k]), (name, k, np.max(np.abs(got[k] - want[k])))
    gh = _ghosts(g)
    for k in ("relax0", "relax1"):
        assert np.array_equal(got[k][gh], got["q0"][gh]), (name, k)
    assert np.array_equal(got["residual"][gh], got["r0"][gh]), name


# ------------------------------------------------------------------ 2. matvec3
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_matvec3_vs_oracle(K, oracle, case):
    """cedar_amd_matvec3 (residual3_kernel<.., MV = true>, both stencils): the interior bit for bit"""
    name, nx, ny, nz, nst = case
    g = _grid((nx, ny, nz))
    sd = cases._seed(name) + 2000
    so = pb.random_op(g, nst, sd, zero_ghost=False)
    q = pb.uniform(g, sd + 1, -1, 1)
    got, want = np.zeros(g), np.zeros(g)
    K.matvec3(so, q, got)
    oracle.matvec3(so, q, want)
    inner = (slice(1, -1),) * 3
    assert np.any(want[inner] != 0)
    assert np.array_equal(got[inner], want[inner]), (name, np.max(np.abs(got[inner] - want[inner])))


# ------------------------------------------------------------------ 3. plane-fused sweep on wide rows
def _relax_problem(oracle, shape, sd):
    g = _grid(shape)
    so = pb.random_op(g, 14, sd, zero_ghost=False)
    qf, q0 = pb.uniform(g, sd + 1, -1, 1), pb.uniform(g, sd + 2, -1, 1)
    sor = np.zeros((2,) + g)
    oracle.setup_recip3(so, sor)
    return g, so, qf, q0, sor


@pytest.fixture(scope="module")
def wide_sweeps(oracle):
    """the reference sweeps of the plane-fused cases, computed once per shape: {shape: (so, qf, q0, sor, [DOWN, UP])}"""
    memo = {}

    def get(shape):
        if shape not in memo:
            g, so, qf, q0, sor = _relax_problem(oracle, shape, 41)
            want = []
            for ud in (DOWN, UP):
                w = q0.copy()
                oracle.relax3(so, qf, w, sor, ud)
                w.setflags(write=False)
                want.append(w)
            memo[shape] = (so, qf, q0, sor, want)
        return memo[shape]
    return get


@pytest.mark.parametrize("shape,frun", [(s, f) for s in [(514, 16, 5), (600, 9, 4), (1024, 13, 3)] for f in (1, 2, 3)
                                        if s[1] >= 4 * f] + [((1030, 9, 4), 2)], ids=str)
def test_plane_fused_relax_on_wide_rows(K, wide_sweeps, monkeypatch, shape, frun):
    """relax27_plane<512> + the deferred rows between runs (ny >= 4 frun) for nx 513 .. 1024, both directions, bit for
    bit in the reference order; at nx = 1030 the launcher must leave the plane-fused path for whole colours"""
    monkeypatch.setenv("CEDAR_AMD_FRUN", str(frun))
    so, qf, q0, sor, want = wide_sweeps(shape)
    for ud in (DOWN, UP):
        got = q0.copy()
        K.relax3(so, qf, got, sor, ud)
        assert np.array_equal(got, want[ud]), (shape, frun, ud, np.max(np.abs(got - want[ud])))


# ------------------------------------------------------------------ 4. sweep pieces
PIECE_SHAPES = [(600, 9, 6), (1024, 6, 5), (1030, 7, 4)]


def _device_problem(capi, oracle, shape, sd):
    g, so, qf, q0, sor = _relax_problem(oracle, shape, sd)
    want = []
    for ud in (DOWN, UP):
        w = q0.copy()
        oracle.relax3(so, qf, w, sor, ud)
        want.append(w)
    dev = tuple(capi.DeviceArray.from_numpy(a) for a in (so, qf, sor))
    return g, q0, want, dev


@pytest.mark.parametrize("shape", PIECE_SHAPES, ids=str)
def test_partial_row_class_passes_on_long_rows(capi, oracle, shape):
    """cedar_amd_relax3_pass_part (launch_part<512>, relax27_rows_shell<512>; whole colours from 1025 points on):
    interior rows then shell rows of a row class equal the whole class for every class, both colour orders and every
    face mask; the four classes in sweep order equal the reference sweep, whole and in parts.  Where the rows are too
    long for the row kernel, part 1 must leave q as it is and part 2 do the whole class."""
    nx, ny, nz = shape
    g, q0, want, (so, qf, sor) = _device_problem(capi, oracle, shape, 51)
    u = C.c_uint
    f = capi.lib.cedar_amd_relax3_pass_part
    q = capi.DeviceArray(g)
    MASKS = (0, 1, 2, 4, 8, 5, 10, 15)

    def run(jb, kb, efirst, part_sides):
        f(capi._p(so), capi._p(qf), capi._p(q), capi._p(sor), u(nx + 2), u(ny + 2), u(nz + 2), jb, kb, efirst, part_sides)

    for jb in (0, 1):
        for kb in (0, 1):
            for efirst in (0, 1):
                q.upload(q0)
                run(jb, kb, efirst, 0)
                whole = q.numpy()
                assert not np.array_equal(whole, q0)
                for sides in MASKS:
                    q.upload(q0)
                    run(jb, kb, efirst, 1 | (sides << 4))
                    if nx > 1024:
                        assert np.array_equal(q.numpy(), q0), (shape, jb, kb, efirst, sides)
                    run(jb, kb, efirst, 2 | (sides << 4))
                    assert np.array_equal(q.numpy(), whole), (shape, jb, kb, efirst, sides)
    for ud in (DOWN, UP):
        order = [(c & 1, c >> 1) for c in (range(4) if ud == UP else range(3, -1, -1))]
        for sides in (None,) + MASKS:
            q.upload(q0)
            for jb, kb in order:
                for part in ((0,) if sides is None else (1, 2)):
                    run(jb, kb, int(ud == UP), part | ((sides or 0) << 4))
            got = q.numpy()
            assert np.array_equal(got, want[ud]), (shape, ud, sides, np.max(np.abs(got - want[ud])))


@pytest.mark.parametrize("frun", [0, 3])
@pytest.mark.parametrize("shape", PIECE_SHAPES, ids=str)
def test_plane_parity_passes_on_long_rows(capi, oracle, monkeypatch, shape, frun):
    """cedar_amd_relax3_planes (planes_bs<512>; whole colours from 1025 points on): the two k-parities in sweep order
    equal the reference sweep, and so do interior planes + shell planes for every z-face mask; where the rows are too
    long for the row kernels part 1 must leave q as it is and part 2 do the whole parity -- also when the mask leaves
    the parity without a shell plane"""
    monkeypatch.setenv("CEDAR_AMD_FRUN", str(frun))
    nx, ny, nz = shape
    g, q0, want, (so, qf, sor) = _device_problem(capi, oracle, shape, 61)
    u = C.c_uint
    f = capi.lib.cedar_amd_relax3_planes
    q = capi.DeviceArray(g)

    def run(kb, up, part_sides):
        f(capi._p(so), capi._p(qf), capi._p(q), capi._p(sor), u(nx + 2), u(ny + 2), u(nz + 2), kb, up, part_sides)

    for up in (0, 1):
        q.upload(q0)
        for c in range(2):
            run(c if up else 1 - c, up, 0)
        got = q.numpy()
        assert np.array_equal(got, want[up]), (shape, frun, up, np.max(np.abs(got - want[up])))
        for sides in (0, 4, 8, 12):
            q.upload(q0)
            for c in range(2):
                kb = c if up else 1 - c
                before = q.numpy()
                run(kb, up, 1 | (sides << 4))
                if nx > 1024:
                    assert np.array_equal(q.numpy(), before), (shape, frun, up, sides, kb)
                run(kb, up, 2 | (sides << 4))
            got = q.numpy()
            assert np.array_equal(got, want[up]), (shape, frun, up, sides, np.max(np.abs(got - want[up])))


# ------------------------------------------------------------------ 5. batched kernels
MANY_CASES = [((600, 9, 8), 14), ((1024, 5, 4), 14), ((1030, 5, 4), 14), ((600, 6, 5), 4)]


def _items(g, n, seed):
    return np.stack([pb.uniform(g, seed + 17 * m, -1, 1) for m in range(n)])


@pytest.fixture(scope="module")
def many_operator(oracle):
    memo = {}

    def get(shape, nst):
        if (shape, nst) not in memo:
            g = _grid(shape)
            sd = 7 * shape[0] + 131 * shape[1] + 1009 * shape[2] + nst
            so = pb.random_op(g, nst, sd, zero_ghost=False)
            sor = np.zeros((2,) + g)
            oracle.setup_recip3(so, sor)
            gc = pb.coarse_shape(g)
            ci = np.zeros((26,) + gc)
            oracle.setup_interp3(so, ci)
            for a in (so, sor, ci):
                a.setflags(write=False)
            memo[(shape, nst)] = (g, gc, sd, so, sor, ci)
        return memo[(shape, nst)]
    return get


@pytest.mark.parametrize("nrhs", [1, 3, 8])
@pytest.mark.parametrize("shape,nst", MANY_CASES, ids=str)
def test_relax_many_on_long_rows(capi, K, oracle, many_operator, shape, nst, nrhs):
    """relax27_rows_many<512> (nx 513 .. 1024), the item-by-item colour sweeps beyond, relax7_colour_many: two sweeps,
    both directions; every item bit-identical to the oracle on that item alone, the spare item untouched"""
    g, _, sd, so, sor, _ = many_operator(shape, nst)
    qf, q0 = _items(g, nrhs + 1, sd + 1), _items(g, nrhs + 1, sd + 2)
    gh = _ghosts(g)
    for ud in (DOWN, UP):
        dq, dqf = capi.DeviceArray.from_numpy(q0), capi.DeviceArray.from_numpy(qf)
        K.relax3_many(so, dqf, dq, sor, ud, nrhs=nrhs)
        K.relax3_many(so, dqf, dq, sor, ud, nrhs=nrhs)
        got = dq.numpy()
        for m in range(nrhs):
            want = q0[m].copy()
            oracle.relax3(so, qf[m], want, sor, ud)
            oracle.relax3(so, qf[m], want, sor, ud)
            assert np.array_equal(got[m], want), (shape, nst, nrhs, ud, m, np.max(np.abs(got[m] - want)))
            assert np.array_equal(got[m][gh], q0[m][gh])
        assert np.array_equal(got[nrhs], q0[nrhs]), "the item beyond nrhs was touched"
        assert np.array_equal(dqf.numpy(), qf)


@pytest.mark.parametrize("nrhs", [1, 3, 8])
@pytest.mark.parametrize("shape,nst", MANY_CASES, ids=str)
def test_residual_and_transfers_many_on_long_rows(capi, K, oracle, many_operator, shape, nst, nrhs):
    """residual27_rows_many<256> beyond one trip, residual7_many_kernel on its strided trip, restrict3_many with
    several blocks per row, interp_add3_many beyond one trip: item by item against the oracle, spare item untouched"""
    g, gc, sd, so, _, ci = many_operator(shape, nst)
    dev = capi.DeviceArray.from_numpy
    gh = _ghosts(g)
    qf, q, r0 = _items(g, nrhs + 1, sd + 1), _items(g, nrhs + 1, sd + 2), _items(g, nrhs + 1, sd + 3)
    dr = dev(r0)
    K.residual3_many(so, dev(qf), dev(q), dr, nrhs=nrhs)
    got = dr.numpy()
    for m in range(nrhs):
        want = r0[m].copy()
        oracle.residual3(so, qf[m], q[m], want)
        assert np.array_equal(got[m], want), ("residual", shape, nst, nrhs, m, np.max(np.abs(got[m] - want)))
        assert np.array_equal(got[m][gh], r0[m][gh])
    assert np.array_equal(got[nrhs], r0[nrhs])

    qc0 = _items(gc, nrhs + 1, sd + 5)
    dqc = dev(qc0)
    K.restrict3_many(dev(q), dqc, ci, nrhs=nrhs)
    got = dqc.numpy()
    ghc = _ghosts(gc)
    for m in range(nrhs):
        want = qc0[m].copy()
        oracle.restrict3(q[m], want, ci)
        assert np.array_equal(got[m], want), ("restrict", shape, nst, nrhs, m, np.max(np.abs(got[m] - want)))
        assert np.array_equal(got[m][ghc], qc0[m][ghc])
    assert np.array_equal(got[nrhs], qc0[nrhs])

    qc = _items(gc, nrhs + 1, sd + 8) * pb.interior_mask(gc)
    dq, dres = dev(q), dev(r0)
    K.interp_add3_many(dq, dev(qc), so, dres, ci, nrhs=nrhs)
    gq, gr = dq.numpy(), dres.numpy()
    for m in range(nrhs):
        wq, wr = q[m].copy(), r0[m].copy()
        oracle.interp_add3(wq, qc[m], so, wr, ci)
        assert np.array_equal(gq[m], wq), ("interp_add q", shape, nst, nrhs, m, np.max(np.abs(gq[m] - wq)))
        assert np.array_equal(gr[m], wr), ("interp_add res", shape, nst, nrhs, m, np.max(np.abs(gr[m] - wr)))
    assert np.array_equal(gq[nrhs], q[nrhs]) and np.array_equal(gr[nrhs], r0[nrhs])


# ------------------------------------------------------------------ 6. periodic x
PER3 = [("q600x4x6_27_x", 600, 4, 6, 14, 2), ("q1030x4x6_27_x", 1030, 4, 6, 14, 2), ("q1026x4x6_27_xy", 1026, 4, 6, 14, 3),
        ("q600x4x6_7_x", 600, 4, 6, 4, 2)]


@pytest.mark.parametrize("case", PER3, ids=lambda c: c[0])
def test_periodic_x_on_long_rows(K, oracle, case):
    """relax27_rows<512, .., PERX> (launch_rows_perx<512>) at 600 points, the eight-colour periodic sweep beyond 1024,
    and the periodic transfers at these widths: the comparisons of tests/test_gpu_periodic3d.py"""
    got, want = cases.kernel_suite_per3(K, case), cases.kernel_suite_per3(oracle, case)
    assert set(got) == set(want)
    for k in want:
        if k in EXACT_PER3:
            assert np.array_equal(got[k], want[k]), (case[0], k, np.max(np.abs(got[k] - want[k])))
        else:
            assert np.max(np.abs(got[k] - want[k])) <= 1e-13 * np.max(np.abs(want[k])), (case[0], k)


# ------------------------------------------------------------------ 7. resident solver
# (operator, shape, min_coarse).  (1030, 9, 8) with the default min_coarse = 3 stops coarsening at (515, 5, 4): a direct
# solve of 10300 unknowns in a band of 3092, 190 s of set-up in the oracle alone.  min_coarse = 2 adds the level
# (258, 3, 2) -- 1.5 s -- and leaves level 0, the subject of the test, as it is; the oracle's history barely moves
# (1.37e-1 .. 4.85e-9 over six cycles against 1.37e-1 .. 4.82e-9).
SOLVER_CASES = [("fe27", (600, 10, 9), 3), ("fe27", (1030, 9, 8), 2), ("poisson7", (600, 10, 9), 3)]


def _solver_problem(kind, shape):
    return (pb.fe3(*shape) if kind == "fe27" else pb.poisson3(*shape)), pb.rhs3(*shape)


@pytest.mark.parametrize("kind,shape,min_coarse", SOLVER_CASES, ids=str)
def test_resident_solver_history_on_long_rows(capi, oracle, kind, shape, min_coarse):
    """capi.Solver with a level 0 of more than 256 (600 points) and more than 512 (1030 points) pairs per row:
    V(2,1), six cycles, the oracle's history iteration for iteration and its solution.  The 27-point problems
    converge (1.63e-1 .. 5.6e-10 and 1.37e-1 .. 4.9e-9 in the oracle); point relaxation stagnates on the 7-point
    Laplacian of this thin box (relative residual 1.4 after six cycles), where the comparison still pins every kernel
    of the cycle."""
    so, b = _solver_problem(kind, shape)
    ml = oracle.ml_create(so, nrelax_pre=2, nrelax_post=1, min_coarse=min_coarse)
    xo = np.zeros_like(b)
    want = ml.solve(b, xo, maxiter=6)
    ml.close()
    s = capi.Solver(so, nrelax_pre=2, nrelax_post=1, max_iter=6, min_coarse=min_coarse)
    x = np.zeros_like(b)
    h = s.solve(b, x)
    s.close()
    assert len(h) == len(want)
    if kind == "fe27":
        assert want[-1] < 1e-8  # the problem converges: the comparison means something
    np.testing.assert_allclose(h, want, rtol=1e-10, atol=1e-14)
    assert np.max(np.abs(x - xo)) <= 1e-12 * np.max(np.abs(xo))


def test_solve_many_equals_single_solves_on_long_rows(capi):
    """solve_many with three right-hand sides at (600, 10, 9): histories and solutions of three single solves, bit for bit"""
    shape = (600, 10, 9)
    so, b0 = _solver_problem("fe27", shape)
    m = pb.interior_mask(b0.shape)
    b = np.stack([b0] + [pb.uniform(b0.shape, 4242 + t, -1, 1) * m * np.max(np.abs(b0)) for t in (1, 2)])
    sm = capi.Solver(so, max_iter=6, max_rhs=3)
    xs = np.zeros_like(b)
    rel, iters = sm.solve_many(b, xs)
    sm.close()
    s1 = capi.Solver(so, max_iter=6)
    for t in range(3):
        x1 = np.zeros_like(b[t])
        h1 = s1.solve(b[t], x1)
        assert iters[t] == len(h1) - 1, (t, iters, len(h1))
        assert np.array_equal(rel[t][: iters[t] + 1], h1), (t, rel[t], h1)
        assert np.array_equal(xs[t], x1), (t, np.max(np.abs(xs[t] - x1)))
    s1.close()
    assert len(rel[0]) - 1 == max(iters)
