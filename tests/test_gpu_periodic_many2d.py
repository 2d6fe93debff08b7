"""Several right-hand sides at once on periodic 2D handles (cedar_amd_solver_create_many_periodic2; periodic_many2d.hip).

The one rule checked everywhere: item m of a batched result has the bits of the single-vector periodic call on item m
alone (np.array_equal, no tolerance).  Every device array holds one item more than nrhs, and the item beyond must keep
every bit.  The ghost cells of the input vectors are non-zero.

1. The kernels one by one (Kernels.*_periodic_many): the sweep against the oracle's periodic sweep and the single-vector
   drop-in; restriction, interpolation-and-add and the dense coarsest solve against the single-vector drop-ins.  Row
   lengths from the launcher (relax2_gs_per_many): up to 512 interior points one workgroup relaxes a grid row for all
   items; longer rows take one launch per i-colour, 256 points of the colour per workgroup (1030: three segments, the
   last nearly empty; 4094 / 4100 and 8190: eight, nine and sixteen), each followed by the x wrap of its rows; 8190 is
   the limit of the single-vector handle, which the batch keeps.  (A batch whose stride is not ii*jj walks its items
   through the single-vector sweep; the C call always passes ii*jj, so no shape reaches that walk from here.)
2. The cycle and the solve on the nine V-cycle entries of cases.SOLVES_PER against a plain periodic handle; the two
   F-cycle entries are refused by the creation call.
3. One- and two-level handles, nrhs 4 / 1 / 3 on one handle, reuse after cedar_amd_solver_set, reproducibility.
4. Refusals.
"""
import ctypes as C

import numpy as np
import pytest

import cases
import pcg_statement as ps
import problems as pb

pytestmark = pytest.mark.gpu
DOWN, UP = cases.DOWN, cases.UP
NRHS = [1, 2, 3, 8]
NMAX = max(NRHS) + 1  # items the arrays hold
PER = {1: (False, True), 2: (True, False), 3: (True, True)}  # (x, y) of a boundary code


@pytest.fixture(scope="module")
def capi():
    from cedar_amd import capi
    assert capi.device_count() >= 1, "no GPU visible"
    return capi


@pytest.fixture(scope="module")
def K(capi):
    return capi.Kernels()


def _items(g, n, seed, scale=1.0):
    """n vectors drawn with different seeds, ghost cells non-zero"""
    return np.stack([pb.uniform(g, seed + 17 * m, -1, 1) * scale for m in range(n)])


def _dev(capi, a):
    return capi.DeviceArray.from_numpy(np.ascontiguousarray(a))


def periodic_ghosts(g, per):
    m = np.zeros(g, dtype=bool)
    if per[0]:
        m[:, 0] = m[:, -1] = True
    if per[1]:
        m[0, :] = m[-1, :] = True
    return m


# ------------------------------------------------------------------ 1a. the sweep
# (nx, ny): the smallest row; odd nx; either side of the 512-point step between the two kernels; a colour of exactly two
# segments and of one point more (1024, 1026), a last segment of three points (1030); either side of 4096 points (where
# two rows of doubles stop fitting 64 KB of LDS); the limit
SWEEP = [(2, 4), (9, 6), (33, 5), (510, 4), (512, 4), (514, 4), (1024, 3), (1026, 3), (1030, 4), (4094, 3), (4100, 3), (8190, 3)]


@pytest.mark.parametrize("nst", [3, 5])
@pytest.mark.parametrize("shape", SWEEP, ids=str)
def test_relax_periodic_many(capi, K, oracle, shape, nst):
    nx, ny = shape
    g = (ny + 2, nx + 2)
    sd = 7 * nx + 131 * ny + 13 * nst
    so = pb.random_op(g, nst, sd, zero_ghost=False)
    sor = np.zeros((2,) + g)
    oracle.setup_recip2(so, sor)
    qf, q0 = _items(g, NMAX, sd + 1), _items(g, NMAX, sd + 2)
    dso, dsor, dqf = _dev(capi, so), _dev(capi, sor), _dev(capi, qf)
    for ibc in (1, 2, 3):
        fixed = ~pb.interior_mask(g) & ~periodic_ghosts(g, PER[ibc])  # ghost cells of the non-periodic direction
        for order in ((DOWN, UP), (UP, DOWN)):  # two sweeps in a row, either one first
            want = []
            for m in range(NMAX - 1):
                qo, qs, states = q0[m].copy(), q0[m].copy(), []
                for t, ud in enumerate(order):
                    oracle.relax2(so, qf[m], qo, sor, ud, ibc=ibc)
                    K.relax2(so, qf[m], qs, sor, ud, ibc=ibc)
                    assert np.array_equal(qs, qo), ("single", shape, nst, ibc, m, t)
                    states.append(qo.copy())
                want.append(states)
            for nrhs in NRHS:
                dq = _dev(capi, q0)
                for t, ud in enumerate(order):
                    K.relax2_periodic_many(dso, dqf, dq, dsor, ud, ibc, nrhs=nrhs)
                    got = dq.numpy()
                    for m in range(nrhs):
                        assert np.array_equal(got[m], want[m][t]), (shape, nst, ibc, order, nrhs, m, t, np.max(np.abs(got[m] - want[m][t])))
                        assert np.array_equal(got[m][fixed], q0[m][fixed]), ("fixed ghosts", shape, nst, ibc, m)
                    assert np.array_equal(got[nrhs:], q0[nrhs:]), ("item beyond", shape, nst, ibc, nrhs)
    assert np.array_equal(dqf.numpy(), qf) and np.array_equal(dso.numpy(), so)


# ------------------------------------------------------------------ 1b. the transfers
# the fine / coarse pairs of tests/test_gpu_periodic.py: cases.CASES_PER and its EXTRA list
TRANSFERS = cases.CASES_PER + [("x300x7_9_x", 300, 7, 5, 2), ("x1030x5_9_xy", 1030, 5, 5, 3), ("x129x130_5_y", 129, 130, 3, 1),
                               ("x4x4_9_xy", 4, 4, 5, 3), ("x5x4_5_x", 5, 4, 3, 2), ("x600x33_5_xy", 600, 33, 3, 3)]


def test_transfer_cases_cover_both_outcomes_of_the_refresh_test():
    """restrict2_per refreshes the ghosts of a periodic direction only where Nx / 2 + 1 == Nxc (extents with ghosts)"""
    seen = set()
    for _, nx, ny, _, ibc in TRANSFERS:
        gc = pb.coarse_shape((ny + 2, nx + 2))
        if PER[ibc][0]:
            seen.add(("x", (nx + 2) // 2 + 1 == gc[1]))
        if PER[ibc][1]:
            seen.add(("y", (ny + 2) // 2 + 1 == gc[0]))
    assert seen == {("x", True), ("x", False), ("y", True), ("y", False)} and {c[4] for c in TRANSFERS} == {1, 2, 3}


@pytest.mark.parametrize("case", TRANSFERS, ids=lambda c: c[0])
def test_transfers_periodic_many(capi, K, case):
    name, nx, ny, nst, ibc = case
    sd = cases._seed(name)
    g = (ny + 2, nx + 2)
    gc = pb.coarse_shape(g)
    so = pb.random_op(g, nst, sd, zero_ghost=False)
    ci = np.zeros((8,) + gc)
    K.setup_interp2(so, ci, ibc=ibc)
    assert ci.any()
    r0, qc0 = _items(g, NMAX, sd + 3), _items(gc, NMAX, sd + 4)
    x0, res0, xc = _items(g, NMAX, sd + 5), _items(g, NMAX, sd + 6), _items(gc, NMAX, sd + 7)
    want = []
    for m in range(NMAX - 1):
        r, qc = r0[m].copy(), qc0[m].copy()
        K.restrict2(r, qc, ci, ibc=ibc)
        x, res = x0[m].copy(), res0[m].copy()
        K.interp_add2(x, xc[m].copy(), res, so, ci, ibc=ibc)
        want.append((r, qc, x, res))
    assert not np.array_equal(want[0][3], res0[0])  # interp_add's side effect on res
    dso, dci, dxc = _dev(capi, so), _dev(capi, ci), _dev(capi, xc)
    for nrhs in NRHS:
        dr, dqc = _dev(capi, r0), _dev(capi, qc0)
        K.restrict2_periodic_many(dr, dqc, dci, ibc, nrhs=nrhs)
        r, qc = dr.numpy(), dqc.numpy()
        dx, dres = _dev(capi, x0), _dev(capi, res0)
        K.interp_add2_periodic_many(dx, dxc, dres, dso, dci, ibc, nrhs=nrhs)
        x, res = dx.numpy(), dres.numpy()
        assert np.array_equal(dxc.numpy(), xc)
        for m in range(nrhs):
            for what, a, b in zip(("restrict q (refreshed ghosts)", "restrict qc", "interp_add q", "interp_add res"),
                                  (r[m], qc[m], x[m], res[m]), want[m]):
                assert np.array_equal(a, b), (name, nrhs, m, what)
        for a, a0 in ((r, r0), (qc, qc0), (x, x0), (res, res0)):
            assert np.array_equal(a[nrhs:], a0[nrhs:]), ("item beyond", name, nrhs)


# ------------------------------------------------------------------ 1c. the coarsest solve
# interior sizes with 6, 12, 63, 64, 65 and 200 unknowns
CG_MANY = [(3, 2), (4, 3), (9, 7), (8, 8), (13, 5), (20, 10)]


@pytest.mark.parametrize("ibc", [1, 2, 3])
@pytest.mark.parametrize("shape", CG_MANY, ids=str)
def test_coarse_solve_periodic_many(capi, K, shape, ibc):
    nx, ny = shape
    n = nx * ny
    sd = 1000 * nx + 10 * ny + ibc
    so = pb.periodic_random_op(nx, ny, 5, PER[ibc], sd)  # strictly diagonally dominant: the wrapped matrix is definite
    g = so.shape[1:]
    abd = np.zeros((n, n))
    K.setup_cg2(so, abd, ibc=ibc)
    assert np.all(np.isfinite(abd)) and np.all(np.diag(abd) > 0)
    q0, qf = _items(g, NMAX, sd + 2), _items(g, NMAX, sd + 1)
    want = []
    for m in range(NMAX - 1):
        q = q0[m].copy()
        K.solve_cg2(q, qf[m].copy(), abd, ibc=ibc)
        assert np.all(np.isfinite(q))
        want.append(q)
    dabd = _dev(capi, abd)
    for nrhs in (1, 3, 8):
        dq, dqf = _dev(capi, q0), _dev(capi, qf)
        K.solve_cg2_periodic_many(dq, dqf, dabd, ibc, nrhs=nrhs)
        got = dq.numpy()
        for m in range(nrhs):
            assert np.array_equal(got[m], want[m]), (shape, ibc, nrhs, m, np.max(np.abs(got[m] - want[m])))
        assert np.array_equal(got[nrhs:], q0[nrhs:]) and np.array_equal(dqf.numpy(), qf), ("untouched", shape, ibc, nrhs)
    # items do not see each other: the reverse order gives each item the same bits
    dq, dqf = _dev(capi, q0[:8][::-1]), _dev(capi, qf[:8][::-1])
    K.solve_cg2_periodic_many(dq, dqf, dabd, ibc)
    got = dq.numpy()
    for m in range(8):
        assert np.array_equal(got[7 - m], want[m]), (shape, ibc, "reversed", m)
    assert np.array_equal(dabd.numpy(), abd)


# ------------------------------------------------------------------ 2. the cycle and the solve
VCASES = [k for k, v in cases.SOLVES_PER.items() if v[2].get("cycle", "v") == "v"]
FCASES = [k for k in cases.SOLVES_PER if k not in VCASES]


def raw_vcycle_many(capi, s, nrhs, dx, db):
    return capi.lib.cedar_amd_solver_vcycle_many(s.h, nrhs, dx.ptr, db.ptr)


def raw_solve_many(capi, s, nrhs, db, dx, rel, iters):
    return capi.lib.cedar_amd_solver_solve_many(s.h, nrhs, db.ptr, dx.ptr, rel.ctypes.data, iters.ctypes.data_as(C.POINTER(C.c_int)))


def four_items(mk_rhs):
    """five items, the first four take part"""
    b0 = mk_rhs()
    g = b0.shape
    scale = np.max(np.abs(b0))
    return np.stack([b0, 0.5 * b0, ps.random_field(g, 31) * scale, ps.random_field(g, 37) * scale, pb.uniform(g, 41, -1, 1)])


def single_results(s1, b, x0, nrhs):
    """per item on the plain handle: x after one and two cycles, and the solve"""
    out = []
    for m in range(nrhs):
        x = x0[m].copy()
        s1.vcycle(x, b[m])
        v1 = x.copy()
        s1.vcycle(x, b[m])
        xs = x0[m].copy()
        h = s1.solve(b[m], xs)
        out.append((v1, x, xs, h))
    return out


def check_batch(capi, sm, b, x0, want, nrhs, max_iter):
    """vcycle_many twice and solve_many on the first nrhs of the five items the arrays hold"""
    db = _dev(capi, b)
    dx = _dev(capi, x0)
    for t in range(2):
        assert raw_vcycle_many(capi, sm, nrhs, dx, db) == 0
        got = dx.numpy()
        for m in range(nrhs):
            assert np.array_equal(got[m], want[m][t]), ("vcycle", t, m, np.max(np.abs(got[m] - want[m][t])))
        assert np.array_equal(got[nrhs:], x0[nrhs:]), "item beyond"
    dx = _dev(capi, x0)
    sentinel = -3.5
    rel, iters = np.full((nrhs + 1, max_iter + 1), sentinel), np.full(nrhs + 1, 77, dtype=np.int32)
    ran = raw_solve_many(capi, sm, nrhs, db, dx, rel, iters)
    got = dx.numpy()
    assert ran == max(iters[:nrhs]) and iters[nrhs] == 77 and np.all(rel[nrhs] == sentinel) and np.all(rel[:, ran + 1:] == sentinel)
    for m in range(nrhs):
        h = want[m][3]
        assert iters[m] == len(h) - 1, (m, iters, len(h))
        assert np.array_equal(rel[m, : iters[m] + 1], h), (m, rel[m], h)
        if iters[m] == ran:  # (an item that met tol earlier kept being cycled: lockstep)
            assert np.array_equal(got[m], want[m][2]), ("solve x", m)
    assert np.array_equal(got[nrhs:], x0[nrhs:]) and np.array_equal(db.numpy(), b)
    return rel, iters


@pytest.mark.parametrize("name", VCASES, ids=str)
def test_cycle_and_solve_many_equal_the_plain_periodic_handle(capi, name):
    mk_op, mk_rhs, st = cases.SOLVES_PER[name]
    so, b = mk_op(), four_items(mk_rhs)
    sm = capi.Solver(so, max_rhs=4, periodic_batch2d=True, **st)
    s1 = capi.Solver(so, **st)
    try:
        assert sm.max_rhs() == 4 and s1.max_rhs() == 1 and sm.nlevels() == s1.nlevels() > 1
        for x0 in (np.zeros_like(b), _items(b.shape[1:], 5, 900)):
            want = single_results(s1, b, x0, 4)
            rel, iters = check_batch(capi, sm, b, x0, want, 4, sm.max_iter)
            if not x0.any():
                assert iters[0] == iters[1] and np.array_equal(rel[1, 1:], rel[0, 1:])  # from zero, scaling by 0.5 is exact
    finally:
        sm.close()
        s1.close()


@pytest.mark.parametrize("name", FCASES, ids=str)
def test_the_f_cycle_entries_have_no_batch_handle(capi, capfd, name):
    mk_op, _, st = cases.SOLVES_PER[name]
    capfd.readouterr()
    with pytest.raises(RuntimeError):
        capi.Solver(mk_op(), max_rhs=3, periodic_batch2d=True, **st)
    err = capfd.readouterr().err
    assert "cedar_amd_solver_create_many_periodic2" in err and "only the V-cycle" in err


# ------------------------------------------------------------------ 3. level counts, capacity, reuse
@pytest.mark.parametrize("shape,nst,ibc,relax,nlev", [((8, 8), 5, 3, "point", 1), ((130, 8), 5, 2, "point", 2), ((12, 16), 3, 1, "line-xy", 2),
                                                      ((10, 6), 3, 2, "line-y", 1)], ids=str)
def test_one_and_two_level_handles(capi, shape, nst, ibc, relax, nlev):
    nx, ny = shape
    per = PER[ibc]
    so = pb.periodic_random_op(nx, ny, 5, per, 5) if nst == 5 else pb.periodic_poisson2(nx, ny, per)
    st = dict(relax=relax, nrelax_pre=2, nrelax_post=1, ibc=ibc, num_levels=nlev, max_iter=6)
    b = four_items(lambda: pb.periodic_rhs2(nx, ny, per))
    x0 = _items(b.shape[1:], 5, 901)
    sm = capi.Solver(so, max_rhs=3, periodic_batch2d=True, **st)
    s1 = capi.Solver(so, **st)
    try:
        assert sm.nlevels() == nlev == s1.nlevels() and sm.max_rhs() == 3
        check_batch(capi, sm, b, x0, single_results(s1, b, x0, 3), 3, 6)
    finally:
        sm.close()
        s1.close()


@pytest.mark.parametrize("name", ["perrand9_xy_96x80_v21", "perrand9_x_100x75_linexy"])
def test_capacity_reuse_and_reproducibility(capi, name):
    """one max_rhs = 4 handle: nrhs = 4, 1, 3, then the single-vector calls on item 0, then everything again (the
    captured cycles are keyed on the batch count); then a level-1 operator replaced through cedar_amd_solver_set"""
    mk_op, mk_rhs, st = cases.SOLVES_PER[name]
    so, b = mk_op(), four_items(mk_rhs)
    x0 = _items(b.shape[1:], 5, 902)
    sm = capi.Solver(so, max_rhs=4, periodic_batch2d=True, **st)
    s1 = capi.Solver(so, **st)
    try:
        want = single_results(s1, b, x0, 4)
        first = None
        for rnd in range(2):
            outs = []
            for nrhs in (4, 1, 3):
                rel, iters = check_batch(capi, sm, b, x0, want, nrhs, sm.max_iter)
                outs.append((rel.copy(), iters.copy()))
            x = x0[0].copy()
            h = sm.solve(b[0], x)  # the single-vector kernels on item 0
            assert np.array_equal(h, want[0][3]) and np.array_equal(x, want[0][2])
            x = x0[1].copy()
            sm.vcycle(x, b[1])
            assert np.array_equal(x, want[1][0])
            if first is None:
                first = outs
            else:
                for (r0, i0), (r1, i1) in zip(first, outs):
                    assert np.array_equal(r0, r1) and np.array_equal(i0, i1)
        # reuse after set: scale the level-1 operator on both handles; the batch follows the plain handle
        A1 = s1.array(1, "A")
        for s in (s1, sm):
            s.set_array(1, "A", 1.25 * A1)
        want2 = single_results(s1, b, x0, 4)
        assert not np.array_equal(want2[0][0], want[0][0])
        check_batch(capi, sm, b, x0, want2, 4, sm.max_iter)
    finally:
        sm.close()
        s1.close()


# ------------------------------------------------------------------ 4. refusals
def test_refusals(capi, capfd):
    sentinel = -3.5
    new = "cedar_amd_solver_create_many_periodic2"
    so = pb.periodic_random_op(32, 24, 5, (True, False), 3)
    g = so.shape[1:]
    b = np.stack([ps.random_field(g, 1 + m) for m in range(4)])

    def no_handle(text, so_=so, **kw):
        capfd.readouterr()
        with pytest.raises(RuntimeError):
            capi.Solver(so_, **kw)
        err = capfd.readouterr().err
        assert text in err, (text, err)
        return err

    for kw, text in ((dict(ibc=2, max_rhs=2, cycle="f"), "only the V-cycle"), (dict(ibc=2, max_rhs=0), "max_rhs must be 1 .. 32"),
                     (dict(ibc=2, max_rhs=33), "max_rhs must be 1 .. 32"), (dict(ibc=4, max_rhs=2), "boundary codes"),
                     (dict(ibc=-1, max_rhs=2), "boundary codes")):
        assert new in no_handle(text, periodic_batch2d=True, **kw)
    # what cedar_amd_solver_create refuses for a periodic 2D handle (point relaxation, a row of more than 8190 points): its
    # message first, then a line that names the new call
    err = no_handle("periodic boundary conditions are implemented for the definite periodic codes",
                    so_=pb.periodic_poisson2(8191, 3, (True, False)), ibc=2, max_rhs=2, periodic_batch2d=True)
    assert err.index("cedar_amd_solver_create:") < err.index(new)
    # the 3D call keeps turning a 2D operator away
    assert "cedar_amd_solver_create_many_periodic:" in no_handle("3D only", ibc=2, max_rhs=2, periodic_batch=True)

    def refused(call, text, who, rc=-1):
        capfd.readouterr()
        assert call() == rc
        err = capfd.readouterr().err
        assert text in err and who in err, (text, who, err)

    sm = capi.Solver(so, ibc=2, max_rhs=3, periodic_batch2d=True, nrelax_pre=1, nrelax_post=1)
    sp = capi.Solver(so, ibc=2, max_rhs=4, nrelax_pre=1, nrelax_post=1)  # cedar_amd_solver_create_many: one item, _many refused
    try:
        assert sm.max_rhs() == 3 and sp.max_rhs() == 1
        x = np.full_like(b, sentinel)
        rel, it = np.full((4, sm.max_iter + 1), sentinel), np.full(4, 77, dtype=np.int32)
        itp = it.ctypes.data_as(C.POINTER(C.c_int))
        lib = capi.lib
        refused(lambda: lib.cedar_amd_solver_vcycle_many(sm.h, 4, x.ctypes.data, b.ctypes.data), "nrhs exceeds", "cedar_amd_solver_vcycle_many")
        refused(lambda: lib.cedar_amd_solver_solve_many(sm.h, 4, b.ctypes.data, x.ctypes.data, rel.ctypes.data, itp), "nrhs exceeds",
                "cedar_amd_solver_solve_many")
        refused(lambda: lib.cedar_amd_solver_vcycle_many(sm.h, 0, x.ctypes.data, b.ctypes.data), "at least 1", "cedar_amd_solver_vcycle_many")
        refused(lambda: lib.cedar_amd_solver_time_vcycles_many(sm.h, 4, x.ctypes.data, b.ctypes.data, 1), "nrhs exceeds",
                "cedar_amd_solver_time_vcycles_many", rc=-1.0)
        p = capi.PcgSettings(20, 1e-8, 1, 3, 1)
        hist = np.full((4, 21), sentinel)
        for call in ("cedar_amd_solver_pcg_many", "cedar_amd_solver_fcg_many"):
            refused(lambda: getattr(lib, call)(sm.h, 2, b.ctypes.data, x.ctypes.data, C.byref(p), hist.ctypes.data, itp), "periodic boundary conditions", call)
        refused(lambda: lib.cedar_amd_solver_fcg_periodic(sm.h, b.ctypes.data, x.ctypes.data, C.byref(p), hist.ctypes.data), "max_rhs > 1",
                "cedar_amd_solver_fcg_periodic")
        refused(lambda: lib.cedar_amd_solver_fcg_periodic_many(sm.h, 4, b.ctypes.data, x.ctypes.data, C.byref(p), hist.ctypes.data, itp),
                "nrhs exceeds", "cedar_amd_solver_fcg_periodic_many")
        for call in ("cedar_amd_solver_vcycle_many", "cedar_amd_solver_fcg_periodic_many"):
            args = (x.ctypes.data, b.ctypes.data) if call.endswith("vcycle_many") else (b.ctypes.data, x.ctypes.data, C.byref(p), hist.ctypes.data, itp)
            refused(lambda: getattr(lib, call)(sp.h, 2, *args), "periodic boundary conditions (ibc != 0) are not supported", call)
        # every single-precision switch
        for call in ("cedar_amd_solver_use_fp32_operator", "cedar_amd_solver_use_fp32_operator_many", "cedar_amd_solver_use_fp32_operator_all",
                     "cedar_amd_solver_use_fp32_operator_2d", "cedar_amd_solver_use_fp32_operator_lines", "cedar_amd_solver_use_fp32_interpolation"):
            refused(lambda: getattr(lib, call)(sm.h, 0), "not supported", call)
        assert lib.cedar_amd_solver_fp32_levels(sm.h) == 0 and lib.cedar_amd_solver_fp32_interp_levels(sm.h) == 0
        assert np.all(x == sentinel) and np.all(rel == sentinel) and np.all(it == 77) and np.all(hist == sentinel)
        with pytest.raises(RuntimeError):
            sp.vcycle_many(x[:2], b[:2])
        assert np.all(x == sentinel)
        x = np.zeros_like(b[:3])
        rel3, iters = sm.solve_many(b[:3], x)  # the handle stays usable
        assert max(iters) < sm.max_iter and all(r[-1] < 1e-8 for r in rel3)
    finally:
        sm.close()
        sp.close()


def test_kernel_level_refusals(capi, K, capfd):
    g = (6, 8)
    so = pb.periodic_random_op(6, 4, 5, (True, False), 2)
    sor = np.zeros((2,) + g)
    K.setup_recip2(so, sor)
    q0 = _items(g, 2, 3)
    gc = pb.coarse_shape(g)
    ci, qc = np.zeros((8,) + gc), _items(gc, 2, 4)
    lib = capi.lib
    u, P = capi.u, lambda a: a.ctypes.data_as(capi.P)
    II, JJ, IC, JC = u(g[1]), u(g[0]), u(gc[1]), u(gc[0])
    abd, bbd = np.zeros((24, 24)), np.zeros(2 * 24)
    sc = np.zeros((2, 8))

    def calls(nrhs, ibc, nst, null):
        q = q0.copy()
        a = None if null else P(q)
        return q, [
            ("cedar_amd_relax2_gs_periodic_many", lambda: lib.cedar_amd_relax2_gs_periodic_many(nrhs, P(so), P(q0), a, P(sor), II, JJ, nst, UP, ibc)),
            ("cedar_amd_restrict2_periodic_many", lambda: lib.cedar_amd_restrict2_periodic_many(nrhs, a, P(qc), P(ci), II, JJ, IC, JC, ibc)),
            ("cedar_amd_interp_add2_periodic_many", lambda: lib.cedar_amd_interp_add2_periodic_many(nrhs, a, P(qc), P(q0), P(so), P(ci), IC, JC, II, JJ, nst, ibc)),
            ("cedar_amd_solve_cg2_periodic_many", lambda: lib.cedar_amd_solve_cg2_periodic_many(nrhs, a, P(q0), II, JJ, P(abd), P(bbd), u(24), ibc)),
            ("cedar_amd_pcg_direction2_periodic_many", lambda: lib.cedar_amd_pcg_direction2_periodic_many(nrhs, u(3), P(so), P(q0), P(q0), a, P(q0.copy()), II, JJ, nst, ibc, 0, P(sc))),
        ]

    for nrhs, ibc, nst, null, text, skip in ((0, 2, 5, False, "nrhs must be 1 .. 32", ()), (33, 2, 5, False, "nrhs must be 1 .. 32", ()),
                                             (2, 2, 5, True, "NULL", ()), (2, 4, 5, False, "boundary codes", ()), (2, -1, 5, False, "boundary codes", ()),
                                             (2, 0, 5, False, "ibc = 0", ("pcg_direction2",)),  # (the direction pass forwards it)
                                             (2, 2, 4, False, "nstncl must be 3 or 5", ("restrict2", "solve_cg2"))):
        q, cs = calls(nrhs, ibc, nst, null)
        for who, call in cs:
            if any(s in who for s in skip):
                continue
            capfd.readouterr()
            assert call() == -1, (who, text)
            err = capfd.readouterr().err
            assert who in err and text in err, (who, text, err)
            assert np.array_equal(q, q0) and not sc.any()
    # the 3D direction call keeps refusing a 2D stencil
    capfd.readouterr()
    q = q0.copy()
    assert lib.cedar_amd_pcg_direction_periodic_many(2, u(3), P(so), P(q0), P(q0), P(q), P(q0.copy()), II, JJ, u(1), 5, 2, 0, P(sc)) == -1
    assert "nstncl must be 4 or 14" in capfd.readouterr().err and np.array_equal(q, q0)
