"""Several right-hand sides at once on periodic 3D handles (cedar_amd_solver_create_many_periodic; periodic_many3d.hip).

The one rule checked everywhere: item m of a batched result has the bits of the single-vector periodic call on item m
alone (np.array_equal, no tolerance).  Every device array holds one item more than nrhs, and the item beyond must keep
every bit.  The ghost cells of the input vectors are non-zero.

1. The kernels one by one (Kernels.*_periodic_many): the sweep against the oracle's periodic sweep and the single-vector
   drop-in; restriction, interpolation-and-add and the dense coarsest solve against the single-vector drop-ins.  Row
   lengths from the launcher (relax3_gs_per_many): 64 lanes up to 64 pairs (nx <= 128), 128 up to nx = 256, 256 up to 512,
   512 up to 1024, beyond that the single-vector colour launches item by item; odd periodic nx takes that path too.
2. The cycle and the solve on the nine V-cycle entries of cases.SOLVES_PER3 against a plain periodic handle.
3. One- and two-level handles, nrhs 1 / 3 / 4 on one handle, reuse after cedar_amd_solver_set, reproducibility.
4. Refusals.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import cases
import pcg_statement as ps
import problems as pb

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DOWN, UP = cases.DOWN, cases.UP
NRHS = [1, 2, 3, 8]
NMAX = max(NRHS) + 1  # items the arrays hold


@pytest.fixture(scope="module")
def capi():
    from cedar_amd import capi
    assert capi.device_count() >= 1, "no GPU visible"
    return capi


@pytest.fixture(scope="module")
def K(capi):
    return capi.Kernels()


def _grid(nx, ny, nz):
    return (nz + 2, ny + 2, nx + 2)


def _seed(nx, ny, nz, nst, ibc):
    return 7 * nx + 131 * ny + 1009 * nz + 13 * nst + ibc


def _items(g, n, seed, scale=1.0):
    """n vectors drawn with different seeds, ghost cells non-zero"""
    return np.stack([pb.uniform(g, seed + 17 * m, -1, 1) * scale for m in range(n)])


def _dev(capi, a):
    return capi.DeviceArray.from_numpy(np.ascontiguousarray(a))


def periodic_ghosts(g, per):
    m = np.zeros(g, dtype=bool)
    for axis, on in zip((-1, -2, -3), per):
        if on:
            sl = [slice(None)] * 3
            for end in (0, -1):
                sl[axis] = end
                m[tuple(sl)] = True
    return m


# ------------------------------------------------------------------ 1a. the sweep
# (nx, ny, nz, ibc)
SWEEP27 = [(8, 6, 6, 2), (128, 4, 6, 2), (130, 6, 8, 2), (258, 4, 6, 3), (514, 4, 4, 6), (1026, 4, 4, 2), (40, 36, 30, 8),
           (9, 6, 66, 5), (4, 4, 4, 7), (9, 8, 8, 2), (2, 4, 4, 2)]
SWEEP7 = [(6, 130, 8, 1), (34, 32, 36, 6), (4, 5, 4, 5)]
SWEEPS = [(s, 14) for s in SWEEP27] + [(s, 4) for s in SWEEP7]


def _two_sweeps(impl, so, qf, q, sor, ibc):
    """DOWN then UP on one vector, in place; the state after each"""
    out = []
    for ud in (DOWN, UP):
        impl.relax3(so, qf, q, sor, ud, ibc=ibc)
        out.append(q.copy())
    return out


@pytest.mark.parametrize("shape,nst", SWEEPS, ids=str)
def test_relax_periodic_many(capi, K, oracle, shape, nst):
    nx, ny, nz, ibc = shape
    g, per, sd = _grid(nx, ny, nz), pb.per3_of(ibc), _seed(nx, ny, nz, nst, ibc)
    so = pb.periodic_random_op3(nx, ny, nz, nst, per, sd)
    sor = np.zeros((2,) + g)
    oracle.setup_recip3(so, sor)
    qf, q0 = _items(g, NMAX, sd + 1), _items(g, NMAX, sd + 2)
    q0w = pb.wrap3(q0.copy(), per)  # the same items with consistent ghosts
    fixed = ~pb.interior_mask(g) & ~periodic_ghosts(g, per)  # ghost cells of the non-periodic directions
    dso, dsor, dqf = _dev(capi, so), _dev(capi, sor), _dev(capi, qf)
    for start, flags in ((q0, (0,)), (q0w, (0, 1))):
        want = [_two_sweeps(oracle, so, qf[m], start[m].copy(), sor, ibc) for m in range(NMAX - 1)]
        single = [_two_sweeps(K, so, qf[m], start[m].copy(), sor, ibc) for m in range(NMAX - 1)]
        for m in range(NMAX - 1):
            for t in range(2):
                assert np.array_equal(single[m][t], want[m][t]), ("single", shape, nst, m, t)
        for gc in flags:
            for nrhs in NRHS:
                dq = _dev(capi, start)
                for t, ud in enumerate((DOWN, UP)):
                    K.relax3_periodic_many(dso, dqf, dq, dsor, ud, ibc, ghosts_consistent=gc, nrhs=nrhs)
                    got = dq.numpy()
                    for m in range(nrhs):
                        assert np.array_equal(got[m], want[m][t]), (shape, nst, gc, nrhs, m, t, np.max(np.abs(got[m] - want[m][t])))
                        assert np.array_equal(got[m][fixed], start[m][fixed]), ("fixed ghosts", shape, nst, m)
                    assert np.array_equal(got[nrhs:], start[nrhs:]), ("item beyond", shape, nst, gc, nrhs)


# ------------------------------------------------------------------ 1b. the transfers
# the sweep's shapes with even periodic extents and a coarse grid (the interpolation set-up refuses an odd periodic extent;
# a periodic row of two points has no coarser level)
TRANSFERS = [(s, n) for s, n in SWEEPS if s not in ((9, 8, 8, 2), (2, 4, 4, 2))]


@pytest.mark.parametrize("shape,nst", TRANSFERS, ids=str)
def test_transfers_periodic_many(capi, K, shape, nst):
    nx, ny, nz, ibc = shape
    g, per, sd = _grid(nx, ny, nz), pb.per3_of(ibc), _seed(nx, ny, nz, nst, ibc)
    gc = pb.coarse_shape(g)
    so = pb.periodic_random_op3(nx, ny, nz, nst, per, sd)
    ci = np.zeros((26,) + gc)
    K.setup_interp3(so, ci, ibc=ibc)
    assert ci.any()
    r0, qc0 = _items(g, NMAX, sd + 3), _items(gc, NMAX, sd + 4)
    x0, res0 = _items(g, NMAX, sd + 5), _items(g, NMAX, sd + 6)
    xc = pb.wrap3(_items(gc, NMAX, sd + 7), per)
    want = []
    for m in range(NMAX - 1):
        r, qc = r0[m].copy(), qc0[m].copy()
        K.restrict3(r, qc, ci, ibc=ibc)
        x, res = x0[m].copy(), res0[m].copy()
        K.interp_add3(x, xc[m].copy(), so, res, ci, ibc=ibc)
        want.append((r, qc, x, res))
    dso, dci, dxc = _dev(capi, so), _dev(capi, ci), _dev(capi, xc)
    for nrhs in NRHS:
        dr, dqc = _dev(capi, r0), _dev(capi, qc0)
        K.restrict3_periodic_many(dr, dqc, dci, ibc, nrhs=nrhs)
        r, qc = dr.numpy(), dqc.numpy()
        dx, dres = _dev(capi, x0), _dev(capi, res0)
        K.interp_add3_periodic_many(dx, dxc, dso, dres, dci, ibc, nrhs=nrhs)
        x, res = dx.numpy(), dres.numpy()
        assert np.array_equal(dxc.numpy(), xc)
        for m in range(nrhs):
            for name, a, b in zip(("restrict q (refreshed ghosts)", "restrict qc", "interp_add q", "interp_add res"),
                                  (r[m], qc[m], x[m], res[m]), want[m]):
                assert np.array_equal(a, b), (shape, nst, nrhs, m, name)
        for a, a0 in ((r, r0), (qc, qc0), (x, x0), (res, res0)):
            assert np.array_equal(a[nrhs:], a0[nrhs:]), ("item beyond", shape, nst, nrhs)


# ------------------------------------------------------------------ 1c. the coarsest solve
CG_MANY = [("e4x4x4_xyz", 4, 4, 4, 8), ("e5x3x4_xz", 5, 3, 4, 6), ("e6x4x3_xy", 6, 4, 3, 3), ("e8x8x8_xyz", 8, 8, 8, 8),
           ("e2x4x4_x", 2, 4, 4, 2), ("e16x16x8_z", 16, 16, 8, 5)]  # the last: 2048 unknowns, the most a handle may have


@pytest.mark.parametrize("case", CG_MANY, ids=lambda c: c[0])
def test_coarse_solve_periodic_many(capi, K, case):
    name, nx, ny, nz, ibc = case
    n = nx * ny * nz
    sd = cases._seed(name)
    so = pb.periodic_random_op3(nx, ny, nz, 14, pb.per3_of(ibc), sd)
    g = so.shape[1:]
    abd = np.zeros((n, n))
    K.setup_cg3(so, abd, ibc=ibc)
    NI = 9
    # item 0: the vectors of cases.coarse_solve_per3
    q0 = np.stack([pb.uniform(g, sd + 2, -1, 1)] + [pb.uniform(g, sd + 20 + m, -1, 1) for m in range(1, NI)])
    qf = np.stack([pb.uniform(g, sd + 1, -1, 1)] + [pb.uniform(g, sd + 40 + m, -1, 1) for m in range(1, NI)])
    want = []
    for m in range(NI - 1):
        q = q0[m].copy()
        K.solve_cg3(q, qf[m].copy(), abd, ibc=ibc)
        want.append(q)
    if n <= 512:
        ref = cases.coarse_solve_per3(K, case)
        assert np.array_equal(ref["q"], want[0]) and np.array_equal(ref["abd_upper"], abd.T[np.triu_indices(n)])
    dabd = _dev(capi, abd)
    for nrhs in (1, 3, 8):
        dq, dqf = _dev(capi, q0), _dev(capi, qf)
        K.solve_cg3_periodic_many(dq, dqf, dabd, ibc, nrhs=nrhs)
        got = dq.numpy()
        for m in range(nrhs):
            assert np.array_equal(got[m], want[m]), (name, nrhs, m, np.max(np.abs(got[m] - want[m])))
        assert np.array_equal(got[nrhs:], q0[nrhs:]) and np.array_equal(dqf.numpy(), qf), ("untouched", name, nrhs)
    # items do not see each other: the reverse order gives each item the same bits
    dq, dqf = _dev(capi, q0[:8][::-1]), _dev(capi, qf[:8][::-1])
    K.solve_cg3_periodic_many(dq, dqf, dabd, ibc)
    got = dq.numpy()
    for m in range(8):
        assert np.array_equal(got[7 - m], want[m]), (name, "reversed", m)
    assert np.array_equal(dabd.numpy(), abd)


# ------------------------------------------------------------------ 2. the cycle and the solve
VCASES = [k for k, v in cases.SOLVES_PER3.items() if v[2].get("cycle", "v") == "v"]


def raw_vcycle_many(capi, s, nrhs, dx, db):
    return capi.lib.cedar_amd_solver_vcycle_many(s.h, nrhs, dx.ptr, db.ptr)


def raw_solve_many(capi, s, nrhs, db, dx, rel, iters):
    return capi.lib.cedar_amd_solver_solve_many(s.h, nrhs, db.ptr, dx.ptr, rel.ctypes.data, iters.ctypes.data_as(C.POINTER(C.c_int)))


def four_items(mk_rhs):
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


def check_batch(capi, sm, b, x0, want, nrhs, per, max_iter):
    """vcycle_many twice and solve_many on the first nrhs of the five items the arrays hold"""
    db = _dev(capi, b)
    dx = _dev(capi, x0)
    for t in range(2):
        assert raw_vcycle_many(capi, sm, nrhs, dx, db) == 0
        got = dx.numpy()
        for m in range(nrhs):
            assert np.array_equal(got[m], want[m][t]), ("vcycle", t, m, np.max(np.abs(got[m] - want[m][t])))
            assert np.array_equal(got[m], pb.wrap3(got[m].copy(), per)), ("periodic image", t, m)
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
        assert np.array_equal(got[m], pb.wrap3(got[m].copy(), per)), ("periodic image", m)
    assert np.array_equal(got[nrhs:], x0[nrhs:]) and np.array_equal(db.numpy(), b)
    return rel, iters


@pytest.mark.parametrize("name", VCASES, ids=str)
def test_cycle_and_solve_many_equal_the_plain_periodic_handle(capi, name):
    mk_op, mk_rhs, st = cases.SOLVES_PER3[name]
    so, b = mk_op(), four_items(mk_rhs)
    per = pb.per3_of(st["ibc"])
    sm = capi.Solver(so, max_rhs=4, periodic_batch=True, **st)
    s1 = capi.Solver(so, **st)
    try:
        assert sm.max_rhs() == 4 and s1.max_rhs() == 1 and sm.nlevels() == s1.nlevels()
        for x0 in (np.zeros_like(b), _items(b.shape[1:], 5, 900)):
            want = single_results(s1, b, x0, 4)
            rel, iters = check_batch(capi, sm, b, x0, want, 4, per, sm.max_iter)
            if not x0.any():
                assert iters[0] == iters[1] and np.array_equal(rel[1, 1:], rel[0, 1:])  # from zero, scaling by 0.5 is exact
                gold_all = json.load(open(os.path.join(HERE, "golden", "solves_periodic3d.json")))
                if name in gold_all:  # per_z: the reference's kernels driven end to end
                    gold = gold_all[name]
                    wanth = [float(gold["res0_l2"])] + [float(v) for v in gold["rel_l2"]]
                    h = rel[0, : iters[0] + 1]
                    assert len(h) == len(wanth)
                    np.testing.assert_allclose(h, wanth, rtol=1e-10, atol=1e-14)
    finally:
        sm.close()
        s1.close()


# ------------------------------------------------------------------ 3. level counts, capacity, reuse
@pytest.mark.parametrize("shape,nst,ibc,nlev", [((8, 8, 8), 14, 8, 1), ((130, 8, 8), 14, 2, 2), ((12, 8, 16), 4, 5, 1)], ids=str)
def test_one_and_two_level_handles(capi, shape, nst, ibc, nlev):
    nx, ny, nz = shape
    per = pb.per3_of(ibc)
    so = pb.periodic_random_op3(nx, ny, nz, nst, per, 5) if nst == 14 else pb.periodic_poisson3(nx, ny, nz, per)
    st = dict(nrelax_pre=2, nrelax_post=1, ibc=ibc, num_levels=nlev, max_iter=6)
    b = four_items(lambda: pb.periodic_rhs3(nx, ny, nz, per))
    x0 = _items(b.shape[1:], 5, 901)
    sm = capi.Solver(so, max_rhs=3, periodic_batch=True, **st)
    s1 = capi.Solver(so, **st)
    try:
        assert sm.nlevels() == nlev == s1.nlevels()
        check_batch(capi, sm, b, x0, single_results(s1, b, x0, 3), 3, per, 6)
    finally:
        sm.close()
        s1.close()


def test_capacity_reuse_and_reproducibility(capi):
    """one max_rhs = 4 handle: nrhs = 4, 1, 3, then the single-vector calls on item 0, then everything again (the
    captured cycles are keyed on the batch count); then a level-1 operator replaced through cedar_amd_solver_set"""
    name = "perrand27_xz_32x20x24_v21"
    mk_op, mk_rhs, st = cases.SOLVES_PER3[name]
    so, b = mk_op(), four_items(mk_rhs)
    per = pb.per3_of(st["ibc"])
    x0 = _items(b.shape[1:], 5, 902)
    sm = capi.Solver(so, max_rhs=4, periodic_batch=True, **st)
    s1 = capi.Solver(so, **st)
    try:
        want = single_results(s1, b, x0, 4)
        first = None
        for rnd in range(2):
            outs = []
            for nrhs in (4, 1, 3):
                rel, iters = check_batch(capi, sm, b, x0, want, nrhs, per, sm.max_iter)
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
        check_batch(capi, sm, b, x0, want2, 4, per, sm.max_iter)
    finally:
        sm.close()
        s1.close()


# ------------------------------------------------------------------ 4. refusals
def test_refusals(capi, capfd):
    sentinel = -3.5
    so = pb.periodic_random_op3(16, 16, 16, 14, (1, 0, 0), 3)
    g = so.shape[1:]
    b = np.stack([ps.random_field(g, 1 + m) for m in range(4)])

    def no_handle(text, so_=so, **kw):
        capfd.readouterr()
        with pytest.raises(RuntimeError):
            capi.Solver(so_, periodic_batch=True, **kw)
        err = capfd.readouterr().err
        assert text in err, (text, err)
        return err

    for kw, text in ((dict(ibc=2, max_rhs=2, cycle="f"), "only the V-cycle"), (dict(ibc=2, max_rhs=2, relax="plane-xy"), "point relaxation"),
                     (dict(ibc=2, max_rhs=0), "max_rhs must be 1 .. 32"), (dict(ibc=2, max_rhs=33), "max_rhs must be 1 .. 32")):
        assert "cedar_amd_solver_create_many_periodic" in no_handle(text, **kw)
    assert "cedar_amd_solver_create_many_periodic" in no_handle("3D only", so_=pb.periodic_poisson2(32, 32, (True, False)), ibc=2, max_rhs=2)
    # what cedar_amd_solver_create refuses for a periodic handle: its message, then the new call's name
    assert "cedar_amd_solver_create_many_periodic" in no_handle("periodic", ibc=4, max_rhs=2)
    assert "cedar_amd_solver_create_many_periodic" in no_handle("even extent", so_=pb.periodic_random_op3(10, 16, 16, 14, (1, 0, 0), 1),
                                                                ibc=2, max_rhs=2)

    def refused(call, text, who):
        capfd.readouterr()
        assert call() == -1
        err = capfd.readouterr().err
        assert text in err and who in err, (text, who, err)

    sm = capi.Solver(so, ibc=2, max_rhs=3, periodic_batch=True, nrelax_pre=1, nrelax_post=1)
    sp = capi.Solver(so, ibc=2, max_rhs=4, nrelax_pre=1, nrelax_post=1)  # the old way: one item, _many refused
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
        p = capi.PcgSettings(20, 1e-8, 1, 3, 1)
        hist = np.full((4, 21), sentinel)
        for call in ("cedar_amd_solver_pcg_many", "cedar_amd_solver_fcg_many"):
            refused(lambda: getattr(lib, call)(sm.h, 2, b.ctypes.data, x.ctypes.data, C.byref(p), hist.ctypes.data, itp), "periodic boundary conditions", call)
        refused(lambda: lib.cedar_amd_solver_fcg_periodic(sm.h, b.ctypes.data, x.ctypes.data, C.byref(p), hist.ctypes.data), "max_rhs > 1",
                "cedar_amd_solver_fcg_periodic")
        refused(lambda: lib.cedar_amd_solver_vcycle_many(sp.h, 2, x.ctypes.data, b.ctypes.data), "periodic boundary conditions (ibc != 0) are not supported",
                "cedar_amd_solver_vcycle_many")
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
    g = _grid(6, 4, 4)
    so = pb.periodic_random_op3(6, 4, 4, 14, (1, 0, 0), 2)
    sor = np.zeros((2,) + g)
    K.setup_recip3(so, sor)
    q0 = _items(g, 2, 3)
    gc = pb.coarse_shape(g)
    ci, qc = np.zeros((26,) + gc), _items(gc, 2, 4)
    lib = capi.lib
    u, P = capi.u, lambda a: a.ctypes.data_as(capi.P)
    II, JJ, KK = u(g[2]), u(g[1]), u(g[0])
    IC, JC, KC = u(gc[2]), u(gc[1]), u(gc[0])
    abd, bbd = np.zeros((96, 96)), np.zeros(2 * 96)

    def calls(nrhs, ibc, nst, null):
        q = q0.copy()
        a = None if null else P(q)
        return q, [
            ("cedar_amd_relax3_gs_periodic_many", lambda: lib.cedar_amd_relax3_gs_periodic_many(nrhs, P(so), P(q0), a, P(sor), II, JJ, KK, nst, UP, ibc, 0)),
            ("cedar_amd_restrict3_periodic_many", lambda: lib.cedar_amd_restrict3_periodic_many(nrhs, a, P(qc), P(ci), II, JJ, KK, IC, JC, KC, ibc)),
            ("cedar_amd_interp_add3_periodic_many", lambda: lib.cedar_amd_interp_add3_periodic_many(nrhs, a, P(qc), P(so), P(q0), P(ci), IC, JC, KC, II, JJ, KK, nst, ibc)),
            ("cedar_amd_solve_cg3_periodic_many", lambda: lib.cedar_amd_solve_cg3_periodic_many(nrhs, a, P(q0), II, JJ, KK, P(abd), P(bbd), u(96), ibc)),
        ]

    for nrhs, ibc, nst, null, text, skip in ((0, 2, 14, False, "nrhs must be 1 .. 32", ()), (33, 2, 14, False, "nrhs must be 1 .. 32", ()),
                                             (2, 2, 14, True, "NULL", ()), (2, 4, 14, False, "boundary code", ()),
                                             (2, 2, 5, False, "nstncl must be 4 or 14", ("restrict3", "solve_cg3"))):
        q, cs = calls(nrhs, ibc, nst, null)
        for who, call in cs:
            if any(s in who for s in skip):
                continue  # (no stencil argument)
            capfd.readouterr()
            assert call() == -1, (who, text)
            err = capfd.readouterr().err
            assert who in err and text in err, (who, text, err)
            assert np.array_equal(q, q0)
