"""GPU tests of several right-hand sides on one resident hierarchy (cedar_amd_solver_*_many, many3d.hip).

The statement is exact: the batched kernels keep the reference's term order and the library is built with
-ffp-contract=off, so item m of any batched result has exactly one correct bit pattern -- that of the single-vector
reference-order computation on item m alone.  Every comparison below is np.array_equal, except the two against the
reference's golden histories, which use the tolerances of test_gpu_solver.test_solve_history_vs_reference_golden.
"""
import numpy as np
import pytest

import cases
import problems as pb

pytestmark = pytest.mark.gpu

DOWN, UP = 0, 1
SHAPES27 = [(70, 9, 8), (130, 6, 7), (258, 5, 6), (512, 20, 9), (257, 34, 8), (3, 3, 3)]
SHAPES7 = [(33, 34, 35), (4, 5, 3)]
KCASES = [(s, 14) for s in SHAPES27] + [(s, 4) for s in SHAPES7]
NRHS = [1, 2, 3, 5, 8]


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


def _seed(shape, nst):
    return 7 * shape[0] + 131 * shape[1] + 1009 * shape[2] + nst


def _items(g, n, seed, scale=1.0):
    """n vectors drawn with different seeds, ghost cells non-zero"""
    return np.stack([pb.uniform(g, seed + 17 * m, -1, 1) * scale for m in range(n)])


def _operator(oracle, shape, nst):
    g = _grid(shape)
    sd = _seed(shape, nst)
    so = pb.random_op(g, nst, sd, zero_ghost=False)
    sor = np.zeros((2,) + g)
    oracle.setup_recip3(so, sor)
    gc = pb.coarse_shape(g)
    ci = np.zeros((26,) + gc)
    oracle.setup_interp3(so, ci)
    return g, gc, sd, so, sor, ci


def _dev(capi, a):
    return capi.DeviceArray.from_numpy(a)


# ------------------------------------------------------------------ 1. kernel by kernel against the oracle
@pytest.mark.parametrize("nrhs", NRHS)
@pytest.mark.parametrize("shape,nst", KCASES, ids=str)
def test_relax_many_vs_oracle(capi, K, oracle, shape, nst, nrhs):
    """two sweeps in a row, both directions; device arrays holding one item more than nrhs"""
    g, _, sd, so, sor, _ = _operator(oracle, shape, nst)
    qf, q0 = _items(g, nrhs + 1, sd + 1), _items(g, nrhs + 1, sd + 2)
    m_in = pb.interior_mask(g)
    for ud in (DOWN, UP):
        dq, dqf = _dev(capi, q0), _dev(capi, qf)
        K.relax3_many(so, dqf, dq, sor, ud, nrhs=nrhs)
        K.relax3_many(so, dqf, dq, sor, ud, nrhs=nrhs)
        got = dq.numpy()
        for m in range(nrhs):
            want = q0[m].copy()
            oracle.relax3(so, qf[m], want, sor, ud)
            oracle.relax3(so, qf[m], want, sor, ud)
            assert np.array_equal(got[m], want), (shape, nst, nrhs, ud, m, np.max(np.abs(got[m] - want)))
            assert np.array_equal(got[m][~m_in], q0[m][~m_in])
        assert np.array_equal(got[nrhs], q0[nrhs]), "the item beyond nrhs was touched"
        assert np.array_equal(dqf.numpy(), qf)


@pytest.mark.parametrize("nrhs", NRHS)
@pytest.mark.parametrize("shape,nst", KCASES, ids=str)
def test_residual_many_vs_oracle(capi, K, oracle, shape, nst, nrhs):
    g, _, sd, so, _, _ = _operator(oracle, shape, nst)
    qf, q = _items(g, nrhs + 1, sd + 1), _items(g, nrhs + 1, sd + 2)
    r0 = _items(g, nrhs + 1, sd + 3)
    dr = _dev(capi, r0)
    K.residual3_many(so, _dev(capi, qf), _dev(capi, q), dr, nrhs=nrhs)
    got = dr.numpy()
    m_in = pb.interior_mask(g)
    for m in range(nrhs):
        want = r0[m].copy()
        oracle.residual3(so, qf[m], q[m], want)
        assert np.array_equal(got[m], want), (shape, nst, nrhs, m, np.max(np.abs(got[m] - want)))
        assert np.array_equal(got[m][~m_in], r0[m][~m_in])
    assert np.array_equal(got[nrhs], r0[nrhs])


@pytest.mark.parametrize("nrhs", NRHS)
@pytest.mark.parametrize("shape,nst", KCASES, ids=str)
def test_restrict_many_vs_oracle(capi, K, oracle, shape, nst, nrhs):
    g, gc, sd, _, _, ci = _operator(oracle, shape, nst)
    q, qc0 = _items(g, nrhs + 1, sd + 4), _items(gc, nrhs + 1, sd + 5)
    dqc = _dev(capi, qc0)
    K.restrict3_many(_dev(capi, q), dqc, ci, nrhs=nrhs)
    got = dqc.numpy()
    mc = pb.interior_mask(gc)
    for m in range(nrhs):
        want = qc0[m].copy()
        oracle.restrict3(q[m], want, ci)
        assert np.array_equal(got[m], want), (shape, nst, nrhs, m, np.max(np.abs(got[m] - want)))
        assert np.array_equal(got[m][~mc], qc0[m][~mc])
    assert np.array_equal(got[nrhs], qc0[nrhs])


@pytest.mark.parametrize("nrhs", NRHS)
@pytest.mark.parametrize("shape,nst", KCASES, ids=str)
def test_interp_add_many_vs_oracle(capi, K, oracle, shape, nst, nrhs):
    """q and the mutated res (res /= so(kp), the reference's side effect) of every item"""
    g, gc, sd, so, _, ci = _operator(oracle, shape, nst)
    q0, res0 = _items(g, nrhs + 1, sd + 6), _items(g, nrhs + 1, sd + 7)
    qc = _items(gc, nrhs + 1, sd + 8) * pb.interior_mask(gc)
    dq, dres = _dev(capi, q0), _dev(capi, res0)
    K.interp_add3_many(dq, _dev(capi, qc), so, dres, ci, nrhs=nrhs)
    gq, gr = dq.numpy(), dres.numpy()
    for m in range(nrhs):
        wq, wr = q0[m].copy(), res0[m].copy()
        oracle.interp_add3(wq, qc[m], so, wr, ci)
        assert np.array_equal(gq[m], wq), (shape, nst, nrhs, m, np.max(np.abs(gq[m] - wq)))
        assert np.array_equal(gr[m], wr), (shape, nst, nrhs, m, np.max(np.abs(gr[m] - wr)))
    assert np.array_equal(gq[nrhs], q0[nrhs]) and np.array_equal(gr[nrhs], res0[nrhs])


# ------------------------------------------------------------------ 2. items do not see each other
@pytest.mark.parametrize("shape,nst", [((258, 5, 6), 14), ((257, 34, 8), 14), ((3, 3, 3), 14), ((33, 34, 35), 4)], ids=str)
def test_items_do_not_see_each_other(K, oracle, shape, nst):
    """item m's bits do not change when the other items are replaced by NaN-free junk scaled by 1e30 and the item
    order is permuted"""
    g, gc, sd, so, sor, ci = _operator(oracle, shape, nst)
    n = 5
    perm = [3, 0, 4, 1, 2]  # new position p holds old item perm[p]

    def run(qf, q, res, qc):
        out = {}
        for ud in (DOWN, UP):
            a = q.copy()
            K.relax3_many(so, qf, a, sor, ud)
            out["relax%d" % ud] = a
        r = np.zeros_like(q)
        K.residual3_many(so, qf, q, r)
        out["residual"] = r
        c = np.zeros_like(qc)
        K.restrict3_many(q, c, ci)
        out["restrict"] = c
        a, rr = q.copy(), res.copy()
        K.interp_add3_many(a, qc * pb.interior_mask(gc), so, rr, ci)
        out["interp_q"], out["interp_res"] = a, rr
        return out

    base_in = [_items(g, n, sd + 1), _items(g, n, sd + 2), _items(g, n, sd + 3), _items(gc, n, sd + 4)]
    base = run(*base_in)
    for m in range(n):
        junk_in = []
        for t, a in enumerate(base_in):
            j = _items(a.shape[1:], n, sd + 100 + t, scale=1e30)
            j[m] = a[m]
            junk_in.append(np.ascontiguousarray(j[perm]))
        got = run(*junk_in)
        pos = perm.index(m)
        for k in base:
            assert np.array_equal(got[k][pos], base[k][m]), (shape, nst, m, k)


# ------------------------------------------------------------------ 3. a cycle and a solve against the single-vector solver
def _rhs_items(mk_rhs, n=3):
    b0 = mk_rhs()
    m = pb.interior_mask(b0.shape)
    return np.stack([b0] + [pb.uniform(b0.shape, 4242 + t, -1, 1) * m * np.max(np.abs(b0)) for t in range(1, n)])


def _check_cycle_and_solve(capi, so, st, b, make_single):
    nrhs = b.shape[0]
    sm = capi.Solver(so, max_rhs=nrhs, **st)
    assert sm.max_rhs() == nrhs
    x = np.zeros_like(b)
    sm.vcycle_many(x, b)
    xs = np.zeros_like(b)
    rel, iters = sm.solve_many(b, xs)
    sm.close()
    s1 = make_single()
    for m in range(nrhs):
        x1 = np.zeros_like(b[m])
        s1.vcycle(x1, b[m])
        assert np.array_equal(x[m], x1), ("vcycle", m, np.max(np.abs(x[m] - x1)))
        x1 = np.zeros_like(b[m])
        h = s1.solve(b[m], x1)
        assert iters[m] == len(h) - 1, (m, iters, len(h))
        assert np.array_equal(rel[m][: iters[m] + 1], h), (m, rel[m], h)
    s1.close()
    assert len(rel[0]) - 1 == max(iters)


@pytest.mark.parametrize("name", ["fe27_40x33x50_v21", "fe27_65_v21", "poisson7_64_v21", "poisson7_65_v21", "fe27_129_v21"], ids=str)
def test_cycle_and_solve_many_equal_the_single_vector_solver(capi, name):
    """no level of these problems reaches the 160 rows at which the single-vector solver switches to partial sums:
    its default path IS the reference order"""
    mk_op, mk_rhs, st = cases.SOLVES[name]
    so = mk_op()
    _check_cycle_and_solve(capi, so, st, _rhs_items(mk_rhs), lambda: capi.Solver(so, **st))


def test_cycle_and_solve_many_on_a_partial_sum_sized_level(capi, monkeypatch):
    """a level with >= 160 rows: the batch runs the reference order there, as a single-vector handle created under
    CEDAR_AMD_PSUM=0 does"""
    so = pb.fe3(24, 176, 12)
    st = dict(relax="point", nrelax_pre=2, nrelax_post=1)
    b = _rhs_items(lambda: pb.rhs3(24, 176, 12))

    def single():
        monkeypatch.setenv("CEDAR_AMD_PSUM", "0")
        return capi.Solver(so, **st)

    _check_cycle_and_solve(capi, so, st, b, single)


def test_levels_with_the_row_interleaved_copy_give_the_same_bits(capi, monkeypatch):
    """a single-vector and a batch handle whose two smoothed 27-point levels keep the row-interleaved solve copy
    (CEDAR_AMD_ILV=1; by default only levels of 320 rows do) against the same pair on the Cedar planes (CEDAR_AMD_ILV=0):
    the copy holds the same doubles, so the cycle, the solve and conjugate gradients (on these V(2,1) handles with the
    diagonal preconditioner, on a V(2,2) pair with the cycle as preconditioner) give the same bits"""
    mk_op, mk_rhs, st = cases.SOLVES["fe27_40x33x50_v21"]
    so, b = mk_op(), _rhs_items(mk_rhs)
    monkeypatch.setenv("CEDAR_AMD_PSUM", "0")
    monkeypatch.delenv("CEDAR_AMD_FRUN", raising=False)

    def handles(ilv, st):
        monkeypatch.setenv("CEDAR_AMD_ILV", ilv)
        s1 = capi.Solver(so, **st)
        monkeypatch.setenv("CEDAR_AMD_ILV", ilv)
        return s1, capi.Solver(so, max_rhs=3, **st)

    def pcg(out, s1, sm, tag, **kw):
        for m in range(3):
            x = np.zeros_like(b[m])
            out[tag, "pcg hist", m], out[tag, "pcg x", m] = s1.pcg(b[m], x, **kw), x
        x = np.zeros_like(b)
        hist, iters = sm.pcg_many(b, x, **kw)
        out[tag, "pcg_many x"], out[tag, "pcg_many iters"] = x, iters
        for m in range(3):
            out[tag, "pcg_many hist", m] = hist[m]

    def run(ilv):
        out = {}
        s1, sm = handles(ilv, st)  # the case's V(2,1) cycle
        for m in range(3):
            x = np.zeros_like(b[m])
            s1.vcycle(x, b[m])
            out["vcycle", m] = x
            x = np.zeros_like(b[m])
            out["solve hist", m], out["solve x", m] = s1.solve(b[m], x), x
        x = np.zeros_like(b)
        sm.vcycle_many(x, b)
        out["vcycle_many"] = x
        x = np.zeros_like(b)
        rel, iters = sm.solve_many(b, x)
        out["solve_many x"], out["solve_many iters"] = x, iters
        for m in range(3):
            out["solve_many hist", m] = rel[m]
        pcg(out, s1, sm, "diag", precon="diag", max_iter=25)  # (the multigrid preconditioner wants a symmetric cycle)
        s1.close()
        sm.close()
        s1, sm = handles(ilv, dict(st, nrelax_post=st["nrelax_pre"]))
        pcg(out, s1, sm, "mg")
        s1.close()
        sm.close()
        return out

    planes, copy = run("0"), run("1")
    assert planes.keys() == copy.keys()
    for k in planes:
        assert np.array_equal(planes[k], copy[k]), k
    for m in range(3):
        assert np.array_equal(copy["vcycle_many"][m], copy["vcycle", m]), m


# ------------------------------------------------------------------ 4. against the reference itself
@pytest.mark.parametrize("name", ["fe27_65_v21", "fe27_40x33x50_v21", "poisson7_65_v21"], ids=str)
def test_solve_many_history_vs_reference_golden(capi, golden, name):
    mk_op, mk_rhs, st = cases.SOLVES[name]
    gold = golden["solves"][name]
    b = _rhs_items(mk_rhs)
    s = capi.Solver(mk_op(), max_rhs=3, **st)
    rel, iters = s.solve_many(b, np.zeros_like(b))
    s.close()
    want = [float(gold["res0_l2"])] + [float(v) for v in gold["rel_l2"]]
    h = rel[0][: iters[0] + 1]
    assert len(h) == len(want)
    np.testing.assert_allclose(h, want, rtol=1e-10, atol=cases.HIST_ATOL.get(name, 1e-14))


# ------------------------------------------------------------------ 5. lockstep rules
def test_lockstep_rules(capi):
    """the smooth right-hand side (7 cycles to 1e-8 in the CPU restatement of the reference, its sixth entry 5.7e-8),
    a random one (6 cycles) and a zero item"""
    n = (40, 33, 50)
    so, st = pb.fe3(*n), dict(relax="point", nrelax_pre=2, nrelax_post=1, max_iter=12, tol=1e-8)
    b = _rhs_items(lambda: pb.rhs3(*n))
    b[2] = 0.0
    s = capi.Solver(so, max_rhs=3, **st)
    x = np.zeros_like(b)
    sentinel = -7.25
    rel_buf = np.full((3, st["max_iter"] + 1), sentinel)
    rel, iters = s.solve_many(b, x, rel=rel_buf)
    s.close()
    ran = len(rel[0]) - 1
    s1 = capi.Solver(so, **st)
    single = []
    for m in range(2):
        x1 = np.zeros_like(b[m])
        single.append(s1.solve(b[m], x1))
        assert iters[m] == len(single[m]) - 1
        assert np.array_equal(rel[m][: iters[m] + 1], single[m])
    s1.close()
    assert iters[0] != iters[1], iters  # the two items converge at different speeds, as the single solves do
    assert iters[2] == 0 and np.array_equal(rel[2], np.zeros(ran + 1))
    assert np.array_equal(x[2], np.zeros_like(x[2]))
    assert ran == max(iters) and 0 < ran < st["max_iter"]
    assert np.all(rel_buf[:, ran + 1:] == sentinel)
    # lockstep: the item that met tol first kept being cycled, its row kept being written
    early = int(np.argmin(iters[:2]))
    assert np.all(rel_buf[early, iters[early] + 1: ran + 1] != sentinel)
    assert np.all(rel_buf[early, iters[early]: ran + 1] < st["tol"])


# ------------------------------------------------------------------ 6. capacity and reuse
def test_capacity_and_reuse(capi):
    """one max_rhs = 4 handle: nrhs = 4, then 2, then the plain solve, on device arrays (the captured cycles are keyed
    on the batch count); everything twice"""
    mk_op, mk_rhs, st = cases.SOLVES["fe27_65_v21"]
    so = mk_op()
    b = _rhs_items(mk_rhs, 4)
    s1 = capi.Solver(so, **st)
    want_h, want_x = [], []
    for m in range(4):
        x1 = np.zeros_like(b[m])
        want_h.append(s1.solve(b[m], x1))
        want_x.append(x1)
    s1.close()
    s = capi.Solver(so, max_rhs=4, **st)
    assert s.max_rhs() == 4
    db4, dx4 = capi.DeviceArray.from_numpy(b), capi.DeviceArray(b.shape)
    db2, dx2 = capi.DeviceArray.from_numpy(b[:2]), capi.DeviceArray(b[:2].shape)
    db1, dx1 = capi.DeviceArray.from_numpy(b[0]), capi.DeviceArray(b[0].shape)
    for rep in range(2):
        for nrhs, db, dx in ((4, db4, dx4), (2, db2, dx2)):
            dx.zero()
            rel, iters = s.solve_many(db, dx)
            got = dx.numpy()
            for m in range(nrhs):
                assert iters[m] == len(want_h[m]) - 1
                assert np.array_equal(rel[m][: iters[m] + 1], want_h[m]), (rep, nrhs, m)
                if iters[m] == max(iters):  # (an item that met tol earlier was cycled further than its single solve)
                    assert np.array_equal(got[m], want_x[m]), (rep, nrhs, m)
        dx1.zero()
        h = s.solve(db1, dx1)
        assert np.array_equal(h, want_h[0]) and np.array_equal(dx1.numpy(), want_x[0]), rep
    s.close()


# ------------------------------------------------------------------ 7. refusals
def test_refusals(capi, capfd):
    so3, b3 = pb.fe3(17, 17, 17), pb.rhs3(17, 17, 17)
    so2p, b2p = pb.periodic_poisson2(32, 32, (True, False)), pb.periodic_rhs2(32, 32, (True, False))
    sentinel = -3.5

    def refused(s, b, nrhs, text):
        bb = np.stack([b] * max(nrhs, 1))
        x = np.full_like(bb, sentinel)
        rel = np.full((bb.shape[0], s.max_iter + 1), sentinel)
        it = np.full(bb.shape[0], 77, dtype=np.int32)
        import ctypes as C
        capfd.readouterr()
        rc = capi.lib.cedar_amd_solver_solve_many(s.h, nrhs, bb.ctypes.data, x.ctypes.data, rel.ctypes.data,
                                                  it.ctypes.data_as(C.POINTER(C.c_int)))
        assert rc == -1 and text in capfd.readouterr().err
        assert np.all(x == sentinel) and np.all(rel == sentinel) and np.all(it == 77)
        rc = capi.lib.cedar_amd_solver_vcycle_many(s.h, nrhs, x.ctypes.data, bb.ctypes.data)
        assert rc == -1 and text in capfd.readouterr().err
        assert np.all(x == sentinel)
        if nrhs >= 1:
            with pytest.raises(RuntimeError):
                s.solve_many(bb, x)
            assert np.all(x == sentinel)

    s = capi.Solver(so3, max_rhs=2)
    refused(s, b3, 0, "nrhs must be at least 1")
    refused(s, b3, 3, "exceeds the handle's max_rhs")
    bb = np.stack([b3, b3])
    x = np.zeros_like(bb)
    rel, iters = s.solve_many(bb, x)  # the handle remains usable
    s1 = capi.Solver(so3)
    x1 = np.zeros_like(b3)
    h = s1.solve(b3, x1)
    s1.close()
    s.close()
    assert np.array_equal(rel[0], h) and np.array_equal(rel[1], h) and np.array_equal(x[0], x1) and np.array_equal(x[1], x1)

    for kw, so, b, text in ((dict(ibc=2, nrelax_pre=1, nrelax_post=1), so2p, b2p, "periodic"), (dict(cycle="f"), so3, b3, "V-cycle"),
                            (dict(relax="plane-xy"), so3, b3, "plane relaxation")):
        s = capi.Solver(so, max_rhs=2, **kw)
        assert s.max_rhs() == 1
        refused(s, b, 1, text)
        refused(s, b, 2, text)
        x = np.zeros_like(b)
        h = s.solve(b, x)  # the single-vector entry points serve such a handle as before
        assert len(h) >= 2 and np.all(np.isfinite(h)) and h[-1] < 1.0
        s.close()

    for bad in (0, 33):
        capfd.readouterr()
        with pytest.raises(RuntimeError):
            capi.Solver(so3, max_rhs=bad)
        assert "max_rhs must be 1 .. 32" in capfd.readouterr().err


# ------------------------------------------------------------------ 8. 2D wiring
@pytest.mark.parametrize("name", ["varcoef9_200x120_v21", "poisson5_400_v11"], ids=str)
def test_2d_point_items_equal_the_single_vector_solve(capi, name):
    mk_op, mk_rhs, st = cases.SOLVES[name]
    so = mk_op()
    _check_cycle_and_solve(capi, so, st, _rhs_items(mk_rhs), lambda: capi.Solver(so, **st))


def test_2d_line_relaxation_batch(capi, golden):
    """line relaxation takes the transposed-array path in a batch handle: compare nrhs = 3 against the same kind of
    handle with nrhs = 1 per item, and row 0 against the reference's history"""
    name = "aniso9_512_linexy"
    mk_op, mk_rhs, st = cases.SOLVES[name]
    so, b = mk_op(), _rhs_items(mk_rhs)
    s = capi.Solver(so, max_rhs=3, **st)
    x = np.zeros_like(b)
    rel, iters = s.solve_many(b, x)
    ran = max(iters)
    for m in range(3):
        x1 = np.zeros_like(b[m: m + 1])
        r1, i1 = s.solve_many(b[m: m + 1], x1)
        assert i1[0] == iters[m] and np.array_equal(r1[0], rel[m][: i1[0] + 1]), m
        if iters[m] == ran:
            assert np.array_equal(x1[0], x[m]), m
    s.close()
    gold = golden["solves"][name]
    want = [float(gold["res0_l2"])] + [float(v) for v in gold["rel_l2"]]
    h = rel[0][: iters[0] + 1]
    assert len(h) == len(want)
    np.testing.assert_allclose(h, want, rtol=1e-10, atol=cases.HIST_ATOL.get(name, 1e-14))
