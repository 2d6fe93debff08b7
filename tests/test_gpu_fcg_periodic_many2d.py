"""Flexible CG on a periodic 2D batch (cedar_amd_solver_fcg_periodic_many on a handle of
cedar_amd_solver_create_many_periodic2) and its wrap-around direction pass on several items (krylov.hip
pcg_dir2_per_many through cedar_amd_pcg_direction2_periodic_many).

1. The kernel: item m bit for bit against cedar_amd_pcg_direction_periodic on item m alone and against
   krylov_statement.direction on WRAPPED COPIES, the arrays handed over carrying NaN in every ghost cell of a periodic
   direction.  Integer and real data, first 0 / 1, sigma and alpha bit for bit on integer data, stencils 3 and 5, the 2D
   row lengths of tests/test_gpu_fcg_periodic.py, nrhs in {1, 2, 5, 9}, an `active` mask with holes.  The device arrays
   hold one item more than nrhs.
2. The solver: item m's x, hist row and iters[m] equal Solver.fcg_periodic on item m alone on a plain periodic handle.
3. Freezing, a zero initial residual, precon 1 / 2, the stop tests, ghost independence, forwarding.
"""
import ctypes as C

import numpy as np
import pytest

import cases
import fcg_periodic_statement as fps
import krylov_statement as ks
import pcg_statement as ps
import problems as pb
from test_gpu_fcg_periodic import DIR2, ONE2, cases_of, periodic_ghosts, poisoned
from test_gpu_krylov import direction_data, exact_dot, scalars, shape_of

pytestmark = pytest.mark.gpu
NI = 10  # items the arrays hold: nine at most take part
HOLES = 0b101101011  # items 2, 4, 7 masked


@pytest.fixture(scope="module")
def capi():
    from cedar_amd import capi
    assert capi.device_count() >= 1, "no GPU visible"
    return capi


@pytest.fixture(scope="module")
def K(capi):
    return capi.Kernels()


def _dev(capi, a):
    return capi.DeviceArray.from_numpy(np.ascontiguousarray(a))


# ---------------------------------------------------------------- 1. the kernel
def check_items(capi, K, oracle, g, nst, ibc, integer):
    per = fps.per_of(2, ibc)
    so = direction_data(g, nst, integer, 300 + nst)[0]
    zs, ps_ = [], []
    for m in range(NI):
        _, z, p = direction_data(g, nst, integer, 300 + nst + 7 * m)
        zs.append(poisoned(z, per))
        ps_.append(poisoned(p, per))
    z, p = np.stack(zs), np.stack(ps_)
    betas = [(0.0, 1.0, -2.0, 0.5)[m % 4] if integer else 0.3717 + 0.125 * m for m in range(NI)]
    pn0, w0 = np.stack([pb.uniform(g, 77 + m, 1, 2) for m in range(NI)]), np.stack([pb.uniform(g, 177 + m, 1, 2) for m in range(NI)])
    sc0 = np.stack([scalars(rho=3.0 + m, beta=betas[m]) for m in range(NI)])
    dso, dz, dp = _dev(capi, so), _dev(capi, z), _dev(capi, p)
    for first in (False, True):
        # per item: the statement on wrapped copies, and the single-vector periodic pass
        want = []
        for m in range(NI - 1):
            zw, pw = fps.wrap(z[m].copy(), per), fps.wrap(p[m].copy(), per)
            assert not np.isnan(zw).any() and not np.isnan(pw).any()
            spn, sw = ks.direction(oracle, so, zw, pw, pn0[m], w0[m], betas[m], first)
            pn, w, sc = pn0[m].copy(), w0[m].copy(), sc0[m].copy()
            K.pcg_direction_periodic(so, z[m], np.full(g, np.nan) if first else p[m], pn, w, ibc, first, sc)
            what = (g, nst, ibc, integer, first, m)
            assert np.array_equal(pn, spn) and np.array_equal(w, sw), ("single against the statement", what)
            if integer:
                sigma, _ = exact_dot(spn, sw, True)
                assert np.array_equal(sc, ks.set_alpha(sigma, sc0[m])), (what, sc, sigma)
            want.append((pn, w, sc))
        dp_arg = _dev(capi, np.full_like(p, np.nan)) if first else dp  # first: p is not read
        for nrhs, active in ((1, None), (2, None), (5, None), (9, None), (9, HOLES)):
            dpn, dw, sc = _dev(capi, pn0), _dev(capi, w0), sc0.copy()
            K.pcg_direction2_periodic_many(dso, dz, dp_arg, dpn, dw, ibc, first, sc, nrhs=nrhs, active=active)
            pn, w = dpn.numpy(), dw.numpy()
            for m in range(NI):
                on = m < nrhs and (active is None or (active >> m) & 1)
                what = (g, nst, ibc, integer, first, nrhs, active, m)
                if on:
                    assert np.array_equal(pn[m], want[m][0]), ("pn", what)
                    assert np.array_equal(w[m], want[m][1]), ("w", what, np.nanmax(np.abs(w[m] - want[m][1])))
                    assert np.array_equal(sc[m], want[m][2]), ("sc", what, sc[m], want[m][2])
                else:  # masked or beyond nrhs: outputs and scalar block keep their bits
                    assert np.array_equal(pn[m], pn0[m]) and np.array_equal(w[m], w0[m]) and np.array_equal(sc[m], sc0[m]), ("untouched", what)


@pytest.mark.parametrize("nst", [3, 5])
@pytest.mark.parametrize("ibc,shape", cases_of(DIR2, ONE2, (2, 3), (1, 2, 3)), ids=str)
def test_direction2_periodic_many(capi, K, oracle, ibc, shape, nst):
    for integer in (True, False):
        check_items(capi, K, oracle, shape_of(*shape), nst, ibc, integer)


@pytest.mark.parametrize("shape,nst", [((257, 3), 5), ((3, 2), 3)], ids=str)
def test_direction2_periodic_many_with_ibc_0_is_the_dirichlet_batch(K, shape, nst):
    g = shape_of(*shape)
    so = direction_data(g, nst, False, 950)[0]
    z, p = np.stack([pb.uniform(g, 951 + m, -1, 1) for m in range(3)]), np.stack([pb.uniform(g, 961 + m, -1, 1) for m in range(3)])
    for first in (False, True):
        outs = []
        for call in (lambda pn, w, sc: K.pcg_direction_many(so, z, p, pn, w, first, sc),
                     lambda pn, w, sc: K.pcg_direction2_periodic_many(so, z, p, pn, w, 0, first, sc)):
            pn, w = np.stack([pb.uniform(g, 77, 1, 2)] * 3), np.stack([pb.uniform(g, 78, 1, 2)] * 3)
            sc = np.stack([scalars(rho=3.0, beta=0.3717)] * 3)
            call(pn, w, sc)
            outs.append((pn, w, sc))
        for a, b in zip(*outs):
            assert np.array_equal(a, b), (shape, nst, first)


# ---------------------------------------------------------------- 2. the solver
VCASES = [k for k, v in cases.SOLVES_PER.items() if v[2].get("cycle", "v") == "v"]


def raw_many(capi, s, nrhs, db, dx, hist, iters, **kw):
    p = capi.PcgSettings(kw.get("max_iter", 40), kw.get("tol", 1e-10), kw.get("stop_test", capi.PCG_STOP[kw.get("stop", "rel_l2")]),
                         capi.PCG_PRECON[kw.get("precon", "mg")], kw.get("nmg_cycles", 1))
    ptr = lambda a: a.ptr if isinstance(a, capi.DeviceArray) else (None if a is None else a.ctypes.data)
    return capi.lib.cedar_amd_solver_fcg_periodic_many(s.h, nrhs, ptr(db), ptr(dx), C.byref(p), hist.ctypes.data,
                                                       iters.ctypes.data_as(C.POINTER(C.c_int)))


def check_solver(capi, sm, s1, b, x0, nrhs, **kw):
    """b, x0: nrhs + 1 items; the first nrhs against fcg_periodic per item on the plain handle s1.  Returns iters, hist"""
    max_iter = kw.get("max_iter", 40)
    sentinel = -3.5
    db, dx = _dev(capi, b), _dev(capi, x0)
    hist, iters = np.full((nrhs + 1, max_iter + 1), sentinel), np.full(nrhs + 1, 77, dtype=np.int32)
    most = raw_many(capi, sm, nrhs, db, dx, hist, iters, **kw)
    got = dx.numpy()
    per = fps.per_of(2, kw["ibc"])
    skw = {k: v for k, v in kw.items() if k != "ibc"}
    for m in range(nrhs):
        x = x0[m].copy()
        h = s1.fcg_periodic(b[m], x, **skw)
        assert iters[m] == len(h) - 1, (m, iters, len(h))
        assert np.array_equal(hist[m, : len(h)], h), (m, hist[m], h)
        assert np.all(hist[m, len(h):] == sentinel), m
        assert np.array_equal(got[m], x), (m, np.max(np.abs(got[m] - x)))
        assert np.array_equal(got[m], fps.wrap(got[m].copy(), per)), ("periodic image", m)
    assert most == max(iters[:nrhs]) and iters[nrhs] == 77 and np.all(hist[nrhs] == sentinel)
    assert np.array_equal(got[nrhs], x0[nrhs]) and np.array_equal(db.numpy(), b)
    return [int(v) for v in iters[:nrhs]], hist


def handles(capi, name, max_rhs=3):
    mk_op, _, st = cases.SOLVES_PER[name]
    so = mk_op()
    return so, st, capi.Solver(so, max_rhs=max_rhs, periodic_batch2d=True, **st), capi.Solver(so, **st)


@pytest.mark.parametrize("name", VCASES, ids=str)
def test_fcg_periodic_many_equals_fcg_periodic_per_item(capi, name):
    so, st, sm, s1 = handles(capi, name)
    g = so.shape[1:]
    try:
        b17 = ps.random_field(g, 17)
        b = np.stack([b17, ps.random_field(g, 19), 0.75 * b17, pb.uniform(g, 29, -1, 1)])
        x0 = np.stack([ps.random_field(g, 23)] * 3 + [pb.uniform(g, 30, -1, 1)])
        iters, hist = check_solver(capi, sm, s1, b, x0, 3, ibc=st["ibc"], tol=1e-10, max_iter=40)
        print(name, iters)
        assert all(1 <= n < 40 for n in iters) and all(hist[m, iters[m]] < 1e-10 for m in range(3))
        iters2, hist2 = check_solver(capi, sm, s1, b, x0, 3, ibc=st["ibc"], tol=1e-10, max_iter=40)  # and again
        assert iters2 == iters and np.array_equal(hist2, hist)
        # nrhs == 1 runs the single-vector path itself
        check_solver(capi, sm, s1, b[1:3], x0[1:3], 1, ibc=st["ibc"], tol=1e-10, max_iter=40)
    finally:
        sm.close()
        s1.close()


# ---------------------------------------------------------------- 3. the rules of the loop
POINT5, RAND9, LINEXY = "perpoisson5_y_128x96_v21", "perrand9_xy_96x80_v21", "perrand9_x_100x75_linexy"


def test_items_that_stop_at_different_iterations_are_frozen(capi):
    """absolute stop test, right-hand sides scaled by exact powers of two, x0 = 0: the smaller the item the sooner it
    stops; one item with b = A x0 (both zero): zero initial residual, nothing done"""
    so, st, sm, s1 = handles(capi, POINT5, max_rhs=4)
    g = so.shape[1:]
    try:
        b0 = ps.random_field(g, 17)
        tol = 1e-6 * np.linalg.norm(ps.inner(b0))
        b = np.stack([b0, b0 / 1024.0, np.zeros(g), b0 / 32.0, pb.uniform(g, 29, -1, 1)])
        x0 = np.zeros_like(b)
        x0[4] = pb.uniform(g, 30, -1, 1)
        iters, hist = check_solver(capi, sm, s1, b, x0, 4, ibc=st["ibc"], tol=tol, stop="abs_l2", max_iter=40)
        print(iters)
        assert iters[2] == 0 and hist[2, 0] == 0.0
        assert iters[1] < iters[3] < iters[0], iters
    finally:
        sm.close()
        s1.close()


@pytest.mark.parametrize("precon", ["none", "diag"])
def test_fcg_periodic_many_without_the_cycle(capi, precon):
    """precon 1 | 2: the standard recurrence, as fcg_periodic runs it (diagonally dominant operator: CG alone converges)"""
    so, st, sm, s1 = handles(capi, RAND9)
    g = so.shape[1:]
    try:
        b = np.stack([ps.random_field(g, 17), ps.random_field(g, 19), 2.0 * ps.random_field(g, 17), pb.uniform(g, 29, -1, 1)])
        x0 = np.stack([ps.random_field(g, 23)] * 3 + [pb.uniform(g, 30, -1, 1)])
        iters, hist = check_solver(capi, sm, s1, b, x0, 3, ibc=st["ibc"], tol=1e-10, max_iter=60, precon=precon)
        assert all(2 < n < 60 for n in iters), iters
    finally:
        sm.close()
        s1.close()


@pytest.mark.parametrize("stop", ["abs_l2", "rel_l2", "abs_m", "rel_m"])
@pytest.mark.parametrize("name", [POINT5, LINEXY])
def test_fcg_periodic_many_stop_tests(capi, name, stop):
    so, st, sm, s1 = handles(capi, name)
    g = so.shape[1:]
    try:
        b = np.stack([ps.random_field(g, 17), ps.random_field(g, 19), 0.5 * ps.random_field(g, 17), pb.uniform(g, 29, -1, 1)])
        x0 = np.zeros_like(b)
        x0[3] = pb.uniform(g, 30, -1, 1)
        tol = 1e-9 if stop.startswith("rel") else 1e-9 * np.linalg.norm(ps.inner(b[0]))
        iters, _ = check_solver(capi, sm, s1, b, x0, 3, ibc=st["ibc"], tol=tol, stop=stop, max_iter=50)
        assert all(1 <= n < 50 for n in iters), iters
    finally:
        sm.close()
        s1.close()


@pytest.mark.parametrize("name", ["perpoisson5_x_200x60_linex", RAND9])
def test_ghost_layers_of_x_and_b_do_not_matter(capi, name):
    """b: NaN in every ghost cell (none is read).  x: NaN in the ghost cells of the periodic directions -- every item is
    wrapped before the first residual; the ghost layer of a Dirichlet side is the boundary value (zero)"""
    so, st, sm, s1 = handles(capi, name)
    s1.close()
    g = so.shape[1:]
    per = fps.per_of(2, st["ibc"])
    try:
        inner = pb.interior_mask(g)
        b = np.stack([ps.random_field(g, 17), ps.random_field(g, 19), ps.random_field(g, 21)])
        x0 = np.stack([ps.random_field(g, 23), ps.random_field(g, 25), np.zeros(g)]) * inner
        bg, xg = b.copy(), x0.copy()
        bg[:, ~inner] = np.nan
        xg[:, periodic_ghosts(g, per)] = np.nan
        x, xn = x0.copy(), xg.copy()
        h, it = sm.fcg_periodic_many(b, x, tol=1e-10, max_iter=40)
        hn, itn = sm.fcg_periodic_many(bg, xn, tol=1e-10, max_iter=40)
        assert it == itn and all(np.array_equal(a, c) for a, c in zip(h, hn)) and np.array_equal(x, xn)
        assert not np.isnan(xn).any() and all(r[-1] < 1e-10 for r in h)
    finally:
        sm.close()


def test_a_dirichlet_batch_handle_is_served_by_fcg_many(capi):
    so = pb.varcoef9(45, 38)
    g = so.shape[1:]
    b, x0 = np.stack([ps.random_field(g, 17 + m) for m in range(3)]), np.stack([ps.random_field(g, 23)] * 3)
    for pbatch in (False, True):  # (ibc = 0: the new creation call forwards too)
        s = capi.Solver(so, nrelax_pre=2, nrelax_post=1, max_rhs=3, periodic_batch2d=pbatch)
        try:
            assert s.max_rhs() == 3
            x, xf = x0.copy(), x0.copy()
            h, it = s.fcg_periodic_many(b, x, tol=1e-10, max_iter=40)
            hf, itf = s.fcg_many(b, xf, tol=1e-10, max_iter=40)
            assert it == itf and min(it) > 2 and all(np.array_equal(a, c) for a, c in zip(h, hf)) and np.array_equal(x, xf)
        finally:
            s.close()
