"""Conjugate gradients on several right-hand sides at once (cedar_amd_solver_pcg_many, the *_many kernels of krylov.hip).

The statement is exact.  The batched passes keep the single passes' operation order and summation geometry per item and
the library is built with -ffp-contract=off, so every vector and every scalar of item m has one correct bit pattern:
the one the single-vector pass (or solve) gives on item m alone.  Every comparison below is np.array_equal, except
section 6, which compares with the numpy statement through the tolerances of tests/test_gpu_pcg.py (imported).
"""
import ctypes as C

import numpy as np
import pytest

import cases
import krylov_statement as ks
import pcg_statement as ps
import problems as pb
from test_gpu_krylov import ALPHAS, BETAS, direction_data, exact_dot, ints, scalars, shape_of, update_data
from test_gpu_many import _rhs_items
from test_gpu_pcg import PARITY, SLOW, compare_hist

pytestmark = pytest.mark.gpu

NRHS = [1, 2, 3, 5, 8]
REAL_BETAS = [0.3717, 0.0, -1.25, 0.77, 0.5, -0.3, 1.5, 0.1, 0.9]
REAL_ALPHAS = [-0.4142, 0.0, 0.73, 1.9, -0.01, 0.3, 2.5, -1.1, 0.6]


@pytest.fixture(scope="module")
def capi():
    from cedar_amd import capi
    assert capi.device_count() >= 1, "no GPU visible"
    return capi


@pytest.fixture(scope="module")
def K(capi):
    return capi.Kernels()


def dev(capi, a):
    return None if a is None else capi.DeviceArray.from_numpy(a)


def blocks(n, **per_item):
    """n scalar blocks with the marks of test_gpu_krylov.scalars; per_item: slot name -> list of values"""
    return np.stack([scalars(**{k: v[m] for k, v in per_item.items()}) for m in range(n)])


def stack(make, n, seed):
    return np.stack([make(seed + 31 * m) for m in range(n)])


# ---------------------------------------------------------------- 1 + 2. the passes, item by item
# 27-point: 64 / 128 / 256 lanes, odd nx (half pair), a row of more than 512 points (two trips: the item-by-item route);
# 7-point: 64 / 128 / 256 lanes and a second trip; 2D: several workgroups per row
DIR = [((63, 5, 6), 14), ((129, 6, 5), 14), ((258, 5, 6), 14), ((255, 18, 7), 14), ((600, 5, 4), 14),
       ((64, 5, 6), 4), ((65, 18, 7), 4), ((600, 5, 6), 4), ((257, 40), 5), ((600, 9), 3), ((1030, 7), 5)]


def operator_views(capi, K, monkeypatch, so, g, nst):
    """[host planes] and, for a 27-point operator, the registered device operator with its row-interleaved copy"""
    if nst != 14:
        return [so], lambda: None
    monkeypatch.setenv("CEDAR_AMD_ILV", "1")  # a solve copy at any size
    capi.lib.cedar_amd_relax3_prepare.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint]
    so_d, sor_d = capi.DeviceArray.from_numpy(so), capi.DeviceArray((2,) + g)
    K.setup_recip3(so_d, sor_d)
    assert capi.lib.cedar_amd_relax3_prepare(so_d.ptr, sor_d.ptr, g[2], g[1], g[0]) & 1

    def done():
        so_d.free()
        sor_d.free()
    return [so, so_d], done


def direction_inputs(g, nst, integer, n, seed):
    so = direction_data(g, nst, integer, seed)[0]
    mk = (lambda s: ints(g, s, -8, 8)) if integer else (lambda s: pb.uniform(g, s, -1, 1))
    z, p = stack(mk, n, seed + 1), stack(mk, n, seed + 2)
    pn0, w0 = stack(lambda s: pb.uniform(g, s, 1, 2), n, seed + 3), stack(lambda s: pb.uniform(g, s, 1, 2), n, seed + 4)
    betas = [(BETAS if integer else REAL_BETAS)[m % (4 if integer else 9)] for m in range(n)]
    return so, z, p, pn0, w0, betas


def check_direction_many(capi, K, oracle, so_arg, so, z, p, pn0, w0, betas, first, integer, nrhs, active=None):
    """item m < nrhs with its bit set: the statement's arrays; on integer data the one correct scalar block, on real data
    the block the single-vector pass leaves for item m alone.  Everything else untouched."""
    n = z.shape[0]
    sc0 = blocks(n, rho=[3.0 + m for m in range(n)], beta=betas)
    dpn, dw, sc = dev(capi, pn0), dev(capi, w0), sc0.copy()
    p_arg = np.full(z.shape, np.nan) if first else p  # first: p is not read
    K.pcg_direction_many(so_arg, dev(capi, z), dev(capi, p_arg), dpn, dw, first, sc, nrhs=nrhs, active=active)
    pn, w = dpn.numpy(), dw.numpy()
    act = (1 << nrhs) - 1 if active is None else active
    for m in range(n):
        what = (z.shape, m, nrhs, first, integer, betas[m], type(so_arg).__name__)
        if m >= nrhs or not (act >> m) & 1:
            assert np.array_equal(pn[m], pn0[m]) and np.array_equal(w[m], w0[m]) and np.array_equal(sc[m], sc0[m]), ("touched", what)
            continue
        want_pn, want_w = ks.direction(oracle, so, z[m], p[m], pn0[m], w0[m], betas[m], first)
        assert np.array_equal(pn[m], want_pn), ("pn", what)
        assert np.array_equal(w[m], want_w), ("w", what, np.max(np.abs(w[m] - want_w)))
        if integer:
            sigma, _ = exact_dot(want_pn, want_w, True)
            assert np.array_equal(sc[m], ks.set_alpha(sigma, sc0[m])), (what, sc[m], sigma)
        else:
            pn1, w1, sc1 = pn0[m].copy(), w0[m].copy(), sc0[m].copy()
            K.pcg_direction(so, z[m], p_arg[m], pn1, w1, first, sc1)
            assert np.array_equal(sc[m], sc1), (what, sc[m], sc1)
            assert np.array_equal(pn[m], pn1) and np.array_equal(w[m], w1), what
    return pn, w, sc


@pytest.mark.parametrize("integer", [True, False], ids=["int", "real"])
@pytest.mark.parametrize("shape,nst", DIR, ids=str)
def test_direction_many_item_by_item(capi, K, oracle, monkeypatch, shape, nst, integer):
    g = shape_of(*shape)
    for nrhs in NRHS:
        so, z, p, pn0, w0, betas = direction_inputs(g, nst, integer, nrhs + 1, 1300 + nst + nrhs)
        views, done = operator_views(capi, K, monkeypatch, so, g, nst)
        try:
            outs = []
            for so_arg in views:
                for first in (False, True):
                    outs.append(check_direction_many(capi, K, oracle, so_arg, so, z, p, pn0, w0, betas, first, integer, nrhs))
            for a, b in zip(outs[:2], outs[2:]):  # the two operator views agree in every bit
                assert all(np.array_equal(u, v) for u, v in zip(a, b))
        finally:
            done()


UPD = [(5, 2100), (600, 9), (1030, 7), (7, 50, 47), (129, 6, 5), (600, 5, 4)]


def update_inputs(g, integer, n, seed):
    per = [update_data(g, integer, seed + 53 * m) for m in range(n)]
    x, r, p, w, z = (np.stack([per[m][0][t] for m in range(n)]) for t in range(5))
    diag = per[0][1]  # shared by the items, like the operator
    alphas = [0.0 if m == 1 else (ALPHAS[m % 3] if integer else REAL_ALPHAS[m % 9]) for m in range(n)]
    if n > 1:  # item 1 has alpha = 0 with infinities and NaN in p and w: the breakdown rule, x and r untouched
        p[1].ravel()[::7], p[1].ravel()[3::11] = np.inf, np.nan
        w[1].ravel()[::5], w[1].ravel()[2::13] = -np.inf, np.nan
    return x, r, p, w, z, diag, alphas


def check_update_many(capi, K, g, data, zmode, move, first, integer, nrhs, active=None):
    x, r, p, w, zin, diag, alphas = data
    n = r.shape[0]
    zmark = stack(lambda s: pb.uniform(g, s, 1, 2), n, 79)
    z0 = zin if zmode == 2 else zmark if zmode == 1 else None
    sc0 = blocks(n, rho=[5.0 + m for m in range(n)], alpha=alphas)
    a = (x, p, w) if move else (None, None, None)
    dx, dr, dz, sc = dev(capi, a[0]), dev(capi, r), dev(capi, z0), sc0.copy()
    K.pcg_update_many(zmode, move, dx, dr, dev(capi, a[1]), dev(capi, a[2]), dz, diag if zmode == 1 else None, first, sc,
                      nrhs=nrhs, active=active)
    gx, gr, gz = (None if d is None else d.numpy() for d in (dx, dr, dz))
    act = (1 << nrhs) - 1 if active is None else active
    for m in range(n):
        what = (g, m, nrhs, zmode, move, first, integer, alphas[m])
        if m >= nrhs or not (act >> m) & 1:
            assert np.array_equal(gr[m], r[m]) and np.array_equal(sc[m], sc0[m]), ("touched", what)
            assert gx is None or np.array_equal(gx[m], x[m], equal_nan=True)
            assert gz is None or np.array_equal(gz[m], z0[m])
            continue
        am = [None if v is None else v[m] for v in a]
        with np.errstate(invalid="ignore"):
            want_x, want_r, want_z = ks.update(zmode, move, am[0], r[m], am[1], am[2], None if z0 is None else z0[m], diag, alphas[m])
        assert np.array_equal(gr[m], want_r), ("r", what)
        assert gx is None or np.array_equal(gx[m], want_x), ("x", what)
        assert gz is None or np.array_equal(gz[m], want_z), ("z", what)
        if integer:
            rr, _ = exact_dot(want_r, want_r, True)
            rz = exact_dot(want_r, want_z, True)[0] if zmode in (1, 2) else 0.0
            assert np.array_equal(sc[m], ks.update_scalars(zmode, rr, rz, first, sc0[m])), (what, sc[m], rr, rz)
        else:
            x1, r1 = (None if am[0] is None else am[0].copy()), r[m].copy()
            z1, sc1 = (None if z0 is None else z0[m].copy()), sc0[m].copy()
            K.pcg_update(zmode, move, x1, r1, am[1], am[2], z1, diag if zmode == 1 else None, first, sc1)
            assert np.array_equal(sc[m], sc1), (what, sc[m], sc1)
            assert np.array_equal(gr[m], r1) and (gx is None or np.array_equal(gx[m], x1)) and (gz is None or np.array_equal(gz[m], z1))
    return gx, gr, gz, sc


@pytest.mark.parametrize("integer", [True, False], ids=["int", "real"])
@pytest.mark.parametrize("shape", UPD, ids=str)
def test_update_many_item_by_item(capi, K, shape, integer):
    """every zmode, move and first on and off; items with different alpha, item 1 the breakdown item"""
    g = shape_of(*shape)
    for nrhs in NRHS:
        data = update_inputs(g, integer, nrhs + 1, 1500 + nrhs)
        for zmode in range(4):
            for move in (0, 1):
                for first in (False, True):
                    check_update_many(capi, K, g, data, zmode, move, first, integer, nrhs)


def test_more_items_than_one_workgroup_holds(capi, K, oracle):
    """20 items: three item chunks of the 7-point direction and the update kernels, and a 27-point batch past 8 items"""
    for shape, nst in (((65, 18, 7), 4), ((129, 6, 5), 14)):
        g = shape_of(*shape)
        so, z, p, pn0, w0, betas = direction_inputs(g, nst, True, 21, 1700)
        check_direction_many(capi, K, oracle, so, so, z, p, pn0, w0, betas, False, True, 20)
        data = update_inputs(g, True, 21, 1710)
        check_update_many(capi, K, g, data, 1, 1, False, True, 20)
        check_update_many(capi, K, g, data, 2, 1, True, True, 20, active=0b10110011100011110101)


# ---------------------------------------------------------------- 3. active mask and isolation
@pytest.mark.parametrize("shape,nst", [((129, 6, 5), 14), ((600, 5, 4), 14), ((65, 18, 7), 4), ((257, 40), 5)], ids=str)
def test_active_mask_skips_items(capi, K, oracle, shape, nst):
    g = shape_of(*shape)
    for active in (0b01101, 0b10000, 0):
        so, z, p, pn0, w0, betas = direction_inputs(g, nst, True, 6, 1800)
        for first in (False, True):
            check_direction_many(capi, K, oracle, so, so, z, p, pn0, w0, betas, first, True, 5, active=active)
        data = update_inputs(g, True, 6, 1810)
        for zmode in range(4):
            check_update_many(capi, K, g, data, zmode, 1, False, True, 5, active=active)
            check_update_many(capi, K, g, data, zmode, 0, True, False, 5, active=active)


@pytest.mark.parametrize("shape,nst", [((258, 5, 6), 14), ((600, 5, 4), 14), ((65, 18, 7), 4), ((600, 9), 3)], ids=str)
def test_items_do_not_see_each_other(capi, K, oracle, shape, nst):
    """item m's bits do not change when the other items are replaced by junk scaled by 1e30 and the order is permuted"""
    g = shape_of(*shape)
    n, perm = 5, [3, 0, 4, 1, 2]  # new position q holds old item perm[q]
    so = direction_data(g, nst, False, 1900)[0]
    fields = [stack(lambda s: pb.uniform(g, s, -1, 1), n, 1901 + 7 * t) for t in range(6)]  # z, p, x, r, w, zin
    betas, alphas = REAL_BETAS[:n], [0.7, -0.4142, 0.0, 1.3, 0.25]
    diag = pb.uniform(g, 1950, 1, 3)

    def run(f, betas, alphas):
        z, p, x, r, w, zin = f
        sc = blocks(n, rho=[3.0] * n, beta=betas, alpha=alphas)
        pn, wn = np.zeros_like(z), np.zeros_like(z)
        K.pcg_direction_many(so, z, p, pn, wn, False, sc)
        out = [pn, wn, sc.copy()]
        for zmode in (1, 2):
            xg, rg, zg, s2 = x.copy(), r.copy(), zin.copy(), sc.copy()
            K.pcg_update_many(zmode, 1, xg, rg, p, w, zg, diag if zmode == 1 else None, False, s2)
            out += [xg, rg, zg, s2]
        return out

    base = run(fields, betas, alphas)
    for m in range(n):
        junk = []
        for t, a in enumerate(fields):
            j = stack(lambda s: pb.uniform(g, s, -1, 1) * 1e30, n, 2000 + 11 * t)
            j[m] = a[m]
            junk.append(np.ascontiguousarray(j[perm]))
        pos = perm.index(m)
        jb, ja = [9.5] * n, [-3.25] * n
        jb[pos], ja[pos] = betas[m], alphas[m]
        with np.errstate(over="ignore", invalid="ignore"):
            got = run(junk, jb, ja)
        for k, (u, v) in enumerate(zip(got, base)):
            assert np.array_equal(u[pos], v[m]), (shape, nst, m, k)


# ---------------------------------------------------------------- 4. the solve against the single-vector solver
def symmetric(st):
    return dict(st, nrelax_post=st["nrelax_pre"])


def check_pcg_many(capi, so, st, b, make_single, x0=None, **kw):
    nrhs = b.shape[0]
    x0 = np.zeros_like(b) if x0 is None else x0
    sm = capi.Solver(so, max_rhs=nrhs, **st)
    x = x0.copy()
    hist, iters = sm.pcg_many(b, x, **kw)
    sm.close()
    s1 = make_single()
    for m in range(nrhs):
        x1 = x0[m].copy()
        h = s1.pcg(b[m], x1, **kw)
        assert iters[m] == len(h) - 1, (m, iters, len(h), kw)
        assert np.array_equal(hist[m], h), (m, hist[m], h, kw)
        assert np.array_equal(x[m], x1), (m, kw, np.max(np.abs(x[m] - x1)))
    s1.close()
    return hist, iters


SOLVE3 = ["fe27_40x33x50_v21", "fe27_65_v21", "poisson7_64_v21", "poisson7_65_v21", "fe27_129_v21"]


@pytest.mark.parametrize("name", SOLVE3, ids=str)
def test_pcg_many_equals_the_single_vector_pcg(capi, name):
    """no level of these problems reaches the 160 rows at which the single-vector cycle switches to partial sums"""
    mk_op, mk_rhs, st = cases.SOLVES[name]
    so, st = mk_op(), symmetric(st)
    _, iters = check_pcg_many(capi, so, st, _rhs_items(mk_rhs), lambda: capi.Solver(so, **st), tol=1e-10)
    assert min(iters) > 1


@pytest.mark.parametrize("precon", ["mg", "diag", "none"])
@pytest.mark.parametrize("stop", ["abs_l2", "rel_l2", "abs_m", "rel_m"])
def test_pcg_many_every_precon_and_stop_test(capi, precon, stop):
    mk_op, mk_rhs, st = cases.SOLVES["fe27_40x33x50_v21"]
    so, st = mk_op(), dict(st, nrelax_pre=1, nrelax_post=1)
    b = _rhs_items(mk_rhs)
    tol = 1e-9 if stop.startswith("rel") else 1e-9 * np.linalg.norm(ps.inner(b[0]))
    x0 = np.stack([pb.uniform(b[0].shape, 77 + m, -1, 1) * pb.interior_mask(b[0].shape) for m in range(3)])
    _, iters = check_pcg_many(capi, so, st, b, lambda: capi.Solver(so, **st), x0=x0, tol=tol, stop=stop, precon=precon,
                              max_iter=40 if precon == "mg" else 25)
    assert min(iters) > 1


def test_pcg_many_two_cycles_per_preconditioner(capi):
    mk_op, mk_rhs, st = cases.SOLVES["fe27_40x33x50_v21"]
    so, st = mk_op(), symmetric(st)
    check_pcg_many(capi, so, st, _rhs_items(mk_rhs), lambda: capi.Solver(so, **st), nmg_cycles=2, tol=1e-10)


def test_pcg_many_on_a_partial_sum_sized_level(capi, monkeypatch):
    """a level with >= 160 rows: the batch runs the reference order there, as a single-vector handle created under
    CEDAR_AMD_PSUM=0 does"""
    so = pb.fe3(24, 176, 12)
    st = dict(relax="point", nrelax_pre=1, nrelax_post=1)
    b = _rhs_items(lambda: pb.rhs3(24, 176, 12))

    def single():
        monkeypatch.setenv("CEDAR_AMD_PSUM", "0")
        return capi.Solver(so, **st)

    check_pcg_many(capi, so, st, b, single, tol=1e-10)


@pytest.mark.parametrize("name", ["varcoef9_200x120_v21", "poisson5_400_v11", "aniso9_512_linexy"], ids=str)
def test_pcg_many_2d_point_and_line_relaxation(capi, name):
    mk_op, mk_rhs, st = cases.SOLVES[name]
    so, st = mk_op(), symmetric(st)
    check_pcg_many(capi, so, st, _rhs_items(mk_rhs), lambda: capi.Solver(so, **st), tol=1e-10)
    check_pcg_many(capi, so, st, _rhs_items(mk_rhs), lambda: capi.Solver(so, **st), precon="diag", max_iter=12)


def test_pcg_many_with_one_item_is_the_single_vector_path(capi):
    """nrhs = 1 on a level of 176 rows: the partial-sum sweeps of the default single-vector path included"""
    so = pb.fe3(24, 176, 12)
    st = dict(relax="point", nrelax_pre=1, nrelax_post=1)
    b = pb.rhs3(24, 176, 12)[None]
    check_pcg_many(capi, so, st, b, lambda: capi.Solver(so, **st), tol=1e-10)
    sm = capi.Solver(so, max_rhs=3, **st)
    x, x1 = np.zeros_like(b), np.zeros_like(b[0])
    hist, iters = sm.pcg_many(b, x, tol=1e-10)
    h = sm.pcg(b[0], x1, tol=1e-10)
    sm.close()
    assert np.array_equal(hist[0], h) and np.array_equal(x[0], x1) and iters == [len(h) - 1]


# ---------------------------------------------------------------- 5. lockstep and freeze
def test_lockstep_and_freeze(capi):
    """an absolute target: the item scaled by 1e-4 needs about half the iterations of the others; plus a zero item"""
    n = (40, 33, 50)
    so, st = pb.fe3(*n), dict(relax="point", nrelax_pre=1, nrelax_post=1)
    b = _rhs_items(lambda: pb.rhs3(*n), 4)
    b[1] *= 1e-4
    b[3] = 0.0
    kw = dict(stop="abs_l2", tol=1e-9 * np.linalg.norm(ps.inner(b[0])), max_iter=30)
    s1 = capi.Solver(so, **st)
    single, xs = [], []
    for m in range(4):
        x1 = np.zeros_like(b[m])
        single.append(s1.pcg(b[m], x1, **kw))
        xs.append(x1)
    s1.close()
    n1 = [len(h) - 1 for h in single]
    assert n1[1] < n1[0] and n1[1] < n1[2] and n1[3] == 0, n1  # the single-vector counts differ
    sentinel = -7.25
    buf = np.full((4, kw["max_iter"] + 1), sentinel)
    x = np.zeros_like(b)
    s = capi.Solver(so, max_rhs=4, **st)
    ps_ = capi.PcgSettings(kw["max_iter"], kw["tol"], capi.PCG_STOP["abs_l2"], capi.PCG_PRECON["mg"], 1)
    it = np.full(4, 77, dtype=np.int32)
    rc = capi.lib.cedar_amd_solver_pcg_many(s.h, 4, b.ctypes.data, x.ctypes.data, C.byref(ps_), buf.ctypes.data,
                                            it.ctypes.data_as(C.POINTER(C.c_int)))
    assert it.tolist() == n1 and rc == max(n1) and 0 < rc < kw["max_iter"]
    for m in range(4):
        assert np.array_equal(buf[m, : n1[m] + 1], single[m]), m
        assert np.all(buf[m, n1[m] + 1:] == sentinel), m  # a frozen item's row is not written any further
        assert np.array_equal(x[m], xs[m]), m  # the early item was left alone: the difference from solve_many
    assert buf[3, 0] == 0.0 and np.all(x[3] == 0.0)
    # through the front end, with hist handed in
    buf2, x2 = np.full_like(buf, sentinel), np.zeros_like(b)
    hist, iters = s.pcg_many(b, x2, hist=buf2, **kw)
    s.close()
    assert iters == n1 and np.array_equal(buf2, buf) and np.array_equal(x2, x)
    assert [len(h) for h in hist] == [k + 1 for k in n1]


def test_one_item_breaks_down_while_the_others_go_on(capi):
    """a 2D 5-point operator of two uncoupled regions, the centre plane sign-flipped in the right one: -(4 I + N) there is
    negative definite, so a right-hand side supported there has p.Ap < 0 in its first iteration.  Uploaded after a
    healthy set-up; precon = none reads the level-0 operator only."""
    nx = ny = 31
    good = pb.poisson2(nx, ny)
    bad = good.copy()
    h = 16  # columns 1 .. h healthy, h+1 .. nx flipped
    bad[pb.KW, :, h + 1] = 0.0  # the couplings between columns h and h+1
    bad[pb.KO, :, h + 1:] *= -1.0
    g = good.shape[1:]
    left, right = np.zeros(g, dtype=bool), np.zeros(g, dtype=bool)
    left[1:-1, 1: h + 1], right[1:-1, h + 1: nx + 1] = True, True
    b = np.stack([pb.uniform(g, 31, -1, 1) * left, pb.uniform(g, 32, -1, 1) * right, pb.uniform(g, 33, -1, 1) * left])
    x0 = np.stack([pb.uniform(g, 41 + m, -1, 1) * msk for m, msk in enumerate((left, right, left))])
    st = dict(relax="point", nrelax_pre=1, nrelax_post=1)
    kw = dict(precon="none", tol=1e-8, max_iter=200)
    s1 = capi.Solver(good, **st)
    s1.set_array(0, "A", bad)
    single, xs = [], []
    for m in range(3):
        x1 = x0[m].copy()
        single.append(s1.pcg(b[m], x1, **kw))
        xs.append(x1)
    s1.close()
    # the single-vector call itself: the breakdown item returns at once with x as given, the healthy ones converge
    assert len(single[1]) == 1 and single[1][0] > 0 and np.array_equal(xs[1], x0[1]) and np.all(np.isfinite(xs[1]))
    assert all(2 < len(single[m]) - 1 < 200 and single[m][-1] < 1e-8 for m in (0, 2))
    s = capi.Solver(good, max_rhs=3, **st)
    s.set_array(0, "A", bad)
    x = x0.copy()
    hist, iters = s.pcg_many(b, x, **kw)
    s.close()
    assert iters == [len(hh) - 1 for hh in single] and iters[1] == 0
    for m in range(3):
        assert np.array_equal(hist[m], single[m]) and np.array_equal(x[m], xs[m]), m


# ---------------------------------------------------------------- 6. against the statement
@pytest.mark.parametrize("name,mk,st", PARITY, ids=[c[0] for c in PARITY])
def test_pcg_many_parity_with_statement(capi, oracle, name, mk, st):
    """item 0 of a batch of three, compared as tests/test_gpu_pcg.py compares the single-vector solve"""
    so = mk()
    g = so.shape[1:]
    b = np.stack([ps.random_field(g, 17), ps.random_field(g, 18), ps.random_field(g, 19)])
    x0 = np.stack([ps.random_field(g, 23), ps.random_field(g, 24), ps.random_field(g, 25)])
    s = capi.Solver(so, max_rhs=3, **st)
    ml = oracle.ml_create(so, **st)
    try:
        x = x0.copy()
        hist, iters = s.pcg_many(b, x, tol=1e-10, max_iter=40)
        xs = x0[0].copy()
        ns, hs = ps.pcg(oracle, so, b[0], xs, ml=ml, tol=1e-10, max_iter=40)
        h = hist[0]
        compare_hist(h, hs, iters[0], ns)
        if name in SLOW:
            assert ns == 40 and len(h) == 41 and hs[-1] >= 1e-10 and h[-1] >= 1e-10
        else:
            assert h[-1] < 1e-10
    finally:
        s.close()
        ml.close()


# ---------------------------------------------------------------- 7. determinism, capacity and reuse
def test_pcg_many_is_deterministic(capi):
    so = pb.fe3(24, 164, 12)
    g = so.shape[1:]
    b = np.stack([ps.random_field(g, 5 + m) for m in range(3)])
    s = capi.Solver(so, nrelax_pre=1, nrelax_post=1, max_rhs=3)
    out = []
    for _ in range(2):
        x = np.zeros_like(b)
        hist, iters = s.pcg_many(b, x, tol=1e-12, max_iter=30)
        out.append((x, np.concatenate(hist), np.array(iters)))
    s.close()
    assert all(np.array_equal(u, v) for u, v in zip(*out))


def test_capacity_and_reuse(capi):
    """one max_rhs = 4 handle: pcg_many with 4, then 2, then pcg, then solve_many, then pcg_many again, on device arrays,
    twice (the captured cycles are keyed on the batch count, the Krylov storage is shared by all of them)"""
    mk_op, mk_rhs, st = cases.SOLVES["fe27_65_v21"]
    so, st = mk_op(), symmetric(st)
    b = _rhs_items(mk_rhs, 4)
    kw = dict(tol=1e-10, max_iter=30)
    s1 = capi.Solver(so, **st)
    want_h, want_x = [], []
    for m in range(4):
        x1 = np.zeros_like(b[m])
        want_h.append(s1.pcg(b[m], x1, **kw))
        want_x.append(x1)
    x1 = np.zeros_like(b[0])
    want_solve = s1.solve(b[0], x1)
    s1.close()
    s = capi.Solver(so, max_rhs=4, **st)
    db4, dx4 = capi.DeviceArray.from_numpy(b), capi.DeviceArray(b.shape)
    db2, dx2 = capi.DeviceArray.from_numpy(b[:2]), capi.DeviceArray(b[:2].shape)
    db1, dx1 = capi.DeviceArray.from_numpy(b[0]), capi.DeviceArray(b[0].shape)

    def many(nrhs, db, dx, rep):
        dx.zero()
        hist, iters = s.pcg_many(db, dx, **kw)
        got = dx.numpy()
        for m in range(nrhs):
            assert np.array_equal(hist[m], want_h[m]) and np.array_equal(got[m], want_x[m]), (rep, nrhs, m)

    for rep in range(2):
        many(4, db4, dx4, rep)
        many(2, db2, dx2, rep)
        dx1.zero()
        h = s.pcg(db1, dx1, **kw)
        assert np.array_equal(h, want_h[0]) and np.array_equal(dx1.numpy(), want_x[0]), rep
        dx2.zero()
        rel, its = s.solve_many(db2, dx2)
        assert np.array_equal(rel[0][: its[0] + 1], want_solve), rep
        many(4, db4, dx4, rep)
    s.close()


# ---------------------------------------------------------------- 8. refusals
def test_refusals(capi, capfd):
    so3, b3 = pb.fe3(17, 17, 17), pb.rhs3(17, 17, 17)
    so2p, b2p = pb.periodic_poisson2(32, 32, (True, False)), pb.periodic_rhs2(32, 32, (True, False))
    sentinel = -3.5
    v11 = dict(nrelax_pre=1, nrelax_post=1)

    def refused(s, b, nrhs, text, **kw):
        bb = np.stack([b] * max(nrhs, 1))
        x = np.full_like(bb, sentinel)
        p = capi.PcgSettings(kw.get("max_iter", 20), 1e-8, kw.get("stop_test", 1), kw.get("precon", 3), 1)
        hist = np.full((bb.shape[0], max(p.max_iter, 0) + 1), sentinel)
        it = np.full(bb.shape[0], 77, dtype=np.int32)
        capfd.readouterr()
        rc = capi.lib.cedar_amd_solver_pcg_many(s.h, nrhs, bb.ctypes.data, x.ctypes.data, C.byref(p), hist.ctypes.data,
                                                it.ctypes.data_as(C.POINTER(C.c_int)))
        err = capfd.readouterr().err
        assert rc == -1 and text in err and "cedar_amd_solver_pcg_many" in err, (text, err)
        assert np.all(x == sentinel) and np.all(hist == sentinel) and np.all(it == 77)
        if nrhs >= 1 and not kw:
            with pytest.raises(RuntimeError):
                s.pcg_many(bb, x)
            assert np.all(x == sentinel)

    def still_solves(s, b, nrhs):
        bb = np.stack([b] * nrhs)
        x = np.zeros_like(bb)
        hist, iters = s.pcg_many(bb, x)
        assert all(0 < k < 50 and hh[-1] < 1e-8 for k, hh in zip(iters, hist)) and np.all(np.isfinite(x))

    s = capi.Solver(so3, max_rhs=2, **v11)
    refused(s, b3, 0, "nrhs must be at least 1")
    refused(s, b3, 3, "exceeds the handle's max_rhs")
    refused(s, b3, 2, "stop_test must be 0..3", stop_test=7)
    refused(s, b3, 2, "precon must be 1..3", precon=0)
    refused(s, b3, 2, "max_iter must not be negative", max_iter=-1)
    still_solves(s, b3, 2)
    s.close()

    s = capi.Solver(so3, max_rhs=2, nrelax_pre=2, nrelax_post=1)
    refused(s, b3, 2, "nrelax_pre == nrelax_post")
    x = np.zeros((2,) + b3.shape)
    bb = np.stack([b3, pb.uniform(b3.shape, 91, -1, 1) * pb.interior_mask(b3.shape)])
    hist, iters = s.pcg_many(bb, x, precon="diag", max_iter=5)  # V(2,1) is no obstacle without the cycle
    for m in range(2):  # (b3 is an eigenvector of this operator: one iteration; the random item uses all five)
        x1 = np.zeros_like(b3)
        h = s.pcg(bb[m], x1, precon="diag", max_iter=5)
        assert iters[m] == len(h) - 1 >= 1 and np.array_equal(hist[m], h) and np.array_equal(x[m], x1), (m, iters, h)
    assert iters[1] == 5, iters
    s.close()

    for kw, so, b, text in ((dict(ibc=2, **v11), so2p, b2p, "periodic"), (dict(cycle="f", **v11), so3, b3, "V-cycle"),
                            (dict(relax="plane-xy", **v11), so3, b3, "plane relaxation")):
        s = capi.Solver(so, max_rhs=2, **kw)
        refused(s, b, 1, text)
        refused(s, b, 2, text)
        x = np.zeros_like(b)
        h = s.solve(b, x)  # the single-vector entry points serve such a handle as before
        assert len(h) >= 2 and np.all(np.isfinite(h)) and h[-1] < 1.0
        s.close()

    assert capi.lib.cedar_amd_solver_pcg_many(None, 1, b3.ctypes.data, b3.ctypes.data, None, None, None) == -1


def test_pass_entry_points_refuse_what_they_do_not_serve(capi, K):
    g = (5, 6, 7)
    f = np.stack([pb.uniform(g, 1, -1, 1)] * 2)
    so = pb.random_op(g, 14, 2)
    sc = blocks(2)
    ptr, u = (lambda a: a.ctypes.data_as(capi.P)), capi.u
    for nrhs in (0, 33):  # refused before anything is read
        assert capi.lib.cedar_amd_pcg_direction_many(nrhs, u(1), ptr(so), ptr(f), ptr(f), ptr(f), ptr(f), u(7), u(6), u(5), 14, 0,
                                                     ptr(sc)) == -1
        assert capi.lib.cedar_amd_pcg_update_many(nrhs, u(1), 0, 0, None, ptr(f), None, None, None, None, u(7), u(6), u(5), 0,
                                                  ptr(sc)) == -1
    with pytest.raises(RuntimeError):
        K.pcg_direction_many(so[:7].copy(), f, f, f.copy(), f.copy(), False, sc)
    with pytest.raises(RuntimeError):
        K.pcg_direction_many(so, f, None, f.copy(), f.copy(), False, sc)  # p is needed unless first
    with pytest.raises(RuntimeError):
        K.pcg_update_many(4, 0, None, f.copy(), None, None, None, None, False, sc)
    with pytest.raises(RuntimeError):
        K.pcg_update_many(1, 0, None, f.copy(), None, None, f.copy(), None, False, sc)  # zmode 1 needs the diagonal
    with pytest.raises(RuntimeError):
        K.pcg_update_many(0, 1, None, f.copy(), f, f, None, None, False, sc)  # move needs x
    assert np.array_equal(sc, blocks(2))
