"""Flexible CG on periodic handles (cedar_amd_solver_fcg_periodic, Solver.fcg_periodic) and its wrap-around operator pass
(krylov.hip pcg_dir2_per / pcg_dir7_per / pcg_dir27_per through cedar_amd_pcg_direction_periodic).

1. The kernel, bit for bit: against krylov_statement.direction applied to WRAPPED COPIES of z and p (problems.wrap3), the
   arrays handed to the kernel carrying NaN in every ghost cell whose index lies on the ghost layer of a periodic
   direction and zero in the other ghost cells.  A NaN that reached any arithmetic would show in pn, w or sigma.  Data
   as in tests/test_gpu_krylov.py: small integers (sigma and alpha have one correct bit pattern) and random reals
   (sigma inside the any-order bound).  Row lengths from the launcher (krylov.hip pcg_direction_periodic): the 27-point
   kernel runs 64 lanes up to 64 pairs (nx <= 128), 128 up to 128 pairs (nx <= 256), else 256 with a second trip of the
   pair loop past 512 points; the 7-point kernel 64 lanes up to nx = 64, 128 up to 255 (second trip past 128), else 256
   (second trip past 256); the 2D kernel one workgroup per 256 points of a row.  One length on either side of each, nx = 2
   and odd nx (a half pair at the row end, whose right neighbour is the wrap); ny, nz in {2, 3, 5}.
2. The solver against tests/fcg_periodic_statement.py on the 22 periodic solve cases, by compare_hist's rule.
3. Ghost independence, 4. reproducibility, 5. forwarding on a Dirichlet handle, 6. refusals.
"""
import ctypes as C

import numpy as np
import pytest

import cases
import fcg_periodic_statement as fps
import krylov_statement as ks
import pcg_statement as ps
import problems as pb
from test_gpu_krylov import BETAS, direction_data, exact_dot, scalars, shape_of
from test_gpu_pcg import compare_hist

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from cedar_amd import capi
    assert capi.device_count() >= 1, "no GPU visible"
    return capi


@pytest.fixture(scope="module")
def K(capi):
    return capi.Kernels()


# ---------------------------------------------------------------- 1. the kernel
def periodic_ghosts(g, per):
    """mask of the cells whose index lies on the ghost layer of a periodic direction; per = (x, y, z)"""
    m = np.zeros(g, dtype=bool)
    for axis, on in zip((-1, -2, -3), per):
        if on and len(g) >= -axis:
            sl = [slice(None)] * len(g)
            for end in (0, -1):
                sl[axis] = end
                m[tuple(sl)] = True
    return m


def poisoned(a, per):
    """ghost cells of a periodic direction NaN, every other ghost cell zero"""
    out = np.where(pb.interior_mask(a.shape), a, 0.0)
    out[periodic_ghosts(a.shape, per)] = np.nan
    return out


def check_direction_periodic(K, oracle, so, z, p, ibc, beta, first, integer, rho=3.0):
    g = z.shape
    per = fps.per_of(len(g), ibc)
    zk, pk = poisoned(z, per), poisoned(p, per)
    zw, pw = fps.wrap(zk.copy(), per), fps.wrap(pk.copy(), per)
    assert not np.isnan(zw).any() and not np.isnan(pw).any()  # the wrap overwrote every poisoned cell
    pn0, w0 = pb.uniform(g, 77, 1, 2), pb.uniform(g, 78, 1, 2)  # sentinels: untouched outside the interior
    sc0 = scalars(rho=rho, beta=beta)
    want_pn, want_w = ks.direction(oracle, so, zw, pw, pn0, w0, beta, first)
    sigma, bound = exact_dot(want_pn, want_w, integer)
    p_arg = np.full(g, np.nan) if first else pk  # first: p is not read
    pn, w, sc = pn0.copy(), w0.copy(), sc0.copy()
    K.pcg_direction_periodic(so, zk, p_arg, pn, w, ibc, first, sc)
    what = (g, ibc, beta, first, integer)
    assert np.array_equal(pn, want_pn), ("pn", what)
    assert np.array_equal(w, want_w), ("w", what, np.nanmax(np.abs(w - want_w)))
    if integer:
        assert np.array_equal(sc, ks.set_alpha(sigma, sc0)), (what, sc, sigma)
    else:
        assert abs(sc[ks.SIGMA] - sigma) <= bound, (what, sc[ks.SIGMA], sigma, bound)
        assert np.array_equal(sc, ks.set_alpha(float(sc[ks.SIGMA]), sc0)) and sc[ks.FLAG] == 0.0, (what, sc)
    # rank-grid variant: the same sum into partial[0], sc only read
    pn2, w2, sc2, part = pn0.copy(), w0.copy(), sc0.copy(), np.array([55.0])
    K.pcg_direction_periodic(so, zk, p_arg, pn2, w2, ibc, first, sc2, part)
    assert np.array_equal(pn2, want_pn) and np.array_equal(w2, want_w), what
    assert np.array_equal(sc2, sc0) and part[0] == sc[ks.SIGMA], (what, sc2, part, sc[ks.SIGMA])


def sweep(K, oracle, g, nst, ibc):
    for integer in (True, False):
        so, z, p = direction_data(g, nst, integer, 300 + nst)
        for beta in (BETAS if integer else [0.3717]):
            check_direction_periodic(K, oracle, so, z, p, ibc, beta, False, integer)
        check_direction_periodic(K, oracle, so, z, p, ibc, 0.625, True, integer)  # first: beta forced to 0


def with_rows(nxs, rows):
    return [(nx,) + rows[t % len(rows)] for t, nx in enumerate(nxs)]


# (nx, ny, nz): both sides of the 64 | 128 | 256 lane switches and of the second trip; 2 and odd
DIR27 = with_rows([2, 3, 128, 129, 256, 257, 512, 513], [(2, 3), (3, 5), (5, 2), (3, 3)])
DIR7 = with_rows([2, 3, 64, 65, 128, 129, 255, 256, 257], [(2, 3), (3, 5), (5, 2), (3, 3)])
DIR2 = with_rows([2, 3, 255, 256, 257, 512, 513], [(2,), (3,), (5,)])
ONE27, ONE7, ONE2 = (129, 3, 5), (65, 5, 3), (257, 3)  # the one shape of the codes that do not get the whole list


def cases_of(shapes, one, full_codes, codes):
    return [(ibc, s) for ibc in codes for s in (shapes if ibc in full_codes else [one])]


@pytest.mark.parametrize("ibc,shape", cases_of(DIR27, ONE27, (2, 8), (1, 2, 3, 5, 6, 7, 8)), ids=str)
def test_direction_periodic_27pt(K, oracle, ibc, shape):
    sweep(K, oracle, shape_of(*shape), 14, ibc)


@pytest.mark.parametrize("ibc,shape", cases_of(DIR7, ONE7, (2, 8), (1, 2, 3, 5, 6, 7, 8)), ids=str)
def test_direction_periodic_7pt(K, oracle, ibc, shape):
    sweep(K, oracle, shape_of(*shape), 4, ibc)


@pytest.mark.parametrize("nst", [3, 5])
@pytest.mark.parametrize("ibc,shape", cases_of(DIR2, ONE2, (2, 3), (1, 2, 3)), ids=str)
def test_direction_periodic_2d(K, oracle, ibc, shape, nst):
    sweep(K, oracle, shape_of(*shape), nst, ibc)


@pytest.mark.parametrize("shape,nst", [((129, 3, 5), 14), ((3, 2, 2), 14), ((65, 5, 3), 4), ((257, 3), 5), ((3, 2), 3)], ids=str)
def test_direction_periodic_with_ibc_0_is_the_dirichlet_pass(K, shape, nst):
    """ghosts non-zero everywhere: the forwarded call reads them as cedar_amd_pcg_direction does"""
    g = shape_of(*shape)
    so, z, p = direction_data(g, nst, False, 950)
    for first in (False, True):
        outs = []
        for call in (lambda *a: K.pcg_direction(*a), lambda so_, z_, p_, pn_, w_, f_, sc_: K.pcg_direction_periodic(so_, z_, p_, pn_, w_, 0, f_, sc_)):
            pn, w, sc = pb.uniform(g, 77, 1, 2), pb.uniform(g, 78, 1, 2), scalars(rho=3.0, beta=0.3717)
            call(so, z, p, pn, w, first, sc)
            outs.append((pn, w, sc))
        for a, b in zip(*outs):
            assert np.array_equal(a, b), (shape, nst, first)
        assert outs[0][2][ks.FLAG] == 0.0 and np.isfinite(outs[0][2][ks.SIGMA])


def test_direction_periodic_refuses_codes_the_dimension_does_not_define(K):
    for g, nst, bad in (((5, 6), 3, (4, 5, 8, -1)), ((5, 6, 7), 4, (4, 9, -1))):
        f = pb.uniform(g, 1, -1, 1)
        so = pb.random_op(g, nst, 2)
        for ibc in bad:
            pn, w, sc = f.copy(), f.copy(), scalars()
            with pytest.raises(RuntimeError):
                K.pcg_direction_periodic(so, f, f, pn, w, ibc, False, sc)
            assert np.array_equal(pn, f) and np.array_equal(w, f) and np.array_equal(sc, scalars())


# ---------------------------------------------------------------- 2. the solver against the statement
ALL = [("2d", k) for k in cases.SOLVES_PER] + [("3d", k) for k in cases.SOLVES_PER3]


def problem(dim, name):
    mk_op, _, st = (cases.SOLVES_PER if dim == "2d" else cases.SOLVES_PER3)[name]
    so = mk_op()
    g = so.shape[1:]
    return so, st, ps.random_field(g, 17), ps.random_field(g, 23)


@pytest.mark.parametrize("dim,name", ALL, ids=[n for _, n in ALL])
def test_fcg_periodic_parity_with_statement(capi, oracle, dim, name):
    so, st, b, x0 = problem(dim, name)
    s = capi.Solver(so, **st)
    ml = oracle.ml_create(so, **st)
    try:
        x = x0.copy()
        h = s.fcg_periodic(b, x, tol=1e-10, max_iter=40)
        xs = x0.copy()
        ns, hs = fps.fcg_periodic(oracle, so, b, xs, ml, st["ibc"], tol=1e-10, max_iter=40)
        m = min(len(h), len(hs))
        true = fps.true_residual(oracle, so, b, x, st["ibc"]) / h[0]
        print(name, "device", len(h) - 1, "statement", ns, "max rel diff", np.max(np.abs(h[1:m] / hs[1:m] - 1)), "true", true)
        compare_hist(h, hs, len(h) - 1, ns)
        assert h[-1] < 1e-10
        assert true < 1e-10, true
    finally:
        s.close()
        ml.close()


SETTINGS_CASES = [("2d", "perrand9_xy_96x80_v21"), ("3d", "perrand27_xyz_32_v21")]  # diagonally dominant: CG alone converges


@pytest.mark.parametrize("precon", ["none", "diag"])
@pytest.mark.parametrize("dim,name", SETTINGS_CASES, ids=[n for _, n in SETTINGS_CASES])
def test_fcg_periodic_without_the_cycle(capi, oracle, dim, name, precon):
    """precon 1 | 2: M is exactly symmetric and the library runs the standard beta, as fcg does on Dirichlet handles"""
    so, st, b, x0 = problem(dim, name)
    s = capi.Solver(so, **st)
    try:
        x = x0.copy()
        h = s.fcg_periodic(b, x, tol=1e-10, max_iter=40, precon=precon)
        xs = x0.copy()
        ns, hs = fps.fcg_periodic(oracle, so, b, xs, None, st["ibc"], standard=True, tol=1e-10, max_iter=40, precon=precon)
        print(name, precon, "device", len(h) - 1, "statement", ns)
        compare_hist(h, hs, len(h) - 1, ns)
        assert h[-1] < 1e-10 and fps.true_residual(oracle, so, b, x, st["ibc"]) / h[0] < 1e-10
    finally:
        s.close()


STOP_CASES = [("2d", "perpoisson5_y_128x96_v21"), ("3d", "perpoisson7_z_24x20x32_v11")]


@pytest.mark.parametrize("stop", ["abs_l2", "rel_l2", "abs_m", "rel_m"])
@pytest.mark.parametrize("dim,name", STOP_CASES, ids=[n for _, n in STOP_CASES])
def test_fcg_periodic_stop_tests(capi, oracle, dim, name, stop):
    so, st, b, _ = problem(dim, name)
    g = so.shape[1:]
    tol = 1e-9 if stop.startswith("rel") else 1e-9 * np.linalg.norm(ps.inner(b))
    s = capi.Solver(so, **st)
    ml = oracle.ml_create(so, **st)
    try:
        x = np.zeros(g)
        h = s.fcg_periodic(b, x, tol=tol, stop=stop)
        xs = np.zeros(g)
        ns, hs = fps.fcg_periodic(oracle, so, b, xs, ml, st["ibc"], tol=tol, stop=stop)
        compare_hist(h, hs, len(h) - 1, ns)
        assert 2 < ns < 50
    finally:
        s.close()
        ml.close()


# ---------------------------------------------------------------- 3. ghost independence, 4. reproducibility
GHOST_CASES = [("2d", "perpoisson5_x_200x60_linex"), ("2d", "perrand9_xy_96x80_f21"), ("3d", "perpoisson7_xy_32x32x24_v21"),
               ("3d", "perrand27_xyz_32_v21")]


@pytest.mark.parametrize("dim,name", GHOST_CASES, ids=[n for _, n in GHOST_CASES])
def test_ghost_layers_of_x_and_b_do_not_matter(capi, dim, name):
    """b: every ghost cell garbage (none is read).  x: garbage in the ghost cells of the periodic directions -- they are
    wrapped before the first residual; the ghost layer of a Dirichlet side is the boundary value of the problem (zero),
    as for every solve of the library.  On return the ghosts of x hold the periodic image."""
    so, st, b, x0 = problem(dim, name)
    per = fps.per_of(so.ndim - 1, st["ibc"])
    ghost = ~pb.interior_mask(b.shape)
    bg, xg = b.copy(), x0.copy()
    bg[ghost] = 1e30 * pb.uniform(b.shape, 5, -1, 1)[ghost]
    pg = periodic_ghosts(b.shape, per)
    xg[pg] = 1e30 * pb.uniform(b.shape, 6, -1, 1)[pg]
    s = capi.Solver(so, **st)
    try:
        x = x0.copy()
        h = s.fcg_periodic(b, x, tol=1e-10, max_iter=40)
        hg = s.fcg_periodic(bg, xg, tol=1e-10, max_iter=40)
        x2 = x0.copy()
        h2 = s.fcg_periodic(b, x2, tol=1e-10, max_iter=40)  # 4. the first run again
    finally:
        s.close()
    assert len(h) > 3 and h[-1] < 1e-10
    assert np.array_equal(h, hg) and np.array_equal(ps.inner(x), ps.inner(xg))
    for a in (x, xg):
        assert np.array_equal(a, fps.wrap(a.copy(), per))  # the periodic image, bit for bit
        assert not np.any(a[ghost & ~pg])  # Dirichlet ghosts as given: zero
    assert np.array_equal(h, h2) and np.array_equal(x, x2)


# ---------------------------------------------------------------- 5. forwarding
@pytest.mark.parametrize("mk,st", [(lambda: pb.fe3(25, 22, 19), dict(nrelax_pre=2, nrelax_post=1)),
                                   (lambda: pb.varcoef9(65, 60, sigma=8.0), dict(nrelax_pre=2, nrelax_post=1, cycle="f"))],
                         ids=["fe3-v21", "varcoef9-f21"])
def test_a_dirichlet_handle_is_served_by_fcg(capi, mk, st):
    so = mk()
    g = so.shape[1:]
    b, x0 = ps.random_field(g, 17), ps.random_field(g, 23)
    s = capi.Solver(so, **st)
    try:
        x, xf = x0.copy(), x0.copy()
        h = s.fcg_periodic(b, x, tol=1e-10, max_iter=40)
        hf = s.fcg(b, xf, tol=1e-10, max_iter=40)
        assert len(h) > 3 and np.array_equal(h, hf) and np.array_equal(x, xf)
    finally:
        s.close()


# ---------------------------------------------------------------- 6. refusals
def raw(capi, h, b, x, hist, **kw):
    p = capi.PcgSettings(kw.get("max_iter", 20), 1e-8, kw.get("stop_test", 1), kw.get("precon", 3), kw.get("nmg_cycles", 1))
    return capi.lib.cedar_amd_solver_fcg_periodic(h, b.ctypes.data, x.ctypes.data, C.byref(p), hist.ctypes.data)


def test_fcg_periodic_refusals(capi, capfd):
    sentinel = -3.5
    per = (True, False)
    so = pb.periodic_poisson2(32, 32, per)
    g = so.shape[1:]
    b = ps.random_field(g, 1)

    def refused(h, text, who="cedar_amd_solver_fcg_periodic", **kw):
        x, hist = np.full(g, sentinel), np.full(21, sentinel)
        capfd.readouterr()
        assert raw(capi, h, b, x, hist, **kw) == -1
        err = capfd.readouterr().err
        assert text in err and who in err, (text, err)
        assert np.all(x == sentinel) and np.all(hist == sentinel)

    refused(None, "")
    s = capi.Solver(so, nrelax_pre=1, nrelax_post=1, ibc=pb.ibc_of(per))
    try:
        refused(s.h, "stop_test must be 0..3", stop_test=7)
        refused(s.h, "precon must be 1..3", precon=0)
        refused(s.h, "nmg_cycles must be at least 1", nmg_cycles=0)
        refused(s.h, "max_iter must not be negative", max_iter=-1)
        x = np.full(g, sentinel)
        with pytest.raises(RuntimeError):
            s.fcg_periodic(b, x, nmg_cycles=0)
        assert np.all(x == sentinel)
        x = np.zeros(g)
        h = s.fcg_periodic(b, x)  # the handle stays usable
        assert 1 < len(h) - 1 < 50 and h[-1] < 1e-8
        # the calls that refuse periodic handles still do
        for call in (s.pcg, s.fcg):
            x = np.full(g, sentinel)
            with pytest.raises(RuntimeError):
                call(b, x)
            assert np.all(x == sentinel)
    finally:
        s.close()
    # a handle that holds more than one right-hand side (Dirichlet: a periodic handle never does)
    sd = pb.poisson2(31, 29)
    gd = sd.shape[1:]
    sm = capi.Solver(sd, max_rhs=2)
    try:
        assert sm.max_rhs() == 2
        bd = ps.random_field(gd, 1)
        x, hist = np.full(gd, sentinel), np.full(21, sentinel)
        capfd.readouterr()
        assert raw(capi, sm.h, bd, x, hist) == -1
        err = capfd.readouterr().err
        assert "max_rhs > 1" in err and "cedar_amd_solver_fcg_periodic" in err, err
        assert np.all(x == sentinel) and np.all(hist == sentinel)
        x = np.zeros(gd)
        h = sm.fcg(bd, x)  # the handle stays usable
        assert 1 < len(h) - 1 < 50 and h[-1] < 1e-8
    finally:
        sm.close()
    # a periodic handle asked for with max_rhs = 2 holds one right-hand side and is served
    sp = capi.Solver(so, nrelax_pre=1, nrelax_post=1, ibc=pb.ibc_of(per), max_rhs=2)
    try:
        assert sp.max_rhs() == 1
        x = np.zeros(g)
        h = sp.fcg_periodic(b, x)
        assert h[-1] < 1e-8
    finally:
        sp.close()
