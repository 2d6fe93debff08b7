"""Flexible conjugate gradients on the device (cedar_amd_solver_fcg / _fcg_many, Solver.fcg / fcg_many) and its one new
pass (krylov.hip pcg_dwz / pcg_dwz_many through cedar_amd_pcg_dots_wz[_many]).

The pass is held to the exact dot as tests/test_gpu_krylov.py holds pcg_update: on small-integer data every partial sum
is an exact double, so r.r, r.z, w.z have one correct bit pattern and beta = -((alpha * w.z) / rho) follows; on real data
the dots are inside the any-order bound and beta is recomputed from the device's own alpha, w.z, rho bit for bit.  The
solver is compared with the numpy statement of tests/fcg_statement.py on the oracle by compare_hist's rule.
"""
import ctypes as C

import numpy as np
import pytest

import fcg_statement as fs
import krylov_statement as ks
import pcg_statement as ps
import problems as pb
from test_gpu_krylov import ALPHAS, UPD, exact_dot, ints, shape_of
from test_gpu_pcg import compare_hist

pytestmark = pytest.mark.gpu

WZ = 7  # the slot of w.z in the scalar block (common.h PCG_WZ)
# what the pass must leave alone (sigma, alpha, flag) or overwrite (the rest)
MARKS = {ks.SIGMA: 101.0, ks.ALPHA: 102.0, ks.BETA: 103.0, ks.RR: 104.0, ks.RZ: 105.0, ks.FLAG: 106.0, WZ: 107.0}


@pytest.fixture(scope="module")
def capi():
    from cedar_amd import capi
    assert capi.device_count() >= 1, "no GPU visible"
    return capi


@pytest.fixture(scope="module")
def K(capi):
    return capi.Kernels()


def block(rho, alpha):
    sc = np.zeros(ks.NSC)
    for k, v in MARKS.items():
        sc[k] = v
    sc[ks.RHO], sc[ks.ALPHA] = rho, alpha
    return sc


def flex_scalars(rr, rz, wz, first, sc0):
    """krylov.hip set_rho_flex"""
    sc = np.array(sc0, dtype=np.float64)
    rho, alpha = float(sc[ks.RHO]), float(sc[ks.ALPHA])
    sc[ks.RR], sc[ks.RZ], sc[WZ] = rr, rz, wz
    sc[ks.BETA] = 0.0 if first or rho == 0.0 else -((alpha * wz) / rho)
    sc[ks.RHO] = rz
    return sc


def wz_data(g, integer, seed):
    """r, z, w with non-zero ghosts; integer: |r|, |z| <= 8 and |w| < 2^12, so |w z| < 2^15 per point"""
    if integer:
        return ints(g, seed, -8, 8), ints(g, seed + 1, -8, 8), ints(g, seed + 2, -4095, 4095)
    return pb.uniform(g, seed, -1, 1), pb.uniform(g, seed + 1, -1, 1), pb.uniform(g, seed + 2, -1, 1)


# ---------------------------------------------------------------- 1. the new pass alone
# test_gpu_krylov's shapes for pcg_upd (more rows than workgroups, odd nx = a half pair, nx > 512 = a second trip of the
# pair loop, 2D and 3D) and the smallest grids
SHAPES = UPD + [(3, 3), (3, 3, 3)]


def check_dots_wz(capi, K, g, r, z, w, rho, alpha, first, integer):
    sc0 = block(rho, alpha)
    dr, dz, dw = (capi.DeviceArray.from_numpy(a) for a in (r, z, w))
    sc = sc0.copy()
    K.pcg_dots_wz(dr, dz, dw, first, sc)
    what = (g, rho, alpha, first, integer)
    for d, a in ((dr, r), (dz, z), (dw, w)):  # the pass writes no vector
        assert np.array_equal(d.numpy(), a), what
        d.free()
    assert sc[ks.ALPHA] == sc0[ks.ALPHA] and sc[ks.SIGMA] == sc0[ks.SIGMA] and sc[ks.FLAG] == sc0[ks.FLAG], (what, sc)
    (rr, brr), (rz, brz), (wz, bwz) = exact_dot(r, r, integer), exact_dot(r, z, integer), exact_dot(w, z, integer)
    if integer:
        assert np.array_equal(sc, flex_scalars(rr, rz, wz, first, sc0)), (what, sc, rr, rz, wz)
    else:
        assert abs(sc[ks.RR] - rr) <= brr, (what, sc[ks.RR], rr, brr)
        assert abs(sc[ks.RZ] - rz) <= brz, (what, sc[ks.RZ], rz, brz)
        assert abs(sc[WZ] - wz) <= bwz, (what, sc[WZ], wz, bwz)
        assert np.array_equal(sc, flex_scalars(float(sc[ks.RR]), float(sc[ks.RZ]), float(sc[WZ]), first, sc0)), (what, sc)
        # r.r and r.z in the order of the pass it is a twin of
        sc1 = sc0.copy()
        K.pcg_update(2, 0, None, r.copy(), None, None, z.copy(), None, first, sc1)
        assert sc[ks.RR] == sc1[ks.RR] and sc[ks.RZ] == sc1[ks.RZ], (what, sc, sc1)
    return sc


@pytest.mark.parametrize("integer", [True, False], ids=["int", "real"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_dots_wz_against_the_exact_dot(capi, K, shape, integer):
    g = shape_of(*shape)
    r, z, w = wz_data(g, integer, 2100)
    for n, rho in enumerate([4.0, 0.5, -2.0]):
        alpha = ALPHAS[n] if integer else -0.4142
        sc = check_dots_wz(capi, K, g, r, z, w, rho if integer else 0.77 * rho, alpha, False, integer)
        assert sc[ks.BETA] != 0.0
    sc = check_dots_wz(capi, K, g, r, z, w, 4.0, 0.5, True, integer)  # first: beta = 0, the dots still stored
    assert sc[ks.BETA] == 0.0 and sc[ks.RHO] == sc[ks.RZ] and sc[WZ] != 107.0
    sc = check_dots_wz(capi, K, g, r, z, w, 0.0, 0.5, False, integer)  # rho = 0 on entry
    assert sc[ks.BETA] == 0.0 and sc[ks.RHO] == sc[ks.RZ]


def test_dots_wz_refusals(capi, K):
    g = (5, 6, 7)
    f = pb.uniform(g, 1, -1, 1)
    sc = block(3.0, 0.5)
    with pytest.raises(RuntimeError):
        K.pcg_dots_wz(f, f, None, False, sc)
    with pytest.raises(RuntimeError):
        K.pcg_dots_wz(np.zeros((2, 5)), np.zeros((2, 5)), np.zeros((2, 5)), False, sc)
    ptr, u = (lambda a: a.ctypes.data_as(capi.P)), capi.u
    f2 = np.stack([f, f])
    for nrhs in (0, 33):
        assert capi.lib.cedar_amd_pcg_dots_wz_many(nrhs, u(1), ptr(f2), ptr(f2), ptr(f2), u(7), u(6), u(5), 0, ptr(sc)) == -1
    assert np.array_equal(sc, block(3.0, 0.5))


# ---------------------------------------------------------------- 2. the batched pass
@pytest.mark.parametrize("integer", [True, False], ids=["int", "real"])
@pytest.mark.parametrize("shape", [(5, 2100), (1030, 7), (129, 6, 5), (7, 50, 47)], ids=str)
def test_dots_wz_many_item_by_item(capi, K, shape, integer):
    """nrhs 1, 3, 9 (nine: a second ITEM_CHUNK) of nrhs + 1 items: item m's block is the single pass' on item m, a clear
    bit of `active` and the item beyond nrhs keep their block (the slab comes from the library's pool and cannot be seen
    from here; the kernel skips an item's slab where it skips its sums)"""
    g = shape_of(*shape)
    for nrhs in (1, 3, 9):
        n = nrhs + 1
        per = [wz_data(g, integer, 2300 + 17 * m) for m in range(n)]
        r, z, w = (np.stack([per[m][t] for m in range(n)]) for t in range(3))
        sc0 = np.stack([block(4.0 + m if integer else 0.77 + m, ALPHAS[m % 3] if integer else -0.4142 + 0.1 * m) for m in range(n)])
        single = []
        for m in range(n):
            s1 = sc0[m].copy()
            K.pcg_dots_wz(r[m], z[m], w[m], False, s1)
            single.append(s1)
        for active in (None, 0b101010101 & ((1 << nrhs) - 1)):
            for first in (False, True):
                dr, dz, dw = (capi.DeviceArray.from_numpy(a) for a in (r, z, w))
                sc = sc0.copy()
                K.pcg_dots_wz_many(dr, dz, dw, first, sc, nrhs=nrhs, active=active)
                act = (1 << nrhs) - 1 if active is None else active
                for d, a in ((dr, r), (dz, z), (dw, w)):
                    assert np.array_equal(d.numpy(), a)
                    d.free()
                for m in range(n):
                    what = (g, nrhs, m, active, first, integer)
                    if m >= nrhs or not (act >> m) & 1:
                        assert np.array_equal(sc[m], sc0[m]), ("touched", what)
                        continue
                    want = single[m] if not first else flex_scalars(single[m][ks.RR], single[m][ks.RZ], single[m][WZ], True, sc0[m])
                    assert np.array_equal(sc[m], want), (what, sc[m], want)
                    if integer:
                        dots = [exact_dot(a[m], b[m], True)[0] for a, b in ((r, r), (r, z), (w, z))]
                        assert np.array_equal(sc[m], flex_scalars(*dots, first, sc0[m])), (what, sc[m], dots)


# ---------------------------------------------------------------- 3. the solver against the statement
V21, V12, V20 = dict(nrelax_pre=2, nrelax_post=1), dict(nrelax_pre=1, nrelax_post=2), dict(nrelax_pre=2, nrelax_post=0)
F11, F21 = dict(nrelax_pre=1, nrelax_post=1, cycle="f"), dict(nrelax_pre=2, nrelax_post=1, cycle="f")
CASES = [
    ("fe3-v21", lambda: pb.fe3(25, 22, 19), V21),
    ("fe3-v12", lambda: pb.fe3(25, 22, 19), V12),
    ("fe3-v20", lambda: pb.fe3(25, 22, 19), V20),
    ("fe3-f11", lambda: pb.fe3(25, 22, 19), F11),
    ("fe3-f21", lambda: pb.fe3(25, 22, 19), F21),
    ("poisson3-v21", lambda: pb.poisson3(23, 21, 19), V21),
    ("poisson3-v20", lambda: pb.poisson3(23, 21, 19), V20),
    ("poisson3-f21", lambda: pb.poisson3(23, 21, 19), F21),
    ("poisson2-v21", lambda: pb.poisson2(63, 57), V21),
    ("poisson2-f21", lambda: pb.poisson2(63, 57), F21),
    ("varcoef9-s1-v21", lambda: pb.varcoef9(65, 60, sigma=1.0), V21),
    ("aniso9-linexy-v21", lambda: pb.aniso9(64, 48), dict(relax="line-xy", **V21)),
    ("fe3-164rows-v21", lambda: pb.fe3(24, 164, 12), V21),  # the partial-sum sweep level
    ("fe3-planexy-v21", lambda: pb.fe3(13, 12, 11), dict(relax="plane-xy", **V21)),
    ("fe3-planexy-v11", lambda: pb.fe3(13, 12, 11),
     dict(relax="plane-xy", nrelax_pre=1, nrelax_post=1, plane={"nrelax_pre": 1, "nrelax_post": 1})),
]


def fields(so):
    g = so.shape[1:]
    return ps.random_field(g, 17), ps.random_field(g, 23)


@pytest.mark.parametrize("mk", [lambda: pb.fe3(25, 22, 19), lambda: pb.poisson3(23, 21, 19)], ids=["fe3", "poisson3"])
def test_a_handle_without_post_smoothing_cycles_as_the_oracle(capi, oracle, mk):
    """V(2,0), before the cases that use it as a preconditioner: two cycles of the handle against the oracle's"""
    so = mk()
    b, x0 = fields(so)
    s = capi.Solver(so, **V20)
    ml = oracle.ml_create(so, **V20)
    try:
        x, xo = x0.copy(), x0.copy()
        for _ in range(2):
            s.vcycle(x, b)
            ml.vcycle(xo, b)
            assert np.max(np.abs(x - xo)) <= 1e-12 * np.max(np.abs(xo))
        assert not np.array_equal(x, x0)
    finally:
        s.close()
        ml.close()


@pytest.mark.parametrize("name,mk,st", CASES, ids=[c[0] for c in CASES])
def test_fcg_parity_with_statement(capi, oracle, name, mk, st):
    so = mk()
    b, x0 = fields(so)
    s = capi.Solver(so, **st)
    ml = oracle.ml_create(so, **st)
    try:
        x = x0.copy()
        h = s.fcg(b, x, tol=1e-10, max_iter=40)
        xs = x0.copy()
        ns, hs = fs.fcg(oracle, so, b, xs, ml=ml, tol=1e-10, max_iter=40)
        print(name, "device", len(h) - 1, "statement", ns, "max rel diff",
              np.max(np.abs(h[1:min(len(h), len(hs))] / hs[1:min(len(h), len(hs))] - 1)))
        compare_hist(h, hs, len(h) - 1, ns)
        assert h[-1] < 1e-10 and ns <= 10
    finally:
        s.close()
        ml.close()


# ---------------------------------------------------------------- 4. the robustness case
def test_fcg_keeps_its_iteration_count_without_post_smoothing(capi):
    """poisson3 V(2,0): the standard beta needs 20 iterations (tests/test_fcg_statement.py), the flexible one 10"""
    so = pb.poisson3(23, 21, 19)
    b, x = fields(so)
    s = capi.Solver(so, **V20)
    try:
        h = s.fcg(b, x, tol=1e-10, max_iter=40)
        print("iterations", len(h) - 1)
        assert len(h) - 1 <= 11 and h[-1] < 1e-10, h
    finally:
        s.close()


# ---------------------------------------------------------------- 5. symmetric settings
@pytest.mark.parametrize("mk,st", [(lambda: pb.fe3(25, 22, 19), dict(nrelax_pre=1, nrelax_post=1)),
                                   (lambda: pb.varcoef9(65, 60, sigma=8.0), dict(nrelax_pre=2, nrelax_post=2))],
                         ids=["fe3-v11", "varcoef9-v22"])
def test_fcg_reproduces_pcg_on_a_symmetric_cycle(capi, mk, st):
    so = mk()
    b, x0 = fields(so)
    s = capi.Solver(so, **st)
    try:
        x, xp = x0.copy(), x0.copy()
        h = s.fcg(b, x, tol=1e-10, max_iter=40)
        hp = s.pcg(b, xp, tol=1e-10, max_iter=40)
        compare_hist(h, hp, len(h) - 1, len(hp) - 1)
        assert h[-1] < 1e-10
    finally:
        s.close()


@pytest.mark.parametrize("precon", ["none", "diag"])
def test_fcg_without_the_cycle_is_pcg(capi, precon):
    so = pb.poisson2(15, 13)
    g = so.shape[1:]
    b = ps.random_field(g, 4)
    s = capi.Solver(so)  # V(2,1): no obstacle without the cycle
    try:
        x, xp = np.zeros(g), np.zeros(g)
        h = s.fcg(b, x, tol=1e-10, max_iter=60, precon=precon)
        hp = s.pcg(b, xp, tol=1e-10, max_iter=60, precon=precon)
        assert len(h) > 3 and np.array_equal(h, hp) and np.array_equal(x, xp)
    finally:
        s.close()


@pytest.mark.parametrize("stop", ["abs_l2", "abs_m", "rel_m"])
def test_fcg_stop_tests(capi, oracle, stop):
    """abs_m / rel_m: the M-norm branch, where the new pass runs before the stop test"""
    so = pb.fe3(15, 14, 13)
    g = so.shape[1:]
    b = ps.random_field(g, 8)
    tol = 1e-9 if stop.startswith("rel") else 1e-9 * np.linalg.norm(ps.inner(b))
    s = capi.Solver(so, **V21)
    ml = oracle.ml_create(so, **V21)
    try:
        x = np.zeros(g)
        h = s.fcg(b, x, tol=tol, stop=stop)
        xs = np.zeros(g)
        ns, hs = fs.fcg(oracle, so, b, xs, ml=ml, tol=tol, stop=stop)
        compare_hist(h, hs, len(h) - 1, ns)
        assert 2 < ns < 50
    finally:
        s.close()
        ml.close()


# ---------------------------------------------------------------- 6. batch
def batch_fields(so, n=3):
    g = so.shape[1:]
    return (np.stack([ps.random_field(g, 17 + m) for m in range(n)]), np.stack([ps.random_field(g, 23 + m) for m in range(n)]))


@pytest.mark.parametrize("mk", [lambda: pb.fe3(25, 22, 19), lambda: pb.poisson3(23, 21, 19), lambda: pb.varcoef9(65, 60)],
                         ids=["fe3", "poisson3", "varcoef9"])
def test_fcg_many_equals_fcg_item_by_item(capi, mk):
    """V(2,1); every 27-point level of these shapes is below 160 rows: reference order on both handles"""
    so = mk()
    b, x0 = batch_fields(so)
    kw = dict(tol=1e-10, max_iter=40)
    sm = capi.Solver(so, max_rhs=3, **V21)
    x = x0.copy()
    hist, iters = sm.fcg_many(b, x, **kw)
    # nrhs == 1 on the batch handle: the single-vector path
    x1 = x0[:1].copy()
    hist1, iters1 = sm.fcg_many(b[:1], x1, **kw)
    sm.close()
    s1 = capi.Solver(so, **V21)
    for m in range(3):
        xm = x0[m].copy()
        h = s1.fcg(b[m], xm, **kw)
        assert iters[m] == len(h) - 1 > 2 and h[-1] < 1e-10, (m, iters, h)
        assert np.array_equal(hist[m], h), (m, hist[m], h)
        assert np.array_equal(x[m], xm), (m, np.max(np.abs(x[m] - xm)))
        if m == 0:
            assert iters1 == [len(h) - 1] and np.array_equal(hist1[0], h) and np.array_equal(x1[0], xm)
    s1.close()


def test_fcg_many_freezes_items_and_keeps_sentinels(capi):
    so = pb.fe3(25, 22, 19)
    b, _ = batch_fields(so, 4)
    b[1] = 0.0  # nothing to do for this item: frozen at once, the others go on
    b[2] *= 1e-4  # an absolute target: this item stops earlier than items 0 and 3
    kw = dict(stop="abs_l2", tol=1e-9 * np.linalg.norm(ps.inner(b[0])), max_iter=30)
    s1 = capi.Solver(so, **V21)
    single, xs = [], []
    for m in range(3):
        x1 = np.zeros_like(b[m])
        single.append(s1.fcg(b[m], x1, **kw))
        xs.append(x1)
    s1.close()
    n1 = [len(h) - 1 for h in single]
    assert n1[1] == 0 and 0 < n1[2] < n1[0], n1
    sentinel = -7.25
    s = capi.Solver(so, max_rhs=4, **V21)
    buf = np.full((4, kw["max_iter"] + 1), sentinel)
    x = np.zeros_like(b)
    x[3] = sentinel
    st = capi.PcgSettings(kw["max_iter"], kw["tol"], capi.PCG_STOP["abs_l2"], capi.PCG_PRECON["mg"], 1)
    it = np.full(4, 77, dtype=np.int32)
    rc = capi.lib.cedar_amd_solver_fcg_many(s.h, 3, b.ctypes.data, x.ctypes.data, C.byref(st), buf.ctypes.data,
                                            it.ctypes.data_as(C.POINTER(C.c_int)))
    s.close()
    assert it.tolist() == n1 + [77] and rc == max(n1)
    for m in range(3):
        assert np.array_equal(buf[m, : n1[m] + 1], single[m]), m
        assert np.all(buf[m, n1[m] + 1:] == sentinel), m
        assert np.array_equal(x[m], xs[m]), m
    assert buf[1, 0] == 0.0 and np.all(x[1] == 0.0)
    assert np.all(buf[3] == sentinel) and np.all(x[3] == sentinel)  # the item beyond nrhs


# ---------------------------------------------------------------- 7. determinism
def test_fcg_is_deterministic(capi):
    so = pb.fe3(24, 164, 12)
    b, x0 = fields(so)
    s = capi.Solver(so, **V21)
    try:
        out = []
        for _ in range(2):
            x = x0.copy()
            h = s.fcg(b, x, tol=1e-10, max_iter=40)
            out.append((x, h))
        assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and len(out[0][1]) > 3
    finally:
        s.close()


# ---------------------------------------------------------------- 8. refusals and non-interference
def raw_fcg(capi, h, b, x, hist, **kw):
    p = capi.PcgSettings(kw.get("max_iter", 20), 1e-8, kw.get("stop_test", 1), kw.get("precon", 3), kw.get("nmg_cycles", 1))
    return capi.lib.cedar_amd_solver_fcg(h, b.ctypes.data, x.ctypes.data, C.byref(p), hist.ctypes.data)


def raw_fcg_many(capi, h, nrhs, b, x, hist, it):
    p = capi.PcgSettings(20, 1e-8, 1, 3, 1)
    return capi.lib.cedar_amd_solver_fcg_many(h, nrhs, b.ctypes.data, x.ctypes.data, C.byref(p), hist.ctypes.data,
                                              it.ctypes.data_as(C.POINTER(C.c_int)))


def test_fcg_refusals(capi, capfd):
    sentinel = -3.5
    so = pb.poisson2(31, 29)
    g = so.shape[1:]
    b = ps.random_field(g, 1)

    def refused(h, text, **kw):
        x, hist = np.full(g, sentinel), np.full(21, sentinel)
        capfd.readouterr()
        assert raw_fcg(capi, h, b, x, hist, **kw) == -1
        err = capfd.readouterr().err
        assert text in err and "cedar_amd_solver_fcg" in err, (text, err)
        assert np.all(x == sentinel) and np.all(hist == sentinel)

    refused(None, "")
    s = capi.Solver(so)
    try:
        refused(s.h, "stop_test must be 0..3", stop_test=7)
        refused(s.h, "precon must be 1..3", precon=0)
        refused(s.h, "nmg_cycles must be at least 1", nmg_cycles=0)
        refused(s.h, "max_iter must not be negative", max_iter=-1)
        x = np.full(g, sentinel)
        with pytest.raises(RuntimeError):
            s.fcg(b, x, nmg_cycles=0)
        assert np.all(x == sentinel)
        x = np.zeros(g)
        h = s.fcg(b, x)  # the handle stays usable
        assert 1 < len(h) - 1 < 50 and h[-1] < 1e-8
    finally:
        s.close()
    per = (True, False)
    sop = pb.periodic_poisson2(32, 32, per)
    sp = capi.Solver(sop, nrelax_pre=1, nrelax_post=1, ibc=pb.ibc_of(per))
    try:
        gp = sop.shape[1:]
        x, hist = np.full(gp, sentinel), np.full(21, sentinel)
        capfd.readouterr()
        assert raw_fcg(capi, sp.h, ps.random_field(gp, 1), x, hist) == -1
        assert "periodic" in capfd.readouterr().err and np.all(x == sentinel) and np.all(hist == sentinel)
    finally:
        sp.close()
    # the batch call: an F-cycle handle, and more items than the handle holds
    bb = np.stack([b, b, b])
    for st, nrhs, text in ((dict(cycle="f", max_rhs=2), 1, "V-cycle"), (dict(max_rhs=2), 3, "exceeds the handle's max_rhs")):
        sm = capi.Solver(so, **st)
        try:
            x, hist, it = np.full_like(bb, sentinel), np.full((3, 21), sentinel), np.full(3, 77, dtype=np.int32)
            capfd.readouterr()
            assert raw_fcg_many(capi, sm.h, nrhs, bb, x, hist, it) == -1
            err = capfd.readouterr().err
            assert text in err and "cedar_amd_solver_fcg_many" in err, (text, err)
            assert np.all(x == sentinel) and np.all(hist == sentinel) and np.all(it == 77)
            with pytest.raises(RuntimeError):
                sm.fcg_many(bb[:nrhs], x[:nrhs])
            assert np.all(x == sentinel)
        finally:
            sm.close()
    assert raw_fcg_many(capi, None, 1, bb, bb.copy(), np.zeros((3, 21)), np.zeros(3, dtype=np.int32)) == -1


def test_fcg_leaves_pcg_as_it_was(capi):
    """the two share the Krylov storage and the scalar block: pcg's bits before, after a refused and after a served fcg"""
    so = pb.fe3(25, 22, 19)
    b, x0 = fields(so)
    s = capi.Solver(so, nrelax_pre=1, nrelax_post=1)
    try:
        def pcg():
            x = x0.copy()
            return x, s.pcg(b, x, tol=1e-10, max_iter=40)

        first = pcg()
        x = x0.copy()
        with pytest.raises(RuntimeError):
            s.fcg(b, x, stop="rel_l2", nmg_cycles=0)
        assert np.array_equal(x, x0)
        after_refused = pcg()
        h = s.fcg(b, x, tol=1e-10, max_iter=40)
        assert h[-1] < 1e-10
        after_served = pcg()
        for got in (after_refused, after_served):
            assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1])
    finally:
        s.close()


# ---------------------------------------------------------------- 9. single-precision operator in the cycle
def test_fcg_on_a_single_precision_cycle_reaches_the_fp64_residual(capi, oracle):
    so = pb.fe3(40, 33, 50)
    b, x0 = fields(so)
    r0 = np.linalg.norm(ps.inner(b - ps.apply_A(oracle, so, x0)))
    counts = []
    for switch in (False, True):
        s = capi.Solver(so, **V21)
        try:
            if switch:
                assert s.use_fp32_operator(1) >= 2  # every smoothed level, as tests/test_gpu_op32.py switches them
            x = x0.copy()
            h = s.fcg(b, x, tol=1e-10, max_iter=40)
            counts.append(len(h) - 1)
            true = np.linalg.norm(ps.inner(b - ps.apply_A(oracle, so, x))) / r0
            print("fp32" if switch else "fp64", "iterations", len(h) - 1, "recurrence", h[-1], "true", true)
            assert h[-1] < 1e-10
            if switch:
                assert true < 1e-10, (true, h)
        finally:
            s.close()
    assert abs(counts[0] - counts[1]) <= 1, counts
