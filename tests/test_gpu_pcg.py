"""Multigrid-preconditioned conjugate gradients on the device (cedar_amd_solver_pcg / _precondition, Solver.pcg,
solver::pcg of the C++ mirror) against the numpy statement of tests/pcg_statement.py on the oracle."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import pcg_statement as ps
import problems as pb

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def capi():
    from cedar_amd import capi
    assert capi.device_count() >= 1, "no GPU visible"
    return capi


def compare_hist(h, hs, n, ns):
    assert abs(n - ns) <= 1, (n, ns, h, hs)
    m = min(len(h), len(hs))
    np.testing.assert_allclose(h[0], hs[0], rtol=1e-10)
    keep = hs[1:m] >= 1e-10
    np.testing.assert_allclose(h[1:m][keep], hs[1:m][keep], rtol=1e-8)


PARITY = [
    ("poisson2-v11", lambda: pb.poisson2(63, 57), dict(nrelax_pre=1, nrelax_post=1)),
    ("poisson2-v22", lambda: pb.poisson2(63, 57), dict(nrelax_pre=2, nrelax_post=2)),
    ("varcoef9-s1", lambda: pb.varcoef9(65, 60, sigma=1.0), dict(nrelax_pre=1, nrelax_post=1)),
    ("varcoef9-s8", lambda: pb.varcoef9(65, 60, sigma=8.0), dict(nrelax_pre=2, nrelax_post=2)),
    ("aniso9-linexy", lambda: pb.aniso9(64, 48), dict(relax="line-xy", nrelax_pre=1, nrelax_post=1)),
    ("poisson3-v11", lambda: pb.poisson3(23, 21, 19), dict(nrelax_pre=1, nrelax_post=1)),
    ("poisson3-v22", lambda: pb.poisson3(23, 21, 19), dict(nrelax_pre=2, nrelax_post=2)),
    ("fe3-v11", lambda: pb.fe3(25, 22, 19), dict(nrelax_pre=1, nrelax_post=1)),
    ("fe3-164rows", lambda: pb.fe3(24, 164, 12), dict(nrelax_pre=1, nrelax_post=1)),
    # rows long enough for the wider launch variants of krylov.hip: pcg_dir27<128> / <256>, pcg_dir7 with 128 / 256 lanes,
    # pcg_dir2 with several workgroups per row, a second trip of pcg_upd's pair loop
    ("fe3-nx140", lambda: pb.fe3(140, 12, 10), dict(nrelax_pre=1, nrelax_post=1)),
    ("fe3-nx300", lambda: pb.fe3(300, 9, 8), dict(nrelax_pre=1, nrelax_post=1)),
    ("poisson3-nx140", lambda: pb.poisson3(140, 10, 9), dict(nrelax_pre=1, nrelax_post=1)),
    ("poisson3-nx300", lambda: pb.poisson3(300, 9, 8), dict(nrelax_pre=1, nrelax_post=1)),
    ("poisson2-nx600", lambda: pb.poisson2(600, 9), dict(nrelax_pre=1, nrelax_post=1)),
    ("poisson2-nx600-linexy", lambda: pb.poisson2(600, 9), dict(relax="line-xy", nrelax_pre=1, nrelax_post=1)),
    ("varcoef9-nx300", lambda: pb.varcoef9(300, 40), dict(nrelax_pre=1, nrelax_post=1)),
]
# The gallery's Poisson operators are scaled by the mesh widths: at these extents the x coupling is over a hundred times
# the others, point relaxation does not smooth that, and the numpy statement itself is at 2e-6 .. 7e-4 after 40
# iterations.  These cases compare the 40 iterations entry by entry (same criterion) and require of the device exactly
# what the statement does: that it has not converged either.
SLOW = {"poisson3-nx140", "poisson3-nx300", "poisson2-nx600"}


@pytest.mark.parametrize("name,mk,st", PARITY, ids=[c[0] for c in PARITY])
def test_pcg_parity_with_statement(capi, oracle, name, mk, st):
    so = mk()
    g = so.shape[1:]
    b = ps.random_field(g, 17)
    x0 = ps.random_field(g, 23)
    s = capi.Solver(so, **st)
    ml = oracle.ml_create(so, **st)
    try:
        x = x0.copy()
        h = s.pcg(b, x, tol=1e-10, max_iter=40)
        xs = x0.copy()
        ns, hs = ps.pcg(oracle, so, b, xs, ml=ml, tol=1e-10, max_iter=40)
        compare_hist(h, hs, len(h) - 1, ns)
        if name in SLOW:
            assert ns == 40 and len(h) == 41 and hs[-1] >= 1e-10 and h[-1] >= 1e-10
        else:
            assert h[-1] < 1e-10
    finally:
        s.close()
        ml.close()


@pytest.mark.parametrize("precon", ["none", "diag"])
def test_pcg_plain_and_jacobi_cg(capi, oracle, precon):
    so = pb.poisson2(15, 13)
    g = so.shape[1:]
    b = ps.random_field(g, 4)
    s = capi.Solver(so, nrelax_pre=1, nrelax_post=1)
    try:
        x = np.zeros(g)
        h = s.pcg(b, x, tol=1e-10, max_iter=60, precon=precon)
        xs = np.zeros(g)
        ns, hs = ps.pcg(oracle, so, b, xs, precon=precon, tol=1e-10, max_iter=60)
        compare_hist(h, hs, len(h) - 1, ns)
        np.testing.assert_allclose(x, xs, rtol=1e-8, atol=1e-10 * np.abs(xs).max())
    finally:
        s.close()


@pytest.mark.parametrize("stop", ["abs_l2", "abs_m", "rel_m"])
def test_pcg_stop_tests(capi, oracle, stop):
    so = pb.fe3(15, 14, 13)
    g = so.shape[1:]
    b = ps.random_field(g, 8)
    tol = 1e-9 if stop.startswith("rel") else 1e-9 * np.linalg.norm(ps.inner(b))
    s = capi.Solver(so, nrelax_pre=1, nrelax_post=1)
    ml = oracle.ml_create(so, nrelax_pre=1, nrelax_post=1)
    try:
        x = np.zeros(g)
        h = s.pcg(b, x, tol=tol, stop=stop)
        xs = np.zeros(g)
        ns, hs = ps.pcg(oracle, so, b, xs, ml=ml, tol=tol, stop=stop)
        compare_hist(h, hs, len(h) - 1, ns)
    finally:
        s.close()
        ml.close()


ENERGY = [
    ("poisson2", lambda: pb.poisson2(47, 39)),
    ("poisson3", lambda: pb.poisson3(19, 17, 15)),
    ("contrast7", lambda: ps.high_contrast7(24, 24, 24)),
]


@pytest.mark.parametrize("name,mk", ENERGY, ids=[c[0] for c in ENERGY])
def test_pcg_energy_norm_optimality(capi, oracle, name, mk):
    """b = A x*, x0 = 0: ||x* - x_k^PCG||_A <= (1 + 1e-8) ||x* - x_k^MG||_A for k = 1..8"""
    so = mk()
    g = so.shape[1:]
    xs = ps.random_field(g, 31)
    b = ps.apply_A(oracle, so, xs)
    s = capi.Solver(so, nrelax_pre=1, nrelax_post=1)
    try:
        xmg = np.zeros(g)
        for k in range(1, 9):
            s.vcycle(xmg, b)
            x = np.zeros(g)
            h = s.pcg(b, x, max_iter=k, tol=0.0)
            assert len(h) == k + 1
            e_pcg, e_mg = ps.a_norm(oracle, so, xs - x), ps.a_norm(oracle, so, xs - xmg)
            assert e_pcg <= (1 + 1e-8) * e_mg, (k, e_pcg, e_mg)
    finally:
        s.close()


SYM = [
    ("point2", lambda: pb.varcoef9(33, 29, sigma=8.0), {}),
    ("point3", lambda: pb.fe3(13, 12, 11), {}),
    ("linexy2", lambda: pb.aniso9(40, 36), {"relax": "line-xy"}),
    # two levels: the plane solvers of a level are all built from the coefficients of its last plane (the reference's
    # copy_coeff), so the plane smoother is symmetric only where every plane has the same coefficients -- on the fine
    # 7-point level of Poisson, not on the Galerkin levels below it
    ("planexy3", lambda: pb.poisson3(12, 11, 10),
     {"relax": "plane-xy", "num_levels": 2, "plane": {"nrelax_pre": 1, "nrelax_post": 1}}),
]


@pytest.mark.parametrize("nu", [1, 2])
@pytest.mark.parametrize("name,mk,st", SYM, ids=[c[0] for c in SYM])
def test_precondition_is_symmetric(capi, name, mk, st, nu):
    so = mk()
    g = so.shape[1:]
    u, v = ps.random_field(g, 41), ps.random_field(g, 43)
    s = capi.Solver(so, nrelax_pre=nu, nrelax_post=nu, **st)
    try:
        mu, mv = np.zeros(g), np.zeros(g)
        s.precondition(mu, u)
        s.precondition(mv, v)
        lhs, rhs = ps.dot(mu, v), ps.dot(u, mv)
        assert abs(lhs - rhs) <= 1e-12 * np.linalg.norm(ps.inner(mu)) * np.linalg.norm(ps.inner(v)), (lhs, rhs)
        assert ps.dot(mu, u) > 0
    finally:
        s.close()


@pytest.mark.parametrize("mk", [lambda: pb.fe3(24, 164, 12), lambda: pb.varcoef9(65, 60, sigma=8.0)], ids=["fe3", "varcoef9"])
def test_pcg_is_deterministic(capi, mk):
    so = mk()
    g = so.shape[1:]
    b = ps.random_field(g, 5)
    s = capi.Solver(so, nrelax_pre=1, nrelax_post=1)
    try:
        out = []
        for _ in range(2):
            x = np.zeros(g)
            h = s.pcg(b, x, tol=1e-12, max_iter=30)
            out.append((x, h))
        assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    finally:
        s.close()


def test_pcg_edge_cases(capi):
    so = pb.poisson2(31, 31)  # integer coefficients (4, 1) on a square grid: A x is exact for integer x
    g = so.shape[1:]
    s = capi.Solver(so, nrelax_pre=1, nrelax_post=1)
    try:
        # b = 0, x0 = 0
        x = np.zeros(g)
        h = s.pcg(np.zeros(g), x)
        assert len(h) == 1 and h[0] == 0.0 and np.all(x == 0.0)
        # exact x0
        xs = np.round(ps.random_field(g, 3) * 8)
        b = np.zeros(g)
        capi.Kernels().matvec2(so, xs, b)
        x = xs.copy()
        h = s.pcg(b, x)
        assert len(h) == 1 and h[0] == 0.0 and np.array_equal(x, xs)
        # max_iter = 0: the initial residual only, x untouched
        x0 = ps.random_field(g, 9)
        x = x0.copy()
        h = s.pcg(b, x, max_iter=0)
        assert len(h) == 1 and h[0] > 0 and np.array_equal(x, x0)
        # the raw entry point with a NULL handle and with NULL settings (defaults)
        lib = capi.lib
        ps_ = capi.PcgSettings()
        lib.cedar_amd_default_pcg_settings(C.byref(ps_))
        assert (ps_.max_iter, ps_.tol, ps_.stop_test, ps_.precon, ps_.nmg_cycles) == (50, 1e-8, 1, 3, 1)
        assert lib.cedar_amd_solver_pcg(None, b.ctypes.data, x.ctypes.data, None, None) == -1
        lib.cedar_amd_solver_precondition(None, x.ctypes.data, b.ctypes.data)
        assert np.array_equal(x, x0)
        x = np.zeros(g)
        hist = np.zeros(51)
        n = lib.cedar_amd_solver_pcg(s.h, b.ctypes.data, x.ctypes.data, None, hist.ctypes.data)
        assert 0 < n < 50 and hist[n] < 1e-8 and np.all(np.isfinite(x))
    finally:
        s.close()


@pytest.mark.parametrize("kind", ["fcycle", "v21", "periodic", "plane-v21"])
def test_pcg_refusals(capi, kind):
    if kind == "fcycle":
        so, st = pb.poisson2(31, 29), dict(nrelax_pre=1, nrelax_post=1, cycle="f")
    elif kind == "v21":
        so, st = pb.poisson2(31, 29), dict(nrelax_pre=2, nrelax_post=1)
    elif kind == "periodic":
        per = (True, False)
        so, st = pb.periodic_poisson2(32, 32, per), dict(nrelax_pre=1, nrelax_post=1, ibc=pb.ibc_of(per))
    else:
        so, st = pb.poisson3(12, 11, 10), dict(relax="plane-xy", nrelax_pre=1, nrelax_post=1)  # plane-config V(2,1)
    g = so.shape[1:]
    s = capi.Solver(so, **st)
    try:
        x0 = ps.random_field(g, 2)
        b = ps.random_field(g, 1)
        x = x0.copy()
        with pytest.raises(RuntimeError):
            s.pcg(b, x)
        assert np.array_equal(x, x0)
        assert capi.lib.cedar_amd_solver_pcg(s.h, b.ctypes.data, x.ctypes.data, None, None) == -1
        assert np.array_equal(x, x0)
        z = x0.copy()
        s.precondition(z, b)
        assert np.array_equal(z, x0)
    finally:
        s.close()


def test_pcg_full_size_27pt_512(capi):
    """3D 27-point fe at 512^3, V(1,1): rel 1e-10, and the true residual agrees with the recursive one"""
    n = 512
    so, b = capi.gallery("fe3", (n, n, n))
    g = (n + 2,) * 3
    s = capi.Solver(so, nrelax_pre=1, nrelax_post=1, share_operator=True)
    try:
        x = capi.DeviceArray(g)
        x.zero()
        h = s.pcg(b, x, tol=1e-10, max_iter=50)
        assert h[-1] < 1e-10 and len(h) <= 30, h
        r = capi.DeviceArray(g)
        capi.Kernels().residual3(so, b, x, r)
        true = capi.lib.cedar_amd_l2norm(r.ptr, n + 2, n + 2, n + 2)
        assert abs(true - h[-1] * h[0]) <= 1e-11 * h[0], (true, h[-1] * h[0], h[0])
    finally:
        s.close()


def test_cxx_solver_pcg(capi, tmp_path):
    from test_cxx_api import build
    json.dump({"solver": {"cycle": {"nrelax-pre": 1, "nrelax-post": 1}},
               "pcg": {"max-iter": 30, "tol": 1e-10, "stop-test": "rel-l2", "precon": "mg", "nmg-cycles": 1}},
              open(tmp_path / "config.json", "w"))
    exe = tmp_path / "pcg"
    build("pcg.cc", exe)
    p = subprocess.run([str(exe), str(tmp_path)], check=True, capture_output=True, text=True)
    got = json.loads(p.stdout.strip().splitlines()[-1])
    so = pb.poisson2(41, 35)
    b = np.zeros(so.shape[1:])
    i = np.arange(1, 42)[None, :]
    j = np.arange(1, 36)[:, None]
    b[1:-1, 1:-1] = 1.0 / (1.0 + i + 2.0 * j)
    s = capi.Solver(so, nrelax_pre=1, nrelax_post=1)
    h2 = s.pcg(b, np.zeros_like(b), max_iter=30, tol=1e-10)
    s.close()
    so = pb.fe3(17, 15, 13)
    b = np.zeros(so.shape[1:])
    i = np.arange(1, 18)[None, None, :]
    j = np.arange(1, 16)[None, :, None]
    k = np.arange(1, 14)[:, None, None]
    b[1:-1, 1:-1, 1:-1] = 1.0 / (1.0 + i + 2.0 * j + 3.0 * k)
    s = capi.Solver(so, nrelax_pre=1, nrelax_post=1)
    h3 = s.pcg(b, np.zeros_like(b), max_iter=30, tol=1e-10)
    s.close()
    assert len(got["h2"]) == len(h2) > 2 and len(got["h3"]) == len(h3) > 2
    np.testing.assert_allclose(got["h2"], h2, rtol=1e-13)
    np.testing.assert_allclose(got["h3"], h3, rtol=1e-13)
