"""Preconditioned conjugate gradients on a rank grid (cedar_amd_dist3_pcg / cedar_amd_dist2_pcg, DistSolver3.pcg /
DistSolver2.pcg) against the single-domain cedar_amd_solver_pcg on the same global problem.

As in tests/test_gpu_dist.py: 2 and 4 rank processes share device 0 over the host-staged transport (SocketComm handed in as
the ABI's transport table), one case after another, no torch in any rank process.  The single-domain run is a child process
of its own.  Criterion of the distributed V-cycle tests: histories to rtol 1e-10 (atol 1e-14 on the relative entries), the
gathered iterate to 1e-10 max|x|.  The global scalars are summed in rank order, so every rank must hold the same bits."""
import multiprocessing as mp
import os
import socket
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _paths():
    for p in (HERE, ROOT, os.path.join(ROOT, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)


def _global_problem(c):
    """the global operator, right-hand side and initial guess of a case"""
    import pcg_statement as ps
    import problems as pb
    gn = [c["n"][d] * c["pgrid"][d] for d in range(len(c["n"]))]
    so = getattr(pb, c["op"])(*gn)
    g = so.shape[1:]
    return so, ps.random_field(g, 17), ps.random_field(g, 23), g


def _local(c, rank, a):
    """this rank's box (owned points + one ghost layer) of a global array; ghost layer zero"""
    import problems as pb
    n, p = c["n"], c["pgrid"]
    if len(n) == 3:
        co = (rank % p[0], (rank // p[0]) % p[1], rank // (p[0] * p[1]))
    else:
        co = (rank % p[0], rank // p[0])
    sl = tuple(slice(co[d] * n[d], co[d] * n[d] + n[d] + 2) for d in reversed(range(len(n))))
    lead = (slice(None),) * (a.ndim - len(n))
    loc = np.ascontiguousarray(a[lead + sl])
    return loc * pb.interior_mask(loc.shape[len(lead):])


def _solver_kw(c):
    kw = dict(nrelax_pre=c.get("nu", (1, 1))[0], nrelax_post=c.get("nu", (1, 1))[1])
    if len(c["n"]) == 2:
        kw["relax"] = c.get("relax", "point")
    return kw


def _rank(rank, world, port, c, outdir):
    _paths()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["RANK"], os.environ["WORLD_SIZE"] = str(rank), str(world)
    os.environ.update(c.get("env", {}))
    import faulthandler
    faulthandler.dump_traceback_later(int(os.environ.get("CEDAR_AMD_TEST_STUCK_S", "300")), exit=True)  # a stuck rank says where
    from cedar_amd import capi
    from cedar_amd.comm import NativeComm, SocketComm
    from cedar_amd.dist3 import DistSolver2, DistSolver3
    assert "torch" not in sys.modules
    capi.set_device(0)
    comm = NativeComm(rank, world) if c.get("rccl") else SocketComm(rank, world)
    out = lambda name: os.path.join(outdir, f"{name}_r{rank}.npy")  # noqa: E731
    try:
        so, b, x0, g = _global_problem(c)
        A = capi.DeviceArray.from_numpy(_local(c, rank, so))
        bl = capi.DeviceArray.from_numpy(_local(c, rank, b))
        Cls = DistSolver3 if len(c["n"]) == 3 else DistSolver2
        s = Cls(comm, rank, world, A, pgrid=c["pgrid"], agglomerate_below=c.get("agg", 64), **_solver_kw(c))
        if len(c["n"]) == 3:
            np.save(out("levels"), np.array([capi.lib.cedar_amd_dist3_distributed_levels(s.h), s.chain_levels]))
        for i, run in enumerate(c.get("runs", [])):
            for rep in range(2 if c.get("repeat") else 1):
                x = capi.DeviceArray.from_numpy(_local(c, rank, x0))
                h = s.pcg(bl, x, **run)
                np.save(out(f"h{i}_{rep}"), h)
                np.save(out(f"x{i}_{rep}"), x.numpy())
        if c.get("refuse"):
            x = capi.DeviceArray.from_numpy(_local(c, rank, x0))
            try:
                s.pcg(bl, x, tol=1e-8, max_iter=10)
                refused = False
            except RuntimeError:
                refused = True
            untouched = bool(np.array_equal(x.numpy(), _local(c, rank, x0)))
            # the ranks are still in step: a run the settings allow goes through on every rank
            h = s.pcg(bl, x, tol=1e-6, max_iter=5, precon="diag")
            np.save(out("refuse"), np.array([refused, untouched, len(h) >= 2]))
        if c.get("sym"):
            import pcg_statement as ps
            for name, seed in (("u", 41), ("v", 43)):
                r = capi.DeviceArray.from_numpy(_local(c, rank, ps.random_field(g, seed)))
                z = capi.DeviceArray(r.shape)
                s.precondition(z, r)
                np.save(out("M" + name), z.numpy())
        s.close()
    finally:
        comm.close()


def _single(c, outdir):
    """the same runs on one domain: cedar_amd_solver_pcg (Solver.pcg)"""
    _paths()
    from cedar_amd import capi
    capi.set_device(0)
    so, b, x0, _ = _global_problem(c)
    s = capi.Solver(so, **_solver_kw(c))
    for i, run in enumerate(c.get("runs", [])):
        x = x0.copy()
        np.save(os.path.join(outdir, f"hs{i}.npy"), s.pcg(b, x, **run))
        np.save(os.path.join(outdir, f"xs{i}.npy"), x)
    s.close()


def _spawn(target, nproc, args):
    ctx = mp.get_context("spawn")
    ps = [ctx.Process(target=target, args=((r, nproc) if nproc else ()) + args) for r in range(max(nproc, 1))]
    for p in ps:
        p.start()
    for p in ps:
        p.join(600)
    bad = [p.exitcode for p in ps if p.exitcode != 0]
    for p in ps:
        if p.is_alive():
            p.kill()
    assert not bad, f"processes failed: exit codes {bad}"


def _world(c):
    return int(np.prod(c["pgrid"]))


def _run(c, tmp_path, single=True):
    _spawn(_rank, _world(c), (_free_port(), c, str(tmp_path)))
    if single and c.get("runs"):
        _spawn(_single, 0, (c, str(tmp_path)))


def _gather(c, tmp_path, name):
    """the owned points of every rank's box, put together"""
    n, p = c["n"], c["pgrid"]
    gshape = tuple(n[d] * p[d] for d in reversed(range(len(n))))
    out = np.zeros(gshape)
    for r in range(_world(c)):
        co = (r % p[0], (r // p[0]) % p[1], r // (p[0] * p[1])) if len(n) == 3 else (r % p[0], r // p[0])
        own = np.load(tmp_path / f"{name}_r{r}.npy")[(slice(1, -1),) * len(n)]
        out[tuple(slice(co[d] * n[d], co[d] * n[d] + n[d]) for d in reversed(range(len(n))))] = own
    return out


def _check_parity(c, tmp_path, i):
    hs = np.load(tmp_path / f"hs{i}.npy")
    h = np.load(tmp_path / f"h{i}_0_r0.npy")
    assert len(h) == len(hs), (h, hs)
    np.testing.assert_allclose(h[0], hs[0], rtol=1e-10)
    np.testing.assert_allclose(h[1:], hs[1:], rtol=1e-10, atol=1e-14)
    for r in range(1, _world(c)):  # the same bits on every rank
        assert np.array_equal(np.load(tmp_path / f"h{i}_0_r{r}.npy"), h), r
    xs = np.load(tmp_path / f"xs{i}.npy")[(slice(1, -1),) * len(c["n"])]
    x = _gather(c, tmp_path, f"x{i}_0")
    assert np.max(np.abs(x - xs)) <= 1e-10 * np.max(np.abs(xs))


MG = dict(tol=1e-10, max_iter=40)
FRUN2 = {"CEDAR_AMD_FRUN": "2"}  # small boxes take the partial-sum sweep behind the boundary-first chain
PARITY = [
    ("3d7-1x1x2", dict(n=(16, 16, 8), pgrid=(1, 1, 2), op="poisson3")),
    ("3d7-2x1x1", dict(n=(8, 16, 16), pgrid=(2, 1, 1), op="poisson3")),
    ("3d7-2x2x1", dict(n=(8, 8, 16), pgrid=(2, 2, 1), op="poisson3", nu=(2, 2))),
    ("3d27-1x1x2", dict(n=(16, 16, 8), pgrid=(1, 1, 2), op="fe3")),
    ("3d27-2x1x1", dict(n=(8, 16, 16), pgrid=(2, 1, 1), op="fe3", nu=(2, 2))),
    ("3d27-2x2x1-chain", dict(n=(16, 32, 8), pgrid=(2, 2, 1), op="fe3", env=FRUN2, chain=1)),
    ("3d27-2x2x1-rowclass", dict(n=(16, 16, 8), pgrid=(2, 2, 1), op="fe3", env={"CEDAR_AMD_DIST_CHAIN": "0"}, chain=0)),
    # levels 0 and 1 distributed, level 2 (8 x 8 x 8 per rank) gathered onto every rank
    ("3d27-1x1x2-two-levels", dict(n=(32, 32, 16), pgrid=(1, 1, 2), op="fe3", agg=4, levels=3)),
    # odd extents along unsplit directions (create asks for even extents along split directions only).  x split, odd ny:
    # the level is offered the partial-sum sweep but the masked launch takes even nx and ny only, so it keeps the row-class
    # passes (level 0 (16, 9, 8), level 1 (8, 5, 4) gathered); z slabs with odd nx and ny (level 0 (13, 11, 8), level 1
    # (7, 6, 4) gathered); x / y split with odd nz: on the chain, 4 + 3 planes (level 0 (16, 16, 7), level 1 (8, 8, 4) gathered)
    ("3d27-2x1x1-odd-ny", dict(n=(16, 9, 8), pgrid=(2, 1, 1), op="fe3", env=FRUN2, chain=0, odd=True)),
    ("3d27-1x1x2-odd-nx-ny", dict(n=(13, 11, 8), pgrid=(1, 1, 2), op="fe3", chain=0, odd=True)),
    ("3d27-2x2x1-chain-odd-nz", dict(n=(16, 16, 7), pgrid=(2, 2, 1), op="fe3", env=FRUN2, chain=1, odd=True)),
    ("3d7-2x1x1-odd-ny-nz", dict(n=(8, 9, 7), pgrid=(2, 1, 1), op="poisson3", chain=0, odd=True)),
    ("2d9-2x1-odd-ny-linexy", dict(n=(32, 17), pgrid=(2, 1), op="aniso9", relax="line-xy", odd=True)),
    ("2d5-1x2-point", dict(n=(32, 32), pgrid=(1, 2), op="poisson2")),
    ("2d9-2x2-point", dict(n=(32, 32), pgrid=(2, 2), op="varcoef9")),
    ("2d9-1x2-linexy", dict(n=(32, 32), pgrid=(1, 2), op="aniso9", relax="line-xy")),
    ("2d9-2x2-linexy", dict(n=(32, 32), pgrid=(2, 2), op="aniso9", relax="line-xy", nu=(2, 2))),
]


@pytest.mark.parametrize("name,c", PARITY, ids=[p[0] for p in PARITY])
def test_dist_pcg_equals_single_domain(name, c, tmp_path, capfd):
    """the decomposed PCG reproduces the single-domain PCG history and iterate on every rank grid shape, both drivers"""
    c = dict(c, runs=[MG])
    capfd.readouterr()
    _run(c, tmp_path)
    if c.get("odd"):  # no rank printed a library error (a refused launch among them)
        err = capfd.readouterr().err
        assert "refused" not in err and "[cedar_amd]" not in err, err
    if len(c["n"]) == 3:
        lv = np.load(tmp_path / "levels_r0.npy")
        if "chain" in c:
            assert (lv[1] > 0) == bool(c["chain"]), lv
        if "levels" in c:
            assert lv[0] >= c["levels"], lv
    _check_parity(c, tmp_path, 0)
    assert np.load(tmp_path / "hs0.npy")[-1] < 1e-10


MGRUNS = [dict(tol=1e-9, max_iter=30, stop="abs_l2"), dict(tol=1e-9, max_iter=30, stop="rel_l2"),
          dict(tol=1e-9, max_iter=30, stop="abs_m"), dict(tol=1e-9, max_iter=30, stop="rel_m"),
          dict(tol=1e-9, max_iter=30, nmg_cycles=2)]
# Plain and Jacobi CG on the 2D case run at most 30 iterations: over a longer run CG amplifies the rounding of the
# re-associated sums (2x2 ranks, varcoef9, plain CG to 1e-6: equal count, 82 iterations, the last 31 history entries off
# by up to 7.5e-2 relative), so the comparison stops where the criterion still means "same iteration"
SETTINGS = [("3d27-1x1x2", dict(n=(8, 8, 8), pgrid=(1, 1, 2), op="fe3"),
             [dict(tol=1e-6, max_iter=200, precon="none"), dict(tol=1e-6, max_iter=200, precon="diag")]),
            ("2d9-2x2", dict(n=(16, 16), pgrid=(2, 2), op="varcoef9"),
             [dict(tol=1e-6, max_iter=30, precon="none"), dict(tol=1e-6, max_iter=30, precon="diag")])]


@pytest.mark.parametrize("name,c,plain", SETTINGS, ids=[p[0] for p in SETTINGS])
def test_dist_pcg_every_stop_test_and_preconditioner(name, c, plain, tmp_path):
    """the four stop tests, two cycles per preconditioning, plain and Jacobi CG: the single-domain histories"""
    c = dict(c, runs=MGRUNS + plain)
    _run(c, tmp_path)
    for i in range(len(c["runs"])):
        _check_parity(c, tmp_path, i)


def test_dist_pcg_same_bits_on_every_rank_and_run(tmp_path):
    """every rank returns the same history and count, and a second run repeats the first bit for bit"""
    c = dict(n=(8, 8, 16), pgrid=(2, 2, 1), op="fe3", runs=[MG, dict(tol=1e-6, max_iter=100, precon="diag")],
             repeat=True)
    _run(c, tmp_path, single=False)
    for i in range(2):
        h = np.load(tmp_path / f"h{i}_0_r0.npy")
        assert len(h) > 2
        for r in range(4):
            for rep in range(2):
                assert np.array_equal(np.load(tmp_path / f"h{i}_{rep}_r{r}.npy"), h), (i, r, rep)
                assert np.array_equal(np.load(tmp_path / f"x{i}_{rep}_r{r}.npy"), np.load(tmp_path / f"x{i}_0_r{r}.npy"))


SYM = [("3d27-2x1x2", dict(n=(8, 8, 8), pgrid=(2, 1, 2), op="fe3")),
       ("2d9-2x2-linexy", dict(n=(16, 16), pgrid=(2, 2), op="aniso9", relax="line-xy", nu=(2, 2)))]


@pytest.mark.parametrize("name,c", SYM, ids=[p[0] for p in SYM])
def test_dist_precondition_is_symmetric(name, c, tmp_path):
    """<M^-1 u, v> = <u, M^-1 v> for the distributed V(nu,nu) cycle, dots on the gathered arrays"""
    import pcg_statement as ps
    c = dict(c, sym=True)
    _run(c, tmp_path, single=False)
    _, _, _, g = _global_problem(c)
    inner = (slice(1, -1),) * len(c["n"])
    u, v = ps.random_field(g, 41)[inner], ps.random_field(g, 43)[inner]
    mu, mv = _gather(c, tmp_path, "Mu"), _gather(c, tmp_path, "Mv")
    lhs, rhs = float(np.sum(mu * v)), float(np.sum(u * mv))
    assert abs(lhs - rhs) <= 1e-12 * np.linalg.norm(mu) * np.linalg.norm(v), (lhs, rhs)
    assert float(np.sum(mu * u)) > 0


@pytest.mark.parametrize("c", [dict(n=(8, 8, 8), pgrid=(1, 1, 2), op="fe3", nu=(2, 1)),
                               dict(n=(16, 16), pgrid=(1, 2), op="varcoef9", nu=(2, 1))], ids=["3d", "2d"])
def test_dist_pcg_refusal_is_collective(c, tmp_path):
    """V(2,1) is not symmetric: every rank refuses (RuntimeError, x untouched) and no rank is left in a collective --
    the next call, with a setting the handle allows, runs on every rank"""
    c = dict(c, refuse=True)
    _run(c, tmp_path, single=False)
    for r in range(_world(c)):
        refused, untouched, ran = np.load(tmp_path / f"refuse_r{r}.npy")
        assert refused and untouched and ran, r


def test_dist_pcg_one_rank_over_rccl(tmp_path):
    """DistSolver3.pcg on a 1 x 1 x 1 grid over the library's RCCL communicator (NativeComm, the transport behind the bmg
    interface): the single-domain history.  With one rank the all-gather of the partial sums is a device copy, so this
    covers the rank-order combine on the device, not the RCCL collective; a one-GPU box cannot run more than one RCCL rank."""
    c = dict(n=(24, 20, 16), pgrid=(1, 1, 1), op="fe3", agg=8, rccl=True, runs=[MG])
    _run(c, tmp_path)
    _check_parity(c, tmp_path, 0)
