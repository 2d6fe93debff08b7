"""GPU multi-rank tests runnable on the one-GPU box.  No torch in any rank process.
* 2 / 4 ranks share device 0 and talk through the host-staged rehearsal transport (cedar_amd/comm.py SocketComm: RCCL
  refuses two ranks on one device); HIP kernels through the C ABI.  Same criterion as tests/test_dist_cpu.py: the
  decomposed run reproduces the single-domain history (the reference's test/3d/mpi/test_relax.cc:56-59).
* the RCCL transport itself (NativeComm -> cedar_amd_comm_* -> librccl) with the one rank a one-GPU box allows: a
  grouped self send/recv, all-reduce, all-gather, and a whole DistSolver3 solve on a 1x1x1 rank grid."""
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


def _problem(pb, kind, gn):
    """(operator, right-hand side) on the global grid gn = (nx, ny, nz): "rand27" a random 27-point operator, "poisson7" the
    7-point Laplacian (nstencil = 4) -- the generators of tests/test_dist_cpu.py (which cannot be imported here: it brings torch)"""
    g = (gn[2] + 2, gn[1] + 2, gn[0] + 2)
    if kind == "rand27":
        return pb.random_op(g, 14, 77), pb.uniform(g, 78, -1, 1) * pb.interior_mask(g)
    if kind == "poisson7":
        return pb.poisson3(*gn), pb.rhs3(*gn)
    raise ValueError(kind)


def _worker(rank, world, port, n, pgrid, outdir, overlap_min, driver="python", agg=64, maxit=5, kind="rand27"):
    for p in (HERE, ROOT, os.path.join(ROOT, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["RANK"], os.environ["WORLD_SIZE"] = str(rank), str(world)
    import faulthandler
    faulthandler.dump_traceback_later(int(os.environ.get("CEDAR_AMD_TEST_STUCK_S", "600")), exit=True)  # a stuck rank says where
    import problems as pb
    from cedar_amd import capi
    from cedar_amd.comm import SocketComm
    from cedar_amd.dist import DistSolver3, GpuBackend, Topology
    assert "torch" not in sys.modules
    capi.set_device(0)
    comm = SocketComm(rank, world)
    try:
        be = GpuBackend(comm, 0)
        topo = Topology(rank, world, pgrid)
        gn = tuple(n[d] * topo.p[d] for d in range(3))
        gso, gb = _problem(pb, kind, gn)
        ci, cj, ck = topo.coord
        sl = (slice(ck * n[2], ck * n[2] + n[2] + 2), slice(cj * n[1], cj * n[1] + n[1] + 2),
              slice(ci * n[0], ci * n[0] + n[0] + 2))
        m = pb.interior_mask(tuple(s.stop - s.start for s in sl)).astype(np.float64)
        A = be.from_numpy(np.ascontiguousarray(gso[(slice(None),) + sl]) * m)
        b = be.from_numpy(np.ascontiguousarray(gb[sl]) * m)
        x = be.zeros(b.shape)
        if driver == "native":  # the orchestration below the C ABI (cedar_amd/csrc/dist3.cpp); Python hands over arrays + transport
            from cedar_amd.dist3 import DistSolver3 as Native
            s = Native(comm, rank, world, A, pgrid=pgrid, max_iter=maxit, overlap_min=overlap_min, agglomerate_below=agg)
            assert s.coord == topo.coord
            if rank == 0:
                open(os.path.join(outdir, "chain_levels.txt"), "w").write(str(s.chain_levels))
        else:
            s = DistSolver3(be, topo, A, max_iter=5, overlap_min=overlap_min)
        h = s.solve(b, x)
        np.save(os.path.join(outdir, f"x{rank}.npy"), x.numpy())
        if rank == 0:
            np.save(os.path.join(outdir, "hist.npy"), np.array(h))
    finally:
        comm.close()


def _spawn(target, world, args):
    ctx = mp.get_context("spawn")
    ps = [ctx.Process(target=target, args=(r, world) + args) for r in range(world)]
    for p in ps:
        p.start()
    for p in ps:
        p.join(900)
    bad = [p.exitcode for p in ps if p.exitcode != 0]
    for p in ps:
        if p.is_alive():
            p.kill()
    assert not bad, f"rank processes failed: exit codes {bad}"


CASES = [((16, 12, 10), (2, 1, 1), 96), ((8, 8, 8), (2, 2, 1), 96),
         ((12, 10, 16), (1, 1, 2), 4), ((8, 8, 8), (1, 2, 2), 4),
         ((8, 8, 8), (2, 2, 1), 4), ((64, 64, 64), (1, 1, 2), 16), ((20, 16, 8), (1, 1, 4), 4),
         # 320 rows: the slab path runs the plane-fused kernel on level 0
         ((12, 320, 8), (1, 1, 2), 4),
         # 6.5e6 unknowns: plane-fused level 0 under a halo in flight, three
         # distributed levels, gathered 16x80x80 coarse problem
         ((64, 320, 160), (1, 1, 2), 32)]
IDS = ["2ranks-x", "4ranks-xy", "2ranks-z-overlap", "4ranks-yz-overlap", "4ranks-xy-overlap",
       "2ranks-z-64cubed-overlap", "4ranks-z-slabs-overlap", "2ranks-z-plane-fused", "2ranks-z-6M-unknowns"]


def _check_against_single_domain(n, pgrid, tmp_path, oracle, maxit=5, kind="rand27"):
    import problems as pb
    world = pgrid[0] * pgrid[1] * pgrid[2]
    gn = tuple(n[d] * pgrid[d] for d in range(3))
    gso, gb = _problem(pb, kind, gn)
    ml = oracle.ml_create(gso)
    x = np.zeros_like(gb)
    want = ml.solve(gb, x, maxiter=maxit)
    ml.close()
    got = np.load(tmp_path / "hist.npy")
    assert len(got) == len(want)
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-14)
    px, py, pz = pgrid
    for r in range(world):
        ci, cj, ck = r % px, (r // px) % py, r // (px * py)
        xr = np.load(tmp_path / f"x{r}.npy")
        ref = x[ck * n[2]:ck * n[2] + n[2] + 2, cj * n[1]:cj * n[1] + n[1] + 2, ci * n[0]:ci * n[0] + n[0] + 2]
        own = (slice(1, -1),) * 3
        assert np.max(np.abs(xr[own] - ref[own])) <= 1e-12 * np.max(np.abs(x))


@pytest.mark.parametrize("n,pgrid,overlap_min", CASES, ids=IDS)
def test_native_driver_ranks_sharing_one_gpu_equal_single_domain(n, pgrid, overlap_min, tmp_path, oracle):
    """cedar_amd_dist3_* (the distributed V-cycle below the C ABI, cedar_amd/csrc/dist3.cpp) on 2 and 4 ranks sharing
    the GPU over the host-staged transport handed in as the ABI's transport table: the single-domain history and
    solution, on every rank grid shape, with and without the overlapped y/z halo, slab and row-class sweeps"""
    world = pgrid[0] * pgrid[1] * pgrid[2]
    _spawn(_worker, world, (_free_port(), n, pgrid, str(tmp_path), overlap_min, "native"))
    _check_against_single_domain(n, pgrid, tmp_path, oracle)


# Rank grids with an x / y split where the levels take the partial-sum sweep (runs of 2 rows so that boxes of a few thousand
# points qualify): boundary-first chain + one masked launch per k-parity (dist3.cpp chain_parity).  Every role of a rank:
# neighbour on the low / high / both sides in x and in y, with and without a z split.
CHAIN_CASES = [((16, 32, 8), (2, 2, 1)), ((16, 16, 8), (3, 1, 1)), ((8, 24, 8), (1, 3, 1)), ((16, 16, 8), (2, 1, 2)),
               ((8, 16, 8), (1, 2, 2)), ((32, 32, 16), (2, 2, 1)), ((8, 16, 8), (2, 2, 1))]
CHAIN_IDS = ["4ranks-xy", "3ranks-x", "3ranks-y", "4ranks-xz", "4ranks-yz", "4ranks-xy-two-chain-levels", "4ranks-xy-8-columns"]


# the production run length (16 rows from 224 rows per box on) on a 2 x 2 x 1 grid
CHAIN_CASES.append(((16, 256, 32), (2, 2, 1)))  # (z deep enough for a four-level hierarchy: the coarsest level is solved directly)
CHAIN_IDS.append("4ranks-xy-default-run-length")


# 128 rows per rank: below the 160 rows from which a single GPU takes the partial-sum sweep, but on a rank grid with an x / y
# split the driver registers it from 128 rows on (runs of 8 rows)
CHAIN_CASES.append(((16, 128, 16), (2, 2, 1)))
CHAIN_IDS.append("4ranks-xy-128-rows-default-runs")
DEFAULT_RUNS = {(16, 256, 32), (16, 128, 16)}
# (a 3 x 2 x 1 grid -- a rank with neighbours on both sides in x AND one in y -- runs on the CPU statement of the chain,
# tests/test_dist_cpu.py: six rank processes plus this one would exceed the six a one-GPU box lets share its card)
# rows of 512 points per rank: the 256-lane kernels of the production size (masks on lanes 254 / 255, dense column copy of a
# 514-point row), two chain levels; the gathered coarsest level has 4096 unknowns in a band of 1024
CHAIN_CASES.append(((512, 16, 16), (2, 1, 1)))
CHAIN_IDS.append("2ranks-x-512-point-rows")


@pytest.mark.parametrize("n,pgrid", CHAIN_CASES, ids=CHAIN_IDS)
def test_native_driver_boundary_first_chain_equals_single_domain(n, pgrid, tmp_path, oracle, monkeypatch):
    """the partial-sum sweep on rank grids with an x / y split: columns and rows next to a neighbouring rank relaxed ahead,
    stage by stage, the rest of a k-parity in one masked launch -- the single-domain history and solution"""
    if n not in DEFAULT_RUNS:
        monkeypatch.setenv("CEDAR_AMD_FRUN", "2")
    world = pgrid[0] * pgrid[1] * pgrid[2]
    # agglomerate_below = 4: (32, 32, 16) keeps levels 0 and 1 distributed (level 2, 8 x 8 x 4 per rank, is gathered), both on
    # the chain
    deep = {(32, 32, 16): 2, (512, 16, 16): 2}.get(n)
    maxit = 5
    _spawn(_worker, world, (_free_port(), n, pgrid, str(tmp_path), 96, "native", 4 if deep else 64, maxit))
    assert int(open(tmp_path / "chain_levels.txt").read()) == (deep or 1)
    _check_against_single_domain(n, pgrid, tmp_path, oracle, maxit)


# Odd extents along UNSPLIT directions.  create insists on even extents only along split directions (on every distributed
# level below the gathered one); an unsplit direction may be odd on level 0 or turn odd further down (18 -> 9).  Coarsening
# per level: n / 2 along a split direction, (n - 1) / 2 + 1 along an unsplit one.  One case per sweep path of smooth()
# (dist3.cpp), each with the number of chain levels it must report: the masked launch of the chain takes even nx and ny
# only (cedar_amd_relax3_masked_ok), so a level with an odd unsplit nx or ny must stay on the reference-order row-class
# passes -- chain_levels 0 -- while an odd nz does not keep a level off the chain.
#   (id, n, rank grid, overlap_min, agglomerate_below, environment, operator, chain levels)
FRUN2 = {"CEDAR_AMD_FRUN": "2"}  # runs of 2 rows: the partial-sum sweep (hence the chain) from 8 rows on, as in CHAIN_CASES
NOCHAIN = {"CEDAR_AMD_DIST_CHAIN": "0"}
ODD_CASES = [
    # -- chain candidates: x / y split, both extents >= 8, partial-sum sweep on offer
    # level 0 (16, 9, 8), level 1 (8, 5, 4) gathered
    ("chain-x-odd-ny", (16, 9, 8), (2, 1, 1), 96, 64, FRUN2, "rand27", 0),
    # level 0 (16, 17, 8), level 1 (8, 9, 4) gathered
    ("chain-xz-odd-ny", (16, 17, 8), (2, 1, 2), 96, 64, FRUN2, "rand27", 0),
    # level 0 (9, 16, 8), level 1 (5, 8, 4) gathered
    ("chain-y-odd-nx", (9, 16, 8), (1, 2, 1), 96, 64, FRUN2, "rand27", 0),
    # the same box on three ranks: the middle one has a neighbour on both y sides
    ("chain-y3-odd-nx", (9, 16, 8), (1, 3, 1), 96, 64, FRUN2, "rand27", 0),
    # level 0 (32, 18, 16) even: stays on the chain; level 1 (16, 9, 8) odd: row-class; level 2 (8, 5, 4) gathered
    ("chain-x-odd-from-level-1", (32, 18, 16), (2, 1, 1), 96, 4, FRUN2, "rand27", 1),
    # default run lengths, 129 rows (the driver offers the partial-sum sweep from 128 rows on): level 0 (16, 129, 16),
    # level 1 (8, 65, 8) gathered
    ("chain-x-129-rows-default-runs", (16, 129, 16), (2, 1, 1), 96, 64, {}, "rand27", 0),
    # rows of 257 points (the 256-lane kernels, last lane half empty): level 0 (257, 16, 16), level 1 (129, 8, 8) gathered
    # (16 planes: the gathered hierarchy gets a second level and its direct solve a band of 520 instead of 2064)
    ("chain-y-257-point-rows", (257, 16, 16), (1, 2, 1), 96, 64, FRUN2, "rand27", 0),
    # odd nz with an x / y split: 4 planes of one k-parity, 3 of the other; nx and ny even, so the level takes the chain.
    # level 0 (16, 16, 7), level 1 (8, 8, 4) gathered
    ("chain-xy-odd-nz", (16, 16, 7), (2, 2, 1), 96, 64, FRUN2, "rand27", 1),
    # -- slab path (z split only), odd nx and ny
    # level 0 (13, 11, 8), level 1 (7, 6, 4) gathered
    ("slab-odd-nx-ny", (13, 11, 8), (1, 1, 2), 96, 64, {}, "rand27", 0),
    # 321 rows: plane-fused kernel and partial sums on level 0 (13, 321, 8); level 1 (7, 161, 4) gathered
    ("slab-321-rows-plane-fused", (13, 321, 8), (1, 1, 2), 96, 64, {}, "rand27", 0),
    # overlap_min = 4: shell planes / interior planes around the halo on the side stream; level 0 (11, 13, 8), level 1 (6, 7, 4)
    ("slab-odd-nx-ny-overlap", (11, 13, 8), (1, 1, 2), 4, 64, {}, "rand27", 0),
    # rows of 600 points (300 pairs: the 512-lane row kernels under cedar_amd_relax3_planes; cedar_amd_relax3_masked_ok
    # refuses more than 512 points, so no level may take the chain): level 0 (600, 16, 16), level 1 (300, 8, 8) gathered
    ("slab-600-point-rows", (600, 16, 16), (1, 1, 2), 96, 64, FRUN2, "rand27", 0),
    # -- row-class passes asked for outright
    # x split: relax3_fixup on the column next to the neighbour; level 0 (16, 9, 7), level 1 (8, 5, 4) gathered
    ("rowclass-x-odd-ny-nz", (16, 9, 7), (2, 1, 1), 96, 64, NOCHAIN, "rand27", 0),
    # x and z split, overlap_min = 4: interior rows under the y/z halo; level 0 (16, 9, 8), level 1 (8, 5, 4) gathered
    ("rowclass-xz-odd-ny-overlap", (16, 9, 8), (2, 1, 2), 4, 64, NOCHAIN, "rand27", 0),
    # -- 7-point operator on level 0 (two-colour sweep): level 0 (16, 9, 7), level 1 (8, 5, 4) gathered
    ("7pt-x-odd-ny-nz", (16, 9, 7), (2, 1, 1), 96, 64, {}, "poisson7", 0),
]


@pytest.mark.parametrize("name,n,pgrid,overlap_min,agg,env,kind,chain_levels", ODD_CASES, ids=[c[0] for c in ODD_CASES])
def test_native_driver_odd_unsplit_extents_equal_single_domain(name, n, pgrid, overlap_min, agg, env, kind, chain_levels,
                                                               tmp_path, oracle, monkeypatch, capfd):
    """cedar_amd_dist3_* on boxes with an odd extent along an unsplit direction, every sweep path of smooth(): the
    single-domain history and solution, to the tolerances of the even cases.  Each case also pins the path: the number of
    chain levels the driver reports, and a rank that printed a library error (a refused launch among them) fails the case
    even where the numbers agree."""
    for k in ("CEDAR_AMD_FRUN", "CEDAR_AMD_DIST_CHAIN"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for d in range(3):  # what create enforces on level 0; the comments above carry the levels below
        assert pgrid[d] == 1 or n[d] % 2 == 0
    world = pgrid[0] * pgrid[1] * pgrid[2]
    assert world <= 6
    capfd.readouterr()
    _spawn(_worker, world, (_free_port(), n, pgrid, str(tmp_path), overlap_min, "native", agg, 5, kind))
    err = capfd.readouterr().err
    assert "refused" not in err and "[cedar_amd]" not in err and "cedar_amd_dist3" not in err, err
    assert int(open(tmp_path / "chain_levels.txt").read()) == chain_levels
    _check_against_single_domain(n, pgrid, tmp_path, oracle, 5, kind)


# overlap_min = 4: the y/z halo of a row pass travels on a side HIP stream under the interior rows of
# the next pass wherever the level has an interior (the production default, 96, would leave these
# small grids on the in-order path, which the first two cases keep covering)
@pytest.mark.parametrize("n,pgrid,overlap_min", [CASES[0], CASES[3], CASES[4], CASES[7]], ids=[IDS[0], IDS[3], IDS[4], IDS[7]])
def test_two_ranks_one_gpu_equal_single_domain(n, pgrid, overlap_min, tmp_path, oracle):
    """the same orchestration in Python on the GPU backend (cedar_amd/dist.py: the statement of the algorithm that also
    runs on the CPU against the oracle, tests/test_dist_cpu.py)"""
    world = pgrid[0] * pgrid[1] * pgrid[2]
    _spawn(_worker, world, (_free_port(), n, pgrid, str(tmp_path), overlap_min))
    _check_against_single_domain(n, pgrid, tmp_path, oracle)


def _rccl_worker(rank, world, port, outdir):
    for p in (HERE, ROOT, os.path.join(ROOT, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["RANK"], os.environ["WORLD_SIZE"] = str(rank), str(world)
    import problems as pb
    from cedar_amd import capi
    from cedar_amd.comm import NativeComm, Stream
    from cedar_amd.dist import DistSolver3, GpuBackend, Topology
    assert "torch" not in sys.modules
    capi.set_device(0)
    comm = NativeComm(rank, world)
    out = {}
    # grouped self send/recv of two messages, on a side stream of the library
    a = capi.DeviceArray.from_numpy(np.arange(1000.0))
    r = capi.DeviceArray((1000,))
    st = Stream()
    main = capi.lib.cedar_amd_get_stream()
    capi.lib.cedar_amd_stream_wait(st.h, main)
    capi.lib.cedar_amd_set_stream(st.h)
    comm.p2p([(0, a, 0, 600), (0, a, 600, 400)], [(0, r, 0, 600), (0, r, 600, 400)])
    capi.lib.cedar_amd_set_stream(main)
    capi.lib.cedar_amd_stream_wait(main, st.h)
    capi.lib.cedar_amd_device_sync()
    out["p2p"] = bool(np.array_equal(r.numpy(), np.arange(1000.0)))
    out["sum"] = comm.allreduce_sum(3.5)
    g = capi.DeviceArray((1000,))
    comm.allgather(a, 1000, g)
    capi.sync()
    out["gather"] = bool(np.array_equal(g.numpy(), np.arange(1000.0)))
    # the whole distributed solver on a 1x1x1 rank grid over RCCL (all-gather of the coarse level, norm all-reduce)
    n = (24, 20, 16)
    g3 = (n[2] + 2, n[1] + 2, n[0] + 2)
    so = pb.random_op(g3, 14, 77)
    b = pb.uniform(g3, 78, -1, 1) * pb.interior_mask(g3)
    be = GpuBackend(comm, 0)
    s = DistSolver3(be, Topology(0, 1), be.from_numpy(so), max_iter=4, agglomerate_below=8)
    x = be.zeros(b.shape)
    out["hist"] = [float(v) for v in s.solve(be.from_numpy(b), x)]
    # and the native driver with the RCCL communicator handle (all-gather + all-reduce inside the library)
    from cedar_amd.dist3 import DistSolver3 as Native
    A2 = be.from_numpy(so)
    s2 = Native(comm, 0, 1, A2, max_iter=4, agglomerate_below=8)
    x2 = be.zeros(b.shape)
    out["hist_native"] = s2.solve(be.from_numpy(b), x2)
    s2.close()
    comm.close()
    import json
    json.dump(out, open(os.path.join(outdir, "rccl.json"), "w"))


def test_rccl_transport_one_rank(tmp_path, oracle):
    """ncclCommInitRank / grouped ncclSend+ncclRecv / ncclAllReduce / ncclAllGather through the library's C ABI"""
    import json
    import problems as pb
    _spawn(_rccl_worker, 1, (_free_port(), str(tmp_path)))
    out = json.load(open(tmp_path / "rccl.json"))
    assert out["p2p"] and out["gather"] and out["sum"] == 3.5
    n = (24, 20, 16)
    g3 = (n[2] + 2, n[1] + 2, n[0] + 2)
    so = pb.random_op(g3, 14, 77)
    b = pb.uniform(g3, 78, -1, 1) * pb.interior_mask(g3)
    ml = oracle.ml_create(so)
    x = np.zeros_like(b)
    want = ml.solve(b, x, maxiter=4)
    ml.close()
    np.testing.assert_allclose(out["hist"], want, rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(out["hist_native"], want, rtol=1e-10, atol=1e-14)
