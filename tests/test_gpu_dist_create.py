"""What cedar_amd_dist3_create / cedar_amd_dist2_create refuse, and the level counts they plan -- in one process, no rank
subprocesses.  World sizes above 1 take the loop-back transport (cedar_amd_transport_loopback): every refusal comes before
the first message, and the level count depends on the extents alone.  Each refusal: the Python class raises (create
returned NULL), the library printed its reason, and a one-rank solve in the same process still reproduces its history
(the level-1 refusal is the one path that destroys a half-built handle)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _op(n):
    """a gallery operator on the local extents n = (nx, ny[, nz]) with its example right-hand side, in HBM"""
    from cedar_amd import capi
    return capi.gallery("fe3" if len(n) == 3 else "fe2", n)


def _solve(n):
    """history of a one-rank solve of the distributed driver on the gallery problem of extents n"""
    from cedar_amd import capi
    from cedar_amd.dist3 import DistSolver2, DistSolver3
    A, b = _op(n)
    x = capi.DeviceArray(b.shape)
    x.zero()
    s = (DistSolver3 if len(n) == 3 else DistSolver2)(None, 0, 1, A, max_iter=4, agglomerate_below=4)
    h = s.solve(b, x)
    s.close()
    return h


N3, N2 = (12, 10, 9), (20, 13)


@pytest.fixture(scope="module")
def history():
    """the histories every refusal test finds again afterwards; computed before the first refusal"""
    from cedar_amd import capi
    capi.set_device(0)
    h = {3: _solve(N3), 2: _solve(N2)}
    for v in h.values():
        assert len(v) >= 2 and all(np.isfinite(v)) and v[-1] < v[1] < 1  # a solve that converges
    return h


def _refused(capfd, fragment, make):
    capfd.readouterr()
    with pytest.raises(RuntimeError):
        make()
    err = capfd.readouterr().err
    assert fragment in err, err
    return err


def _still_solves(history, nd):
    assert _solve(N3 if nd == 3 else N2) == history[nd]


def _array(shape):
    from cedar_amd import capi
    a = capi.DeviceArray(shape)
    a.zero()
    return a


def test_dist3_create_refuses_bad_arguments(capfd, history):
    from cedar_amd.dist3 import DistSolver3
    A, _ = _op((8, 8, 8))
    bad = _array((5, 10, 10, 10))  # neither 4 nor 14 stencil planes
    _refused(capfd, "must be a device array of a", lambda: DistSolver3(None, 0, 1, bad))
    _refused(capfd, "must be a device array of a", lambda: DistSolver3(None, 1, 1, A))  # rank == world
    _refused(capfd, "needs a communicator", lambda: DistSolver3(None, 0, 2, A))
    _refused(capfd, "does not multiply to the world size", lambda: DistSolver3("loopback", 0, 2, A, pgrid=(1, 1, 1)))
    _still_solves(history, 3)


def test_dist2_create_refuses_bad_arguments(capfd, history):
    from cedar_amd.dist3 import DistSolver2
    A, _ = _op((8, 8))
    bad = _array((4, 10, 10))  # neither 3 nor 5 stencil planes
    _refused(capfd, "must be a device array of a", lambda: DistSolver2(None, 0, 1, bad))
    _refused(capfd, "must be a device array of a", lambda: DistSolver2(None, 1, 1, A))  # rank == world
    _refused(capfd, "needs a communicator", lambda: DistSolver2(None, 0, 2, A))
    _refused(capfd, "must multiply to the world size", lambda: DistSolver2("loopback", 0, 2, A, pgrid=(1, 1)))
    err = _refused(capfd, "must multiply to the world size", lambda: DistSolver2("loopback", 0, 16, A, pgrid=(16, 1)))
    assert "at most 8 ranks per direction" in err
    _refused(capfd, "relaxation must be", lambda: DistSolver2(None, 0, 1, A, relax="plane-xy"))
    _still_solves(history, 2)


# Odd local extent along a split direction, worked out from create's level loop with min_coarse = 3:
#   level 0: (9, 8[, 8]) on (2, 1[, 1]): global (18, 8[, 8]) has two levels, la = 1, and level 0 < la has extent 9 along x.
#   level 1: (18, 16[, 16]) on (2, 1[, 1]) with agglomerate_below = 2: global (36, 16[, 16]) has three levels (coarsest
#            extents 9, 4 then 5, 2 < 3), the smallest local extents 8 and 4 stay above 2, so la = 2; level 0 (18, ..) is even,
#            level 1 (9, 8[, 8]) is odd along x: refused with level 0 already allocated, the handle is destroyed half built.
@pytest.mark.parametrize("n,pgrid,agg,level", [((9, 8, 8), (2, 1, 1), 64, 0), ((18, 16, 16), (2, 1, 1), 2, 1),
                                               ((9, 8), (2, 1), 64, 0), ((18, 16), (2, 1), 2, 1)],
                         ids=["3d-level0", "3d-level1", "2d-level0", "2d-level1"])
def test_create_refuses_odd_extent_along_a_split_direction(n, pgrid, agg, level, capfd, history):
    from cedar_amd.dist3 import DistSolver2, DistSolver3
    cls = DistSolver3 if len(n) == 3 else DistSolver2
    A, _ = _op(n)
    err = _refused(capfd, f"level {level}: local extent 9",
                   lambda: cls("loopback", 0, 2, A, pgrid=pgrid, agglomerate_below=agg))
    assert f"cedar_amd_dist{len(n)}_create" in err
    _still_solves(history, len(n))


def _distributed_levels(n, pgrid, nlev, agg=64):
    """create's agglomeration rule: levels 0 .. la are distributed, la the first level (at least 1) whose smallest local
    extent is at most agg, or the coarsest; n / 2 along a split direction, (n - 1) / 2 + 1 along an unsplit one"""
    la, m = nlev - 1, list(n)
    for l in range(1, nlev):
        m = [(v - 1) // 2 + 1 if p == 1 else v // 2 for v, p in zip(m, pgrid)]
        if min(m) <= agg:
            la = l
            break
    return (max(la, 1) if nlev > 1 else 0) + 1


@pytest.mark.parametrize("n,pgrid", [((8, 8, 8), (2, 2, 1)), ((20, 16, 8), (1, 1, 4)), ((9, 8, 8), (1, 2, 1)),
                                     ((16, 12), (2, 1)), ((33, 16), (1, 2))],
                         ids=lambda v: "x".join(map(str, v)))
def test_global_level_count_equals_the_serial_solver(n, pgrid):
    """nlev_global of a loop-back handle = the level count of the serial solver on the global extents (extents only: any
    operator of the right stencil does); in 3D also the number of distributed levels the agglomeration rule gives"""
    from cedar_amd import capi, dist3
    capi.set_device(0)
    nd = len(n)
    world = int(np.prod(pgrid))
    A, _ = _op(n)
    s = (dist3.DistSolver3 if nd == 3 else dist3.DistSolver2)("loopback", 0, world, A, pgrid=pgrid)
    G, _ = _op(tuple(v * p for v, p in zip(n, pgrid)))
    serial = capi.Solver(G)
    want = serial.nlevels()
    serial.close()
    assert want >= 2
    assert s.nlev_global == want
    if nd == 3:
        assert dist3.lib.cedar_amd_dist3_distributed_levels(s.h) == _distributed_levels(n, pgrid, want)
    s.close()
