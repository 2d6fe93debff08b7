"""The caller's arrays of the handle API between poisoned guard bands (tests/guarded.py).

A resident solver owns its levels, but x, b, the histories and -- with share_operator=True, as every handle here is made --
the level-0 operator are the caller's.  Per handle kind and call, for both device placements (16-byte and 8-byte-only
aligned x, b and operator) and both poisons:

* x and the history have the bits of the same call on a fresh handle of that kind with plain DeviceArrays and a plain
  numpy history (the histories are host arrays: theirs sits in a host arena of its own);
* b and the shared operator keep their bits (include/cedar_amd.h names no handle call that writes either);
* every band holds its poison;
* a batch handle (max_rhs 3) is asked for 2 items: the third keeps its bits.

Every handle runs V(1,1) cycles (what cedar_amd_solver_pcg takes) and at most 3 iterations.  time_relax(x, b, 2) runs two
sweeps of the handle's own level-0 smoother on the caller's arrays: with line relaxation that is the transposed y-line
pipeline (transpose2 of the caller's b) on an 8-byte-aligned base.
"""
import ctypes as C

import numpy as np
import pytest

import guarded as gd
import problems as pb
import semidefinite_cases as sdc

pytestmark = pytest.mark.gpu

MAX_ITER = 3
V11 = dict(nrelax_pre=1, nrelax_post=1, max_iter=MAX_ITER)
SINGLE = ["vcycle", "solve", "pcg", "fcg", "precondition", "time_relax"]
# a batch handle still serves the single-vector entry points on item 0 (include/cedar_amd.h): vcycle and time_relax on the
# caller's batch arrays, whose other items must keep their bits
MANY = ["vcycle_many", "solve_many", "pcg_many", "fcg_many", "vcycle", "time_relax"]
# a semidefinite handle: pcg, fcg, fcg_periodic, their _many forms and precondition are refused by the header's contract
# (cedar_amd_solver_create_semidefinite), vcycle and solve run the semidefinite cycle, time_relax the level-0 smoother
SEMI = ["vcycle", "solve", "time_relax", "fcg_semidefinite"]
# a periodic batch handle: pcg_many and fcg_many are refused (ibc != 0), solve_many writes the caller's rel rows and iters
PERMANY = ["vcycle_many", "solve_many", "fcg_periodic_many", "vcycle", "time_relax"]

# name -> (operator builder, Solver keywords, calls)
KINDS = {
    "2d_9pt_point": (lambda: pb.varcoef9(33, 30), dict(V11), SINGLE),
    # line-xy: level 0 of at most 64 per direction (lines_small.hip); just above 64 with both extents even and both odd
    # (the transposed y lines); lines of 600 unknowns (the scan-ordered factors)
    "2d_linexy_40x33": (lambda: pb.aniso9(40, 33), dict(V11, relax="line-xy"), SINGLE),
    "2d_linexy_70x66": (lambda: pb.aniso9(70, 66), dict(V11, relax="line-xy"), SINGLE),
    "2d_linexy_71x67": (lambda: pb.aniso9(71, 67), dict(V11, relax="line-xy"), SINGLE),
    "2d_linexy_600x66": (lambda: pb.aniso9(600, 66), dict(V11, relax="line-xy"), SINGLE),
    "3d_27pt_point": (lambda: pb.fe3(12, 10, 9), dict(V11), SINGLE),
    "3d_7pt_point": (lambda: pb.poisson3(12, 10, 9), dict(V11), SINGLE),
    "3d_7pt_planexy": (lambda: pb.diag_diffusion3(10, 9, 8, 1.0, 1.0, 1e-3),
                       dict(V11, relax="plane-xy", plane=dict(relax="line-xy", nrelax_pre=1, nrelax_post=1)),
                       SINGLE),  # V(1,1) with plane sweeps 1/1: a symmetric cycle, which pcg takes
    "2d_periodic": (lambda: pb.periodic_random_op(16, 12, 5, (True, True), 5), dict(V11, ibc=3),
                    ["vcycle", "solve", "fcg_periodic", "time_relax"]),
    "3d_periodic": (lambda: pb.periodic_random_op3(8, 8, 8, 14, (1, 1, 1), 15), dict(V11, ibc=8),
                    ["vcycle", "solve", "fcg_periodic", "time_relax"]),
    "2d_batch": (lambda: pb.varcoef9(33, 30), dict(V11, max_rhs=3), MANY),
    "3d_batch": (lambda: pb.fe3(12, 10, 9), dict(V11, max_rhs=3), MANY),
    "2d_periodic_batch": (lambda: pb.periodic_random_op(16, 12, 5, (True, True), 5),
                          dict(V11, ibc=3, max_rhs=3, periodic_batch2d=True), PERMANY),
    "3d_periodic_batch": (lambda: pb.periodic_random_op3(8, 8, 8, 14, (1, 1, 1), 15),
                          dict(V11, ibc=8, max_rhs=3, periodic_batch=True), PERMANY),
    "2d_semidefinite": (lambda: sdc.wrapped_poisson2(32, 32), dict(V11, ibc=3, semidefinite=True), SEMI),
    # fully periodic in 3D: the wrap-around direction pass of fcg_semidefinite on the caller's arrays
    "3d_semidefinite": (lambda: pb.periodic_poisson3(16, 16, 16, (1, 1, 1)), dict(V11, ibc=8, semidefinite=True), SEMI),
    "3d_neumann_semidefinite": (lambda: pb.regime_op((13, 15, 19), 14, 5, p_zero=1), dict(V11, semidefinite=True), SEMI),
}
NRHS = 2


@pytest.fixture(scope="module")
def capi():
    from cedar_amd import capi
    assert capi.device_count() >= 1, "no GPU visible"
    return capi


def run_call(capi, s, call, x, b, hist):
    """the call on the handle s; x, b: DeviceArrays (batch calls: views of the first NRHS items); hist: a numpy array of
    (MAX_ITER + 1,) or (NRHS, MAX_ITER + 1) doubles the library writes into.  Returns what the call returned"""
    lib = capi.lib
    ps = capi.PcgSettings(MAX_ITER, 1e-30, capi.PCG_STOP["rel_l2"], capi.PCG_PRECON["mg"], 1)
    iters = np.zeros(NRHS, dtype=np.int32)
    ip = iters.ctypes.data_as(C.POINTER(C.c_int))
    if call == "vcycle":
        lib.cedar_amd_solver_vcycle(s.h, x.ptr, b.ptr)
        return None
    if call == "precondition":
        lib.cedar_amd_solver_precondition(s.h, x.ptr, b.ptr)
        return None
    if call == "time_relax":
        assert s.time_relax(x, b, 2) >= 0.0
        return None
    if call == "solve":
        return lib.cedar_amd_solver_solve(s.h, b.ptr, x.ptr, hist.ctypes.data)
    if call in ("pcg", "fcg", "fcg_periodic", "fcg_semidefinite"):
        return getattr(lib, "cedar_amd_solver_" + call)(s.h, b.ptr, x.ptr, C.byref(ps), hist.ctypes.data)
    if call == "vcycle_many":
        return lib.cedar_amd_solver_vcycle_many(s.h, NRHS, x.ptr, b.ptr)
    if call == "solve_many":
        return (lib.cedar_amd_solver_solve_many(s.h, NRHS, b.ptr, x.ptr, hist.ctypes.data, ip), iters.tolist())
    assert call in ("pcg_many", "fcg_many", "fcg_periodic_many"), call
    return (getattr(lib, "cedar_amd_solver_" + call)(s.h, NRHS, b.ptr, x.ptr, C.byref(ps), hist.ctypes.data, ip), iters.tolist())


def hist_shape(call):
    return (NRHS, MAX_ITER + 1) if call.endswith("_many") else (MAX_ITER + 1,)


_PLAIN = {}


def inputs(kind):
    mk, kw, _ = KINDS[kind]
    so = mk()
    g = so.shape[1:]
    items = 3 if kw.get("max_rhs", 1) > 1 else None
    shp = g if items is None else (items,) + g
    m = pb.interior_mask(g)
    x, b = pb.uniform(shp, 7, -1, 1) * m, pb.uniform(shp, 8, -1, 1) * m
    if kw.get("semidefinite"):  # cedar_amd_solver_solve wants a compatible b there: zero sum over the interior
        b -= m * (b.sum() / m.sum())
    return so, x, b


def plain(capi, kind, call):
    """(x, hist, return value) of the call on a fresh handle with plain DeviceArrays: computed once, never modified"""
    if (kind, call) not in _PLAIN:
        _, kw, _ = KINDS[kind]
        so, x0, b0 = inputs(kind)
        so_d, x, b = (capi.DeviceArray.from_numpy(a) for a in (so, x0, b0))
        s = capi.Solver(so_d, share_operator=True, **kw)
        View = gd.device_view
        many = call.endswith("_many")
        hist = np.full(hist_shape(call), 7.0)
        try:
            rc = run_call(capi, s, call, View(x.ptr, (NRHS,) + x.shape[1:]) if many else x,
                          View(b.ptr, (NRHS,) + b.shape[1:]) if many else b, hist)
            capi.sync()
            assert rc is None or (rc[0] if isinstance(rc, tuple) else rc) >= 0, f"{kind}: {call} is refused on plain arrays"
            assert gd.same_bits(b.numpy(), b0) and gd.same_bits(so_d.numpy(), so)
            assert not gd.same_bits(x.numpy(), x0), f"{kind}: {call} left x as it was"
            _PLAIN[kind, call] = (x.numpy(), hist, rc)
        finally:
            s.close()
            for a in (so_d, x, b):
                a.free()
    return _PLAIN[kind, call]


@pytest.mark.parametrize("poison", sorted(gd.POISONS))
@pytest.mark.parametrize("placement", ["dev16", "dev8"])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_handle_calls_between_guard_bands(capi, kind, placement, poison):
    _, kw, calls = KINDS[kind]
    so, x0, b0 = inputs(kind)
    nd = so.ndim - 1
    batch = kw.get("max_rhs", 1) > 1
    bad = []
    for call in calls:
        want_x, want_hist, want_rc = plain(capi, kind, call)
        ar = gd.Arena([("so", so.shape), ("x", x0.shape), ("b", b0.shape)], gd.POISONS[poison], placement, nd)
        har = gd.Arena([("hist", hist_shape(call))], gd.POISONS[poison], "host", 2)
        s = None
        try:
            ar.fill("so", so), ar.fill("x", x0), ar.fill("b", b0)
            har.fill("hist", np.full(hist_shape(call), 7.0))
            s = capi.Solver(ar["so"], share_operator=True, **kw)
            many = call.endswith("_many")
            View = gd.device_view
            x = View(ar["x"].ptr, (NRHS,) + x0.shape[1:]) if many else ar["x"]
            b = View(ar["b"].ptr, (NRHS,) + b0.shape[1:]) if many else ar["b"]
            rc = run_call(capi, s, call, x, b, har["hist"])
            capi.sync()
            for a in (ar, har):
                try:
                    a.check()
                except AssertionError as e:
                    bad.append(f"{call}: {e}")
            got = ar.array("x")
            if not gd.same_bits(got, want_x):
                d = np.flatnonzero(gd.bits(got).ravel() != gd.bits(want_x).ravel())
                bad.append(f"{call}: x differs from the plain call at {d.size} of {got.size} elements, first at "
                           f"{np.unravel_index(int(d[0]), got.shape)}: {got.ravel()[d[0]]!r} for {want_x.ravel()[d[0]]!r}")
            if batch:  # a _many call works on NRHS items, a single-vector call on item 0
                used = NRHS if many else 1
                if not gd.same_bits(got[used:], x0[used:]):
                    bad.append(f"{call}: an item of x beyond the first {used} lost its bits")
            if not gd.same_bits(har.array("hist"), want_hist):
                bad.append(f"{call}: history {har.array('hist').tolist()} for {want_hist.tolist()}")
            if not gd.same_bits(ar.array("b"), b0):
                bad.append(f"{call}: b was written")
            if not gd.same_bits(ar.array("so"), so):
                bad.append(f"{call}: the shared operator was written")
            if rc != want_rc:
                bad.append(f"{call}: returned {rc!r}, the plain call {want_rc!r}")
        finally:
            if s is not None:
                s.close()
            ar.close()
            har.close()
    assert not bad, f"{kind} {placement} {poison}: {len(bad)} failures:\n" + "\n".join(bad)
