#!/usr/bin/env python3
"""What several right-hand sides at once cost on a periodic 2D handle (cedar_amd_solver_create_many_periodic2).

    python tools/periodic_many2d_time.py [--n2 4096] [--reps 3] [--out profiles/periodic_many2d_time.json]

Workloads: the 2D one of tools/fcg_periodic_time.py -- the five-point periodic Poisson operator of
examples/ser-periodic-2d.cc, n2^2, ibc 2 (periodic in x, Dirichlet in y, so the operator is definite); device-resident
vectors, b random, x0 = 0, V(2,1):
  2d5_point    point relaxation
  2d5_linexy   the same operator under line-xy relaxation (cyclic x-lines batched through the launch grid, y-lines item
               by item)
Per workload, one handle with max_rhs = 8, everything in one process:
  (a) ms per batched cycle for 1 / 2 / 4 / 8 items (cedar_amd_solver_time_vcycles_many, device events) against the
      single-vector cycle of the same handle (cedar_amd_solver_time_vcycles on item 0), alternating; the figure quoted is
      batched ms / (items * single ms): the per-item time as a fraction of the single-vector cycle;
  (b) wall-clock ms to rel 1e-10 of fcg_periodic_many on four right-hand sides against four fcg_periodic calls on a plain
      periodic handle (host clock around calls that end in a device synchronise), alternating.
Every repetition is kept in the output.  The first error ends the run (an exception; nothing is retried).  Nothing here
is a pass criterion.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import problems as pb  # noqa: E402
from fcg_periodic_time import timed  # noqa: E402

MAX_RHS = 8
ITEMS = (1, 2, 4, 8)


def measure(capi, name, so, ibc, relax, reps, ncyc):
    g = so.shape[1:]
    mask = pb.interior_mask(g)
    b = capi.DeviceArray.from_numpy(np.stack([pb.uniform(g, 17 + m, -1, 1) * mask for m in range(MAX_RHS)]))
    x = capi.DeviceArray((MAX_RHS,) + g)
    so_d = capi.DeviceArray.from_numpy(so)
    res = {"workload": name, "shape": list(g[::-1]), "nstencil": so.shape[0], "ibc": ibc, "relax": relax, "max_rhs": MAX_RHS}
    st = dict(relax=relax, nrelax_pre=2, nrelax_post=1, ibc=ibc, max_iter=100, tol=1e-10, share_operator=True)
    sm = capi.Solver(so_d, max_rhs=MAX_RHS, periodic_batch2d=True, **st)
    s1 = capi.Solver(so_d, **st)
    lib = capi.lib
    npts = int(np.prod(g))

    def checked(ms):
        if not ms >= 0:
            raise RuntimeError(f"{name}: a timed call was refused")
        return ms

    try:
        # (a) the cycle
        cyc = {"ms_single_cycle": [], "cycles_timed": ncyc}
        for n in ITEMS:
            cyc[f"ms_cycle_{n}"] = []
        x.zero()
        checked(lib.cedar_amd_solver_time_vcycles(sm.h, x.ptr, b.ptr, 2))
        for n in ITEMS:
            checked(lib.cedar_amd_solver_time_vcycles_many(sm.h, n, x.ptr, b.ptr, 2))
        for _ in range(reps):
            x.zero()
            cyc["ms_single_cycle"].append(checked(lib.cedar_amd_solver_time_vcycles(sm.h, x.ptr, b.ptr, ncyc)) / ncyc)
            for n in ITEMS:
                x.zero()
                cyc[f"ms_cycle_{n}"].append(checked(lib.cedar_amd_solver_time_vcycles_many(sm.h, n, x.ptr, b.ptr, ncyc)) / ncyc)
        one = statistics.median(cyc["ms_single_cycle"])
        for n in ITEMS:
            cyc[f"per_item_fraction_{n}"] = statistics.median(cyc[f"ms_cycle_{n}"]) / (n * one)
        res["cycle"] = cyc

        # (b) flexible CG to 1e-10: four items against four single calls
        def many(max_iter, tol):
            x.zero()
            ps = capi.PcgSettings(int(max_iter), float(tol), capi.PCG_STOP["rel_l2"], capi.PCG_PRECON["mg"], 1)
            hist, iters = np.zeros((4, max_iter + 1)), np.zeros(4, dtype=np.int32)

            def call():
                n = lib.cedar_amd_solver_fcg_periodic_many(sm.h, 4, b.ptr, x.ptr, C.byref(ps), hist.ctypes.data,
                                                           iters.ctypes.data_as(C.POINTER(C.c_int)))
                if n < 0:
                    raise RuntimeError(f"{name}: fcg_periodic_many was refused")
                return [hist[m, : iters[m] + 1] for m in range(4)], [int(v) for v in iters]
            return timed(capi, call)

        def single(m, max_iter, tol):
            ps = capi.PcgSettings(int(max_iter), float(tol), capi.PCG_STOP["rel_l2"], capi.PCG_PRECON["mg"], 1)
            hist = np.zeros(max_iter + 1)

            def call():
                n = lib.cedar_amd_solver_fcg_periodic(s1.h, b.ptr + m * npts * 8, x.ptr + m * npts * 8, C.byref(ps), hist.ctypes.data)
                if n < 0:
                    raise RuntimeError(f"{name}: fcg_periodic was refused")
                return hist[: n + 1]
            return timed(capi, call)

        many(2, 0.0)  # warm-up: records the graphs, allocates the Krylov vectors
        x.zero()
        single(0, 2, 0.0)
        runs_m, runs_s = [], []
        for _ in range(reps):
            t, (h, it) = many(60, 1e-10)
            runs_m.append({"ms": t, "iterations": it, "rel": [float(r[-1]) for r in h]})
            x.zero()
            tt, its = 0.0, []
            for m in range(4):
                t, h = single(m, 60, 1e-10)
                tt += t
                its.append(len(h) - 1)
            runs_s.append({"ms": tt, "iterations": its})
        res["to_rel_1e-10_four_rhs"] = {"fcg_periodic_many": runs_m, "four_fcg_periodic_calls": runs_s,
                                        "median_ratio_many_over_four_singles": statistics.median(r["ms"] for r in runs_m)
                                        / statistics.median(r["ms"] for r in runs_s)}
    finally:
        sm.close()
        s1.close()
    for a in (b, x, so_d):
        a.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n2", type=int, default=4096)
    ap.add_argument("--cycles", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default=None, help="2d5_point or 2d5_linexy")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from cedar_amd import capi
    if capi.device_count() < 1:
        raise SystemExit("periodic_many2d_time: no GPU visible (there is no CPU fallback)")
    out = {"reps": a.reps, "workloads": []}
    for name, relax in (("2d5_point", "point"), ("2d5_linexy", "line-xy")):
        if a.only and a.only != name:
            continue
        so = pb.periodic_poisson2(a.n2, a.n2, (True, False))
        out["workloads"].append(measure(capi, name, so, 2, relax, a.reps, a.cycles))
        print(json.dumps(out["workloads"][-1]), flush=True)
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
