#!/usr/bin/env python3
"""What several right-hand sides at once cost on a periodic 3D handle (cedar_amd_solver_create_many_periodic).

    python tools/periodic_many_time.py [--n3 256] [--reps 5] [--out profiles/periodic_many_time.json]

Workloads: those of tools/fcg_periodic_time.py in 3D -- periodic Poisson that is Dirichlet in one direction, so the
operator is definite; device-resident vectors, b random, x0 = 0, V(2,1), point relaxation.
  3d7    seven-point, n3^3, ibc 3 (periodic in x and y)
  3d27   27-point, n3^3, ibc 5 (periodic in z): gallery::fe with the couplings across the periodic seam
Per workload, one handle with max_rhs = 8, everything in one process:
  (a) ms per batched cycle for 2 / 4 / 8 items (cedar_amd_solver_time_vcycles_many, device events) against the
      single-vector cycle of the same handle (cedar_amd_solver_time_vcycles on item 0), alternating; the figure quoted is
      batched ms / (items * single ms): the per-item time as a fraction of the single-vector cycle;
  (b) ms per fcg_periodic_many iteration for 4 items -- a run of N2 = 9 and one of N1 = 3 iterations (tol = 0), host clock
      around calls that end in a device synchronise, difference / (N2 - N1) -- against ms per fcg_periodic iteration on a
      plain periodic handle, alternating;
  (c) wall-clock ms to rel 1e-10 of fcg_periodic_many on four right-hand sides against four fcg_periodic calls.
Every repetition is kept in the output.  Nothing here is a pass criterion.
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
from fcg_periodic_time import fe3_periodic_z, timed  # noqa: E402

MAX_RHS = 8


def workloads(n3):
    return [("3d7", lambda: pb.periodic_poisson3(n3, n3, n3, (1, 1, 0)), 3), ("3d27", lambda: fe3_periodic_z(n3), 5)]


def measure(capi, name, so, ibc, reps, n1, n2, ncyc):
    g = so.shape[1:]
    mask = pb.interior_mask(g)
    b = capi.DeviceArray.from_numpy(np.stack([pb.uniform(g, 17 + m, -1, 1) * mask for m in range(MAX_RHS)]))
    x = capi.DeviceArray((MAX_RHS,) + g)
    so_d = capi.DeviceArray.from_numpy(so)
    res = {"workload": name, "shape": list(g[::-1]), "nstencil": so.shape[0], "ibc": ibc, "cycle": "V(2,1)", "max_rhs": MAX_RHS}
    st = dict(nrelax_pre=2, nrelax_post=1, ibc=ibc, max_iter=100, tol=1e-10, share_operator=True)
    sm = capi.Solver(so_d, max_rhs=MAX_RHS, periodic_batch=True, **st)
    s1 = capi.Solver(so_d, **st)
    lib = capi.lib

    npts = int(np.prod(g))

    def settings(max_iter, tol):
        return capi.PcgSettings(int(max_iter), float(tol), capi.PCG_STOP["rel_l2"], capi.PCG_PRECON["mg"], 1)

    try:
        # (a) the cycle
        cyc = {"ms_single_cycle": [], "cycles_timed": ncyc}
        for n in (2, 4, 8):
            cyc[f"ms_cycle_{n}"] = []
        x.zero()
        lib.cedar_amd_solver_time_vcycles(sm.h, x.ptr, b.ptr, 2)
        for n in (2, 4, 8):
            lib.cedar_amd_solver_time_vcycles_many(sm.h, n, x.ptr, b.ptr, 2)
        for _ in range(reps):
            x.zero()
            cyc["ms_single_cycle"].append(lib.cedar_amd_solver_time_vcycles(sm.h, x.ptr, b.ptr, ncyc) / ncyc)
            for n in (2, 4, 8):
                x.zero()
                cyc[f"ms_cycle_{n}"].append(lib.cedar_amd_solver_time_vcycles_many(sm.h, n, x.ptr, b.ptr, ncyc) / ncyc)
        one = statistics.median(cyc["ms_single_cycle"])
        for n in (2, 4, 8):
            cyc[f"per_item_fraction_{n}"] = statistics.median(cyc[f"ms_cycle_{n}"]) / (n * one)
        res["cycle"] = cyc

        # (b), (c) flexible CG: four items against four single calls
        def many(max_iter, tol):  # the first four items of b, x
            x.zero()
            ps, hist, iters = settings(max_iter, tol), np.zeros((4, max_iter + 1)), np.zeros(4, dtype=np.int32)

            def call():
                n = lib.cedar_amd_solver_fcg_periodic_many(sm.h, 4, b.ptr, x.ptr, C.byref(ps), hist.ctypes.data,
                                                           iters.ctypes.data_as(C.POINTER(C.c_int)))
                assert n >= 0
                return [hist[m, : iters[m] + 1] for m in range(4)], [int(v) for v in iters]
            return timed(capi, call)

        def single(m, max_iter, tol):  # item m of b, x on the plain handle
            ps, hist = settings(max_iter, tol), np.zeros(max_iter + 1)

            def call():
                n = lib.cedar_amd_solver_fcg_periodic(s1.h, b.ptr + m * npts * 8, x.ptr + m * npts * 8, C.byref(ps), hist.ctypes.data)
                assert n >= 0
                return hist[: n + 1]
            return timed(capi, call)

        many(2, 0.0)  # warm-up: records the graphs, allocates the Krylov vectors
        x.zero()
        single(0, 2, 0.0)
        it_many, it_one = [], []
        for _ in range(reps):
            t1, _ = many(n1, 0.0)
            t2, _ = many(n2, 0.0)
            it_many.append((t2 - t1) / (n2 - n1))
            x.zero()
            t1, _ = single(0, n1, 0.0)
            x.zero()
            t2, _ = single(0, n2, 0.0)
            it_one.append((t2 - t1) / (n2 - n1))
        res["per_iteration"] = {"ms_fcg_periodic_many_iteration_4_items": it_many, "ms_fcg_periodic_iteration": it_one, "n1": n1,
                                "n2": n2, "per_item_fraction_4": statistics.median(it_many) / (4 * statistics.median(it_one))}
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
    ap.add_argument("--n3", type=int, default=256)
    ap.add_argument("--n1-iters", type=int, default=3)
    ap.add_argument("--n2-iters", type=int, default=9)
    ap.add_argument("--cycles", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, help="3d7 or 3d27")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from cedar_amd import capi
    if capi.device_count() < 1:
        raise SystemExit("periodic_many_time: no GPU visible (there is no CPU fallback)")
    out = {"reps": a.reps, "workloads": []}
    for name, mk, ibc in workloads(a.n3):
        if a.only and a.only != name:
            continue
        out["workloads"].append(measure(capi, name, mk(), ibc, a.reps, a.n1_iters, a.n2_iters, a.cycles))
        print(json.dumps(out["workloads"][-1]), flush=True)
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
