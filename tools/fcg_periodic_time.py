#!/usr/bin/env python3
"""What flexible CG on a periodic handle (cedar_amd_solver_fcg_periodic) costs and what it buys.

    python tools/fcg_periodic_time.py [--n3 256] [--n2 4096] [--reps 5] [--out profiles/fcg_periodic_time.json]

Workloads: periodic Poisson that is Dirichlet in one direction, so the operator is definite; device-resident vectors,
b random, x0 = 0, V(2,1), point relaxation.
  3d7    seven-point, n3^3, ibc 3 (periodic in x and y)             examples/ser-periodic-3d.cc's operator
  3d27   27-point, n3^3, ibc 5 (periodic in z): gallery::fe with the couplings across the periodic seam added and the
         periodic image in its ghost planes
  2d5    five-point, n2^2, ibc 2 (periodic in x)                    examples/ser-periodic-2d.cc's operator
Per workload, everything in one process:
  (a) ms per fcg_periodic iteration -- a run of N2 = 9 and one of N1 = 3 iterations (tol = 0), host clock around calls that
      end in a device synchronise, difference / (N2 - N1), as tools/fcg_time.py -- against ms per cycle of the same
      handle (cedar_amd_solver_time_vcycles, device events), alternating;
  (b) iterations and wall-clock ms to rel 1e-10 of fcg_periodic against the cycles and ms of cedar_amd_solver_solve;
  (c) the periodic direction pass (cedar_amd_pcg_direction_periodic) against the Dirichlet pass (cedar_amd_pcg_direction,
      Cedar planes) on the same device arrays, ms per call over `calls` calls, alternating.
Every repetition is kept in the output.  Nothing here is a pass criterion.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import problems as pb  # noqa: E402


def fe3_periodic_z(n):
    """gallery::fe made periodic in z: the slots that couple a point to plane k - 1 also on the first plane, then the
    periodic image in the ghost planes"""
    so = pb.fe3(n, n, n)
    for s in (pb.KB, pb.KBW, pb.KBE, pb.KBN, pb.KBS, pb.KBNW, pb.KBNE, pb.KBSE, pb.KBSW):
        so[s, 1] = so[s, 2]
    return pb.wrap3(so, (0, 0, 1))


def workloads(n3, n2):
    return [("3d7", lambda: pb.periodic_poisson3(n3, n3, n3, (1, 1, 0)), 3),
            ("3d27", lambda: fe3_periodic_z(n3), 5),
            ("2d5", lambda: pb.periodic_poisson2(n2, n2, (True, False)), 2)]


def timed(capi, fn):
    capi.sync()
    t0 = time.perf_counter()
    out = fn()
    capi.sync()
    return (time.perf_counter() - t0) * 1e3, out


def measure(capi, name, so, ibc, reps, n1, n2, calls):
    g = so.shape[1:]
    nst = so.shape[0]
    mask = pb.interior_mask(g)
    b = capi.DeviceArray.from_numpy(pb.uniform(g, 17, -1, 1) * mask)
    x = capi.DeviceArray(g)
    so_d = capi.DeviceArray.from_numpy(so)
    res = {"workload": name, "shape": list(g[::-1]), "nstencil": nst, "ibc": ibc, "cycle": "V(2,1)"}
    s = capi.Solver(so_d, nrelax_pre=2, nrelax_post=1, ibc=ibc, max_iter=100, tol=1e-10, share_operator=True)
    try:
        def fcg(max_iter, tol):
            x.zero()
            return timed(capi, lambda: s.fcg_periodic(b, x, max_iter=max_iter, tol=tol))

        def solve():
            x.zero()
            return timed(capi, lambda: s.solve(b, x))

        fcg(2, 0.0)  # warm-up: records the graph, allocates the Krylov vectors
        x.zero()
        s.time_vcycles(x, b, 2)
        it_ms, cyc_ms = [], []
        for _ in range(reps):
            t1, h1 = fcg(n1, 0.0)
            t2, h2 = fcg(n2, 0.0)
            assert len(h1) == n1 + 1 and len(h2) == n2 + 1
            it_ms.append((t2 - t1) / (n2 - n1))
            x.zero()
            cyc_ms.append(s.time_vcycles(x, b, n2 - n1) / (n2 - n1))
        res["per_iteration"] = {"ms_fcg_periodic_iteration": it_ms, "ms_cycle": cyc_ms, "n1": n1, "n2": n2,
                                "median_ratio_iteration_over_cycle": statistics.median(it_ms) / statistics.median(cyc_ms)}
        runs_f = [fcg(60, 1e-10) for _ in range(reps)]
        runs_s = [solve() for _ in range(reps)]
        res["to_rel_1e-10"] = {
            "fcg_periodic": {"iterations": [len(h) - 1 for _, h in runs_f], "ms": [t for t, _ in runs_f],
                             "rel": [float(h[-1]) for _, h in runs_f]},
            "solve": {"cycles": [len(h) - 1 for _, h in runs_s], "ms": [t for t, _ in runs_s],
                      "rel": [float(h[-1]) for _, h in runs_s]}}
    finally:
        s.close()
    # (c) the operator pass alone, on zero-ghost vectors (valid input for both passes)
    K = capi.Kernels()
    z = capi.DeviceArray.from_numpy(pb.uniform(g, 1, -1, 1) * mask)
    p = capi.DeviceArray.from_numpy(pb.uniform(g, 2, -1, 1) * mask)
    pn, w = capi.DeviceArray(g), capi.DeviceArray(g)
    pn.zero()
    w.zero()
    sc = np.zeros(8)
    sc[0], sc[3] = 3.0, 0.3717

    def per(first):
        for _ in range(calls):
            K.pcg_direction_periodic(so_d, z, p, pn, w, ibc, first, sc)

    def dirichlet(first):
        for _ in range(calls):
            K.pcg_direction(so_d, z, p, pn, w, first, sc)

    passes = {}
    for first in (False, True):
        per(first)
        dirichlet(first)
        tp, td = [], []
        for _ in range(reps):
            tp.append(timed(capi, lambda: per(first))[0] / calls)
            td.append(timed(capi, lambda: dirichlet(first))[0] / calls)
        passes["first" if first else "later"] = {"ms_periodic": tp, "ms_dirichlet": td,
                                                 "median_ratio_periodic_over_dirichlet": statistics.median(tp) / statistics.median(td)}
    res["direction_pass"] = dict(passes, calls=calls)
    for a in (b, x, so_d, z, p, pn, w):
        a.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n3", type=int, default=256)
    ap.add_argument("--n2", type=int, default=4096)
    ap.add_argument("--n1-iters", type=int, default=3)
    ap.add_argument("--n2-iters", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--only", default=None, help="3d7, 3d27 or 2d5")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from cedar_amd import capi
    if capi.device_count() < 1:
        raise SystemExit("fcg_periodic_time: no GPU visible (there is no CPU fallback)")
    out = {"reps": a.reps, "workloads": []}
    for name, mk, ibc in workloads(a.n3, a.n2):
        if a.only and a.only != name:
            continue
        out["workloads"].append(measure(capi, name, mk(), ibc, a.reps, a.n1_iters, a.n2_iters, a.calls))
        print(json.dumps(out["workloads"][-1]), flush=True)
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
