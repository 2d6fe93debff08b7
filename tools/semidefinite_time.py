#!/usr/bin/env python3
"""What a semidefinite solve (cedar_amd_solver_create_semidefinite, cedar_amd_solver_fcg_semidefinite) costs.

    python tools/semidefinite_time.py [--n3 256] [--n2 4096] [--reps 5] [--out profiles/semidefinite_time.json]

Workloads: operators with zero row sums, device-resident vectors, b random (not compatible: the call projects), x0 = 0,
V(2,1), tolerance 1e-10.
  3d7per    seven-point, n3^3, fully periodic (ibc 8)              problems.periodic_poisson3
  3d7neu    seven-point, n3^3, pure Neumann (ibc 0)                constant couplings 1 / (1 + slot), none across a side,
  3d27neu   27-point, n3^3, pure Neumann (ibc 0)                   diagonal = the sum of the couplings that touch the point
  2d5per    five-point, n2^2, fully periodic (ibc 3), point        problems.periodic_poisson2 with the ghost corners
  2d5perxy  the same, line-xy relaxation                           wrapped
Per workload, everything in one process:
  (a) iterations and wall-clock ms of fcg_semidefinite (host clock around calls that end in a device synchronise);
  (b) ms of one projection (cedar_amd_project_mean on a device vector of the level-0 extents) and the share of the
      solve's projections in (a): r0, the final x, and r and z around every cycle, 2 n + 1 for n iterations;
  (c) ms per cycle (cedar_amd_solver_time_vcycles, device events) of the semidefinite handle against a definite handle
      of the same ibc, size and relaxation made from the same operator with 1e-3 diag added, alternating.  The cycles
      differ only in the coarsest solve (the mean removal at ibc == 0), so the ratio is expected at 1.
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


def neumann_op(g, nst):
    """zero-sum operator on the grid g (ghosts included, slowest first) in the manner of problems.regime_op with
    p_zero = 1: coupling of slot s = 1 / (1 + s), none across a side, diagonal = the sum of the couplings at the point"""
    nd = len(g)
    inner = tuple(slice(1, -1) for _ in g)
    ext = tuple(n - 2 for n in g)
    so = np.zeros((nst,) + tuple(g))
    R = np.zeros(ext)
    offs = pb.slot_offsets(nd, nst)
    for s in range(1, nst):
        v = np.full(ext, 1.0 / (1 + s))
        for o in offs[s]:
            for d in range(nd):
                if o[d]:
                    v[tuple(slice(0, 1) if e == d else slice(None) for e in range(nd))] = 0.0
        for o in offs[s]:
            R += np.roll(v, o, axis=tuple(range(nd)))
        so[s][inner] = v
    so[0][inner] = R
    return so


def wrapped_poisson2(n):
    so = pb.periodic_poisson2(n, n, (1, 1))
    pb.wrap3(so[:, None], (1, 1, 0))
    return so


def workloads(n3, n2):
    return [("3d7per", lambda: pb.periodic_poisson3(n3, n3, n3, (1, 1, 1)), 8, "point"),
            ("3d7neu", lambda: neumann_op((n3 + 2,) * 3, 4), 0, "point"),
            ("3d27neu", lambda: neumann_op((n3 + 2,) * 3, 14), 0, "point"),
            ("2d5per", lambda: wrapped_poisson2(n2), 3, "point"),
            ("2d5perxy", lambda: wrapped_poisson2(n2), 3, "line-xy")]


def timed(capi, fn):
    capi.sync()
    t0 = time.perf_counter()
    out = fn()
    capi.sync()
    return (time.perf_counter() - t0) * 1e3, out


def measure(capi, name, so, ibc, relax, reps, ncyc):
    g = so.shape[1:]
    mask = pb.interior_mask(g)
    b = capi.DeviceArray.from_numpy(pb.uniform(g, 17, -1, 1) * mask)
    x = capi.DeviceArray(g)
    so_d = capi.DeviceArray.from_numpy(so)
    res = {"workload": name, "shape": list(g[::-1]), "nstencil": so.shape[0], "ibc": ibc, "relaxation": relax, "cycle": "V(2,1)"}
    st = dict(relax=relax, nrelax_pre=2, nrelax_post=1, ibc=ibc, max_iter=100, tol=1e-10)
    s = capi.Solver(so_d, semidefinite=True, share_operator=True, **st)
    so[0] *= 1.0 + 1e-3
    sdef = capi.Solver(so, **st)
    del so
    K = capi.Kernels()
    try:
        def fcg():
            x.zero()
            return timed(capi, lambda: s.fcg_semidefinite(b, x, max_iter=100, tol=1e-10))

        def project():
            return timed(capi, lambda: K.project_mean(x))[0]

        fcg()  # warm-up: records the graph, allocates the Krylov vectors
        project()
        runs = [fcg() for _ in range(reps)]
        proj = [project() for _ in range(reps)]
        ms = [t for t, _ in runs]
        res["to_rel_1e-10"] = {"iterations": [len(h) - 1 for _, h in runs], "ms": ms, "rel": [float(h[-1]) for _, h in runs],
                               "ms_one_projection": proj,
                               "projections_per_solve": 2 * (len(runs[0][1]) - 1) + 1,
                               "median_share_of_projections": (2 * (len(runs[0][1]) - 1) + 1) * statistics.median(proj)
                               / statistics.median(ms)}
        x.zero()
        s.time_vcycles(x, b, 2)
        sdef.time_vcycles(x, b, 2)
        cs, cd = [], []
        for _ in range(reps):
            x.zero()
            cs.append(s.time_vcycles(x, b, ncyc) / ncyc)
            x.zero()
            cd.append(sdef.time_vcycles(x, b, ncyc) / ncyc)
        res["cycle"] = {"ms_semidefinite": cs, "ms_definite": cd, "cycles": ncyc,
                        "median_ratio_semidefinite_over_definite": statistics.median(cs) / statistics.median(cd)}
    finally:
        s.close()
        sdef.close()
    for a in (b, x, so_d):
        a.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n3", type=int, default=256)
    ap.add_argument("--n2", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cycles", type=int, default=5)
    ap.add_argument("--only", default=None, help="one of the workload names")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from cedar_amd import capi
    if capi.device_count() < 1:
        raise SystemExit("semidefinite_time: no GPU visible (there is no CPU fallback)")
    out = {"reps": a.reps, "workloads": []}
    for name, mk, ibc, relax in workloads(a.n3, a.n2):
        if a.only and a.only != name:
            continue
        out["workloads"].append(measure(capi, name, mk(), ibc, relax, a.reps, a.cycles))
        print(json.dumps(out["workloads"][-1]), flush=True)
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
