#!/usr/bin/env python3
"""What flexible CG (cedar_amd_solver_fcg) costs and what it buys, on the bench workload.

    python tools/fcg_time.py [--n 512] [--reps 3] [--out profiles/fcg_time.json]

Workload: 3D 27-point gallery::fe at n^3 (device gallery), point relaxation, device-resident vectors, x0 = 0.
  (a) ms per iteration of fcg and of pcg on ONE V(1,1) handle, alternating in the same process: a run of N2 = 9 and one
      of N1 = 3 iterations (tol = 0), host clock around calls that end in a device synchronise, per-iteration figure =
      difference / (N2 - N1), as tools/pcg_time.py.  The flexible pass reads w once more per iteration, 8 bytes per
      point: the condition is median(fcg) / median(pcg) <= 1.02.  Exit status 1 when it is missed.
  (b) iterations and wall-clock ms to rel 1e-10 of pcg with V(1,1) and of fcg with V(1,1), V(2,1), F(1,1), F(2,1);
      recorded, not conditioned.
Every repetition is kept in the output.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

CYCLES = [("pcg", "V(1,1)", dict(nrelax_pre=1, nrelax_post=1)),
          ("fcg", "V(1,1)", dict(nrelax_pre=1, nrelax_post=1)),
          ("fcg", "V(2,1)", dict(nrelax_pre=2, nrelax_post=1)),
          ("fcg", "F(1,1)", dict(nrelax_pre=1, nrelax_post=1, cycle="f")),
          ("fcg", "F(2,1)", dict(nrelax_pre=2, nrelax_post=1, cycle="f"))]


def timed_solve(capi, s, which, b, g, **kw):
    x = capi.DeviceArray(g)
    x.zero()
    capi.sync()
    t0 = time.perf_counter()
    h = getattr(s, which)(b, x, **kw)
    ms = (time.perf_counter() - t0) * 1e3
    x.free()
    return ms, h


def per_iteration(capi, s, which, b, g, n1, n2):
    t1, h1 = timed_solve(capi, s, which, b, g, max_iter=n1, tol=0.0)
    t2, h2 = timed_solve(capi, s, which, b, g, max_iter=n2, tol=0.0)
    assert len(h1) == n1 + 1 and len(h2) == n2 + 1
    return (t2 - t1) / (n2 - n1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--n1", type=int, default=3)
    ap.add_argument("--n2", type=int, default=9)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from cedar_amd import capi
    if capi.device_count() < 1:
        raise SystemExit("fcg_time: no GPU visible (there is no CPU fallback)")
    n = a.n
    g = (n + 2,) * 3
    so, b = capi.gallery("fe3", (n, n, n))
    res = {"workload": f"3d27 fe {n}^3, point relaxation, device vectors", "reps": a.reps}
    # (a) the price of the extra dot product
    s = capi.Solver(so, nrelax_pre=1, nrelax_post=1, share_operator=True)
    try:
        for which in ("fcg", "pcg"):  # warm-up: records the graph, allocates the Krylov vectors
            timed_solve(capi, s, which, b, g, max_iter=2, tol=0.0)
        ms = {"fcg": [], "pcg": []}
        for _ in range(a.reps):
            for which in ("fcg", "pcg"):
                ms[which].append(per_iteration(capi, s, which, b, g, a.n1, a.n2))
    finally:
        s.close()
    ratio = statistics.median(ms["fcg"]) / statistics.median(ms["pcg"])
    res["per_iteration_v11"] = {"ms_fcg": ms["fcg"], "ms_pcg": ms["pcg"], "n1": a.n1, "n2": a.n2,
                                "median_ratio_fcg_over_pcg": ratio, "condition": "<= 1.02", "met": ratio <= 1.02}
    # (b) what a non-symmetric cycle buys
    to_tol = []
    for which, name, st in CYCLES:
        s = capi.Solver(so, share_operator=True, **st)
        try:
            timed_solve(capi, s, which, b, g, max_iter=1, tol=0.0)
            runs = [timed_solve(capi, s, which, b, g, max_iter=60, tol=1e-10) for _ in range(a.reps)]
        finally:
            s.close()
        to_tol.append({"solver": which, "cycle": name, "iterations": [len(h) - 1 for _, h in runs],
                       "ms": [t for t, _ in runs], "rel": [float(h[-1]) for _, h in runs]})
    res["to_rel_1e-10"] = to_tol
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")
    return 0 if ratio <= 1.02 else 1


if __name__ == "__main__":
    sys.exit(main())
