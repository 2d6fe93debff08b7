#!/usr/bin/env python3
"""Timing and iteration counts of the multigrid-preconditioned CG (cedar_amd_solver_pcg) on the bench workload.

    python tools/pcg_time.py [--n 512] [--contrast-n 192] [--out profiles/pcg_time.json]
    python tools/pcg_time.py --stats KERNEL_STATS_CSV [--n 512]    # Krylov kernels' TB/s from a rocprofv3 --stats run

Workload: 3D 27-point gallery::fe at n^3 (device gallery), V(1,1) point relaxation, x0 = 0.
  * ms per PCG iteration and ms per stationary cycle of `solve`: a run of N2 and one of N1 iterations (tol = 0),
    host clock around calls that end in a device synchronise (both loops read one norm per iteration), per-iteration
    figure = difference / (N2 - N1), so set-up, the initial residual and the first preconditioner drop out;
  * of it the preconditioner: one V-cycle on the solver's graph (cedar_amd_solver_time_vcycles, HIP events) plus
    the clear of z; the rest is the Krylov kernels and the host's read of the scalars;
  * iterations to rel 1e-10 of PCG and of the stationary solve on that workload and on a high-contrast 7-point
    problem (two-phase coefficients, contrast 1e6, tests/pcg_statement.py).
Each kernel's TB/s needs its duration: run the same command under `rocprofv3 --kernel-trace --stats` and pass the
stats CSV with --stats; algorithmic bytes per interior point are those stated in cedar_amd/csrc/krylov.hip.
"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

# algorithmic bytes per interior point of each Krylov kernel (krylov.hip header); pcg_dir27 on the row-interleaved
# copy reads 15 slot-rows of 16 (slot 14, 1/diag, is not read): 152 B; on the Cedar planes 144 B
BYTES = {"pcg_dir27": 152, "pcg_upd": 48, "pcg_dots": 16}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def per_iteration(capi, s, b, n1, n2, which, g, s1=None):
    """ms per iteration: difference of a run of n2 and one of n1 iterations (solve: s1 / s were created with
    max_iter n1 / n2 and tol 0)"""
    ts = []
    for n, sv in ((n1, s1 or s), (n2, s)):
        x = capi.DeviceArray(g)
        x.zero()
        if which == "pcg":
            ms, _ = timed(lambda: sv.pcg(b, x, max_iter=n, tol=0.0))
        else:
            ms, h = timed(lambda: sv.solve(b, x))
            assert len(h) == n + 1
        ts.append(ms)
    return (ts[1] - ts[0]) / (n2 - n1)


def iterations(capi, so, b, tol=1e-10, maxit=300, **st):
    import numpy as np
    out = {}
    s = capi.Solver(so, nrelax_pre=1, nrelax_post=1, max_iter=maxit, tol=tol, **st)
    try:
        x = capi.DeviceArray(b.shape) if not isinstance(b, np.ndarray) else np.zeros_like(b)
        if not isinstance(x, np.ndarray):
            x.zero()
        h = s.pcg(b, x, max_iter=maxit, tol=tol)
        out["pcg"] = len(h) - 1 if h[-1] < tol else f">{maxit} (rel {h[-1]:.2e}, best {min(h[1:]):.2e})"
        x = capi.DeviceArray(b.shape) if not isinstance(b, np.ndarray) else np.zeros_like(b)
        if not isinstance(x, np.ndarray):
            x.zero()
        h = s.solve(b, x)
        out["solve"] = len(h) - 1 if h[-1] < tol else f">{maxit} (rel {h[-1]:.2e}, best {min(h[1:]):.2e})"
    finally:
        s.close()
    return out


def from_stats(path, n):
    """per Krylov kernel of a rocprofv3 --stats CSV: calls, average ms, algorithmic TB/s at n^3 interior points"""
    import re
    pts = float(n) ** 3
    res = {}
    for r in csv.DictReader(open(path)):
        m = re.search(r"(pcg_\w+)(<[^>]*>)?", r.get("Name") or r.get("KernelName") or "")
        if not m:
            continue
        name, targs = m.group(1), (m.group(2) or "").replace(" ", "")
        what = {"pcg_dir27": "pcg_dir27", "pcg_upd": "pcg_dots" if targs == "<2,false>" else "pcg_upd"}.get(name)
        avg_ns = float(r.get("AverageNs", 0) or 0)
        ent = {"calls": int(r.get("Calls", 0) or 0), "avg_ms": avg_ns * 1e-6}
        if what:
            ent["bytes_per_point"] = BYTES[what] - (8 if targs == "<256,true>" else 0)  # first iteration: p not read
            ent["TB_per_s"] = ent["bytes_per_point"] * pts / (avg_ns * 1e-9) / 1e12
        res[name + targs] = ent
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--contrast-n", type=int, default=192)
    ap.add_argument("--n1", type=int, default=4)
    ap.add_argument("--n2", type=int, default=14)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--solve-only", action="store_true", help="one PCG solve to 1e-10 (the run to trace)")
    a = ap.parse_args()
    if a.stats:
        print(json.dumps(from_stats(a.stats, a.n), indent=1))
        return
    from cedar_amd import capi
    import pcg_statement as ps
    if capi.device_count() < 1:
        raise SystemExit("pcg_time: no GPU visible (there is no CPU fallback)")
    n = a.n
    g = (n + 2,) * 3
    so, b = capi.gallery("fe3", (n, n, n))
    res = {"workload": f"3d27 fe {n}^3 V(1,1)"}
    s = capi.Solver(so, nrelax_pre=1, nrelax_post=1, share_operator=True, tol=0.0, max_iter=a.n2)
    s1 = None
    try:
        if a.solve_only:
            x = capi.DeviceArray(g)
            x.zero()
            h = s.pcg(b, x, tol=1e-10)
            print(json.dumps({"pcg_iterations": len(h) - 1, "rel": float(h[-1])}))
            return
        s1 = capi.Solver(so, nrelax_pre=1, nrelax_post=1, share_operator=True, tol=0.0, max_iter=a.n1)
        # warm-up: records the graphs, allocates the PCG vectors
        per_iteration(capi, s, b, 1, 2, "pcg", g)
        per_iteration(capi, s, b, a.n1, a.n2, "solve", g, s1)
        pcg_ms = min(per_iteration(capi, s, b, a.n1, a.n2, "pcg", g) for _ in range(3))
        solve_ms = min(per_iteration(capi, s, b, a.n1, a.n2, "solve", g, s1) for _ in range(3))
        s1.close()
        x = capi.DeviceArray(g)
        x.zero()
        s.time_vcycles(x, b, 2)
        vc_ms = min(s.time_vcycles(x, b, 10) / 10 for _ in range(2))
        res.update({"ms_per_pcg_iteration": pcg_ms, "ms_per_solve_cycle": solve_ms, "ratio": pcg_ms / solve_ms,
                    "ms_vcycle_preconditioner": vc_ms, "ms_krylov_and_host": pcg_ms - vc_ms,
                    "ms_residual_and_norm_of_solve": solve_ms - vc_ms})
    finally:
        s.close()
        if s1:
            s1.close()
    res["iterations_to_1e-10_3d27"] = iterations(capi, so, b, share_operator=True)
    del so, b
    m = a.contrast_n
    soc = ps.high_contrast7(m, m, m)
    bc = ps.random_field(soc.shape[1:], 7)
    res["iterations_to_1e-10_contrast7"] = dict(iterations(capi, soc, bc), n=f"{m}^3")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
