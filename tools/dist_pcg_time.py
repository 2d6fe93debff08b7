#!/usr/bin/env python3
"""Time per iteration and iterations to 1e-10 of the distributed PCG (cedar_amd_dist3_pcg) against the distributed
stationary solve (cedar_amd_dist3_solve) on one rank over RCCL.

    python tools/dist_pcg_time.py [--n 512] [--out profiles/dist_pcg_time.json]

Workload: 3D 27-point gallery::fe at n^3 (device gallery), V(1,1), x0 = 0, a 1 x 1 x 1 rank grid on the library's RCCL
communicator (NativeComm): the per-iteration work of the decomposed path -- two all-gathers of the partial sums, the
halo calls, the gathered coarse level -- with the messages of one rank.  The loop-back transport is not used: its ghost
values are meaningless, and CG's scalars would be too.
  * ms per iteration: a run of N2 and one of N1 iterations (tol = 0), host clock around calls that end in a device
    synchronise, figure = difference / (N2 - N1) (set-up, initial residual and first preconditioner drop out).  The
    solve's cycle count is fixed when the handle is made, so its N1 run has a handle of its own;
  * iterations to rel 1e-10: PCG with tol 1e-10, the solve from the history of its N2-cycle run.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--n1", type=int, default=4)
    ap.add_argument("--n2", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29731")
    from cedar_amd import capi
    from cedar_amd.comm import NativeComm
    from cedar_amd.dist3 import DistSolver3
    if capi.device_count() < 1:
        raise SystemExit("dist_pcg_time: no GPU visible (there is no CPU fallback)")
    capi.set_device(0)
    n = a.n
    g = (n + 2,) * 3
    so, b = capi.gallery("fe3", (n, n, n))
    comm = NativeComm(0, 1)
    res = {"workload": f"3d27 fe {n}^3 V(1,1), 1x1x1 rank grid over RCCL", "n1": a.n1, "n2": a.n2}

    def fresh():
        x = capi.DeviceArray(g)
        x.zero()
        return x

    def solve_ms(s, ncyc):
        best, hist = None, None
        for _ in range(a.reps + 1):  # the first run warms up
            ms, hist = timed(lambda: s.solve(b, fresh()))
            assert len(hist) == ncyc + 1
            best = ms if best is None else min(best, ms)
        return best, hist

    try:
        s = DistSolver3(comm, 0, 1, so, pgrid=(1, 1, 1), nrelax_pre=1, nrelax_post=1, max_iter=a.n1, tol=0.0)
        t1, _ = solve_ms(s, a.n1)
        s.close()
        s = DistSolver3(comm, 0, 1, so, pgrid=(1, 1, 1), nrelax_pre=1, nrelax_post=1, max_iter=a.n2, tol=0.0)
        t2, hsolve = solve_ms(s, a.n2)
        s.pcg(b, fresh(), max_iter=2, tol=0.0)  # warm-up: allocates the Krylov vectors
        tp = {}
        for k in (a.n1, a.n2):
            tp[k] = min(timed(lambda: s.pcg(b, fresh(), max_iter=k, tol=0.0))[0] for _ in range(a.reps))
        hpcg = s.pcg(b, fresh(), max_iter=100, tol=1e-10)
        s.close()
    finally:
        comm.close()
    pcg_ms = (tp[a.n2] - tp[a.n1]) / (a.n2 - a.n1)
    cyc_ms = (t2 - t1) / (a.n2 - a.n1)
    below = [i for i, v in enumerate(hsolve) if i > 0 and v < 1e-10]
    res.update({"ms_per_pcg_iteration": pcg_ms, "ms_per_solve_cycle": cyc_ms, "ratio": pcg_ms / cyc_ms,
                "iterations_to_1e-10": {"pcg": len(hpcg) - 1 if hpcg[-1] < 1e-10 else f">100 (rel {hpcg[-1]:.2e})",
                                        "solve": below[0] if below else f">{a.n2} (rel {hsolve[-1]:.2e})"},
                "pcg_history": [float(v) for v in hpcg], "solve_history": [float(v) for v in hsolve]})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
