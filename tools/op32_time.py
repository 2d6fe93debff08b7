#!/usr/bin/env python3
"""What keeping the 27-point operator of the cycle in single precision is worth (cedar_amd_solver_use_fp32_operator).

    python tools/op32_time.py [--sizes 512,256,128] [--out profiles/op32_time.json]

Workload: 3D 27-point gallery::fe at n^3 (device gallery), V(1,1) point relaxation, device-resident vectors.  Per size,
on ONE handle in one process, FP64 first and then after the switch:
  * ms per V-cycle (cedar_amd_solver_time_vcycles: HIP events around 5 replays of the captured cycle, 3 repetitions kept);
  * ms per level-0 relax sweep and per level-0 residual (cedar_amd_solver_time_relax / _time_op, 6 launches);
  * conjugate gradients to 1e-10 from x = 0: iterations and wall-clock ms.
The switch is made level by level: min_rows = n (level 0 alone), then n/2, n/4, .., 1, with the V-cycle timed after every
step -- a switch is never undone, so the steps are cumulative and the difference of two neighbours is what the copy is
worth on the level the step added.  The level-0 sweep of the size-n handle is also the measurement of "a level with n
rows": the same kernels, launch sizes and bytes as a coarse level of that size.
CEDAR_AMD_OP32_MIN_ROWS is not set here: every call passes its min_rows.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST = dict(nrelax_pre=1, nrelax_post=1)
REPS, NCYC, NK = 3, 5, 6


def measure(capi, s, x, b, with_pcg):
    out = {}
    x.zero()
    s.time_vcycles(x, b, 2)  # capture, first touch
    out["vcycle_ms"] = [s.time_vcycles(x, b, NCYC) / NCYC for _ in range(REPS)]
    s.time_relax(x, b, 2)
    out["relax0_ms"] = [s.time_relax(x, b, NK) / NK for _ in range(REPS)]
    s.time_op(x, b, "residual", 2)
    out["residual0_ms"] = [s.time_op(x, b, "residual", NK) / NK for _ in range(REPS)]
    if with_pcg:
        x.zero()
        s.pcg(b, x, max_iter=2, tol=0.0)  # Krylov storage, the cycle on (z, r)
        x.zero()
        capi.sync()
        t0 = time.perf_counter()
        h = s.pcg(b, x, max_iter=60, tol=1e-10)
        capi.sync()
        out["pcg_1e-10"] = {"iterations": len(h) - 1, "ms": 1e3 * (time.perf_counter() - t0), "last_rel": float(h[-1])}
    return out


def one_size(capi, n):
    g = (n + 2,) * 3
    so, b = capi.gallery("fe3", (n, n, n))
    s = capi.Solver(so, share_operator=True, **ST)
    x = capi.DeviceArray(g)
    res = {"levels": [list(s.dims(l)) for l in range(s.nlevels())]}
    try:
        res["fp64"] = measure(capi, s, x, b, True)
        steps, m = [], n
        while m >= 1:
            levels = s.use_fp32_operator(m)
            if levels < 0:
                raise SystemExit("op32_time: the switch was refused")
            if not steps or levels != steps[-1]["fp32_levels"]:
                last = m == 1
                r = measure(capi, s, x, b, last or not steps)
                r.update(min_rows=m, fp32_levels=levels)
                steps.append(r)
            m = 1 if 1 < m < 16 else m // 2
        res["fp32_steps"] = steps
    finally:
        s.close()
        x.free()
        so.free()
        b.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,256,128")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from cedar_amd import capi
    if capi.device_count() < 1:
        raise SystemExit("op32_time: no GPU visible (there is no CPU fallback)")
    res = {"workload": "3d27 fe n^3 V(1,1); ms per cycle / sweep / residual by HIP events, pcg wall clock",
           "repetitions": REPS, "sizes": {}}
    for n in [int(v) for v in a.sizes.split(",")]:
        res["sizes"][str(n)] = one_size(capi, n)
        print("op32_time: %d^3 done" % n, file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
