#!/usr/bin/env python3
"""What the single-precision copy of the 7-point level is worth (cedar_amd_solver_use_fp32_operator_all), and whether the
default (min_rows = 0) should take it.

    python tools/op32_7pt_time.py [--sizes 512,256,128] [--batch-size 256] [--out profiles/op32_7pt_time.json]

Workload: 3D 7-point gallery::poisson at n^3 (device gallery), V(1,1) and V(2,1) point relaxation, device-resident
vectors.  Per size and cycle two handles share ONE operator array, because a switch is never undone and the two legs are
to alternate:
  * leg "fp64":     after cedar_amd_solver_use_fp32_operator(0) -- the 27-point levels switched by the existing default,
                    level 0 in FP64.  This is the baseline;
  * leg "switched": after cedar_amd_solver_use_fp32_operator_all(128) -- the same 27-point levels (their default is 128
                    rows) and the 7-point level 0.  The difference of the two legs is the 7-point level.
Every shape is warmed up (graph capture, first touch), then the legs alternate within one call of this tool, three
repetitions each, all values kept:
  * ms per cycle (cedar_amd_solver_time_vcycles: HIP events around 5 replays of the captured cycle);
  * ms per level-0 sweep and per level-0 residual (cedar_amd_solver_time_relax / _time_op, HIP events, 6 launches);
  * conjugate gradients to 1e-10 from x = 0 (pcg on V(1,1), fcg on V(2,1)): iterations and wall-clock ms.
A pair of max_rhs = 8 handles at --batch-size (V(1,1)) gives the batched cycle at 2, 4 and 8 right-hand sides
(cedar_amd_solver_time_vcycles_many) the same way.

Decision written into the result ("default"): the switch becomes the default at a size when, for V(1,1) and V(2,1) alike,
the median of the switched cycle lies below the FP64 median by more than the spread (max - min of the repetitions) of
either leg.  Where that fails the default leaves the 7-point level in FP64 and an explicit min_rows > 0 still switches it.
OP32_7PT_DEFAULT_MIN_ROWS in solver.cpp is set by hand from this result.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CYCLES = {"v11": dict(nrelax_pre=1, nrelax_post=1), "v21": dict(nrelax_pre=2, nrelax_post=1)}
REPS, NCYC, NK = 3, 5, 6
MIN_ROWS = 128  # the 27-point default: _all(128) switches the same 27-point levels as use_fp32_operator(0)
NRHS = (2, 4, 8)


def median(v):
    return sorted(v)[len(v) // 2]


def verdict(fp64, switched):
    """ratio of the medians, the spreads, and whether the switched leg wins by more than either spread"""
    m0, m1 = median(fp64), median(switched)
    s0, s1 = max(fp64) - min(fp64), max(switched) - min(switched)
    return {"ratio": m1 / m0, "gain_ms": m0 - m1, "spread_fp64_ms": s0, "spread_switched_ms": s1,
            "faster": bool(m0 - m1 > max(s0, s1))}


def alternate(legs, fn, warm):
    """fn(handle, count) -> ms: warm both legs up, then alternate them REPS times; {leg: [ms, ...]}"""
    for s in legs.values():
        warm(s)
    out = {k: [] for k in legs}
    for _ in range(REPS):
        for k, s in legs.items():
            out[k].append(fn(s))
    return out


def one_size(capi, n, cyc):
    g = (n + 2,) * 3
    so, b = capi.gallery("poisson3", (n, n, n))
    legs = {"fp64": capi.Solver(so, share_operator=True, **CYCLES[cyc]), "switched": capi.Solver(so, share_operator=True, **CYCLES[cyc])}
    x = capi.DeviceArray(g)
    res = {"levels": [list(legs["fp64"].dims(l)) for l in range(legs["fp64"].nlevels())]}
    try:
        res["fp32_levels"] = {"fp64": legs["fp64"].use_fp32_operator(0), "switched": legs["switched"].use_fp32_operator_all(MIN_ROWS)}
        if min(res["fp32_levels"].values()) < 0 or res["fp32_levels"]["switched"] != res["fp32_levels"]["fp64"] + 1:
            raise SystemExit("op32_7pt_time: the switch did not take the 7-point level alone: %r" % res["fp32_levels"])
        x.zero()
        res["vcycle_ms"] = alternate(legs, lambda s: s.time_vcycles(x, b, NCYC) / NCYC, lambda s: s.time_vcycles(x, b, 2))
        res["relax0_ms"] = alternate(legs, lambda s: s.time_relax(x, b, NK) / NK, lambda s: s.time_relax(x, b, 2))
        res["residual0_ms"] = alternate(legs, lambda s: s.time_op(x, b, "residual", NK) / NK, lambda s: s.time_op(x, b, "residual", 2))
        for key in ("vcycle_ms", "relax0_ms", "residual0_ms"):
            res[key]["verdict"] = verdict(res[key]["fp64"], res[key]["switched"])
        kind = "pcg" if cyc == "v11" else "fcg"
        res["krylov"] = {"method": kind}
        for k, s in legs.items():
            x.zero()
            getattr(s, kind)(b, x, max_iter=2, tol=0.0)  # Krylov storage, the cycle on (z, r)
            x.zero()
            capi.sync()
            t0 = time.perf_counter()
            h = getattr(s, kind)(b, x, max_iter=60, tol=1e-10)
            capi.sync()
            res["krylov"][k] = {"iterations": len(h) - 1, "ms": 1e3 * (time.perf_counter() - t0), "last_rel": float(h[-1])}
    finally:
        for s in legs.values():
            s.close()
        x.free()
        so.free()
        b.free()
    return res


def batch(capi, n):
    g = (n + 2,) * 3
    so, b = capi.gallery("poisson3", (n, n, n))
    kw = dict(share_operator=True, max_rhs=max(NRHS), **CYCLES["v11"])
    legs = {"fp64": capi.Solver(so, **kw), "switched": capi.Solver(so, **kw)}
    bb, xx = capi.DeviceArray((max(NRHS),) + g), capi.DeviceArray((max(NRHS),) + g)
    for m in range(max(NRHS)):
        capi.lib.cedar_amd_memcpy_d2d(bb.ptr + m * b.size * 8, b.ptr, b.size * 8)

    class View:  # the first nrhs items of a DeviceArray
        def __init__(self, d, nrhs):
            self.ptr, self.shape = d.ptr, (nrhs,) + g

    res = {"n": n, "cycle": "v11"}
    try:
        res["fp32_levels"] = {"fp64": legs["fp64"].use_fp32_operator_many(0), "switched": legs["switched"].use_fp32_operator_all(MIN_ROWS)}
        if min(res["fp32_levels"].values()) < 0:
            raise SystemExit("op32_7pt_time: the batch switch was refused")
        for k in NRHS:
            xx.zero()
            r = alternate(legs, lambda s: s.time_vcycles_many(View(xx, k), View(bb, k), NCYC) / NCYC,
                          lambda s: s.time_vcycles_many(View(xx, k), View(bb, k), 2))
            r["verdict"] = verdict(r["fp64"], r["switched"])
            res[str(k)] = r
    finally:
        for s in legs.values():
            s.close()
        for d in (bb, xx, so, b):
            d.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,256,128")
    ap.add_argument("--batch-size", type=int, default=256, help="n of the batch handles (0: skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from cedar_amd import capi
    if capi.device_count() < 1:
        raise SystemExit("op32_7pt_time: no GPU visible (there is no CPU fallback)")
    res = {"workload": "3d7 poisson n^3, V(1,1) and V(2,1); two handles on one operator, legs alternating; ms by HIP events, "
                       "Krylov wall clock", "repetitions": REPS, "min_rows_of_the_switched_leg": MIN_ROWS, "sizes": {}}

    def write():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            open(a.out, "w").write(json.dumps(res) + "\n")

    for n in [int(v) for v in a.sizes.split(",")]:
        res["sizes"][str(n)] = {cyc: one_size(capi, n, cyc) for cyc in CYCLES}
        print("op32_7pt_time: %d^3 done" % n, file=sys.stderr, flush=True)
        write()
    if a.batch_size:
        res["batch"] = batch(capi, a.batch_size)
        write()
    # the default: the smallest size from which every measured size at or above it wins on both cycles
    wins = {int(n): all(r[c]["vcycle_ms"]["verdict"]["faster"] for c in CYCLES) for n, r in res["sizes"].items()}
    rows = None
    for n in sorted(wins, reverse=True):
        if not wins[n]:
            break
        rows = n
    res["default"] = {"wins": {str(k): v for k, v in wins.items()}, "min_rows": rows,
                      "rule": "median of the switched cycle below the FP64 median by more than the spread of either leg, V(1,1) and V(2,1)"}
    write()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
