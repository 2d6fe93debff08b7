#!/usr/bin/env python3
"""What the single-precision copies of 2D line-relaxed levels are worth (cedar_amd_solver_use_fp32_operator_lines), and
which levels the default (min_rows = 0) should take.

    python tools/op32_lines_time.py [--sizes 8192,4096,2048,1024,512] [--batch-size 2048] [--out profiles/op32_lines_time.json]

Workloads: the nine-point variable-coefficient operator (tests/problems.py varcoef9) and the five-point gallery::poisson
at n^2, zebra line-xy relaxation, V(1,1) and V(2,1), device-resident vectors (8192^2 V(2,1) is the benchmark's third
configuration).  Per operator, size and cycle two handles share ONE operator array, because a switch is never undone and
the two legs are to alternate:
  * leg "fp64":     untouched -- the FP64 line kernels, the baseline;
  * leg "switched": after cedar_amd_solver_use_fp32_operator_lines(min_rows) with an explicit min_rows.
Every shape is warmed up (graph capture, first touch), then the legs alternate within one call of this tool, three
repetitions each, all values kept:
  * ms per cycle (cedar_amd_solver_time_vcycles: HIP events around 5 replays of the captured cycle) with min_rows = n
    (level 0 alone), and then with min_rows stepped down one level at a time on fresh switched handles, to find where
    adding a level stops paying;
  * ms per level-0 line-xy sweep and per level-0 residual (cedar_amd_solver_time_relax / _time_op, HIP events, 6
    launches), and -- on pairs of line-x and line-y handles of the same operator -- per level-0 x sweep and y sweep alone
    (the y sweep with its transposes of b and q);
  * conjugate gradients to 1e-10 from x = 0 (pcg on V(1,1), fcg on V(2,1)): iterations and wall-clock ms.
A pair of max_rhs = 8 handles at --batch-size (varcoef9, V(1,1)) gives the batched cycle at 2, 4 and 8 right-hand sides
(cedar_amd_solver_time_vcycles_many) the same way.

The byte model of a line (operator-derived streams as floats): 68 / 104 = 0.65 for nine-point lines, 0.78 for five-point
lines; it is written beside the measured ratios.

Decision written into the result ("default"): a level size is switched by default only where, for V(1,1) and V(2,1) and
both operators alike, the median of the switched cycle lies below the FP64 median by more than the spread (max - min of
the repetitions) of either leg, at that size (level 0 alone) and at every larger measured size.  Sizes not measured
stay FP64.  If no size meets the rule the default switches nothing.  OP32_LINES_DEFAULT_MIN_ROWS in solver.cpp is set by
hand from this result.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CYCLES = {"v11": dict(nrelax_pre=1, nrelax_post=1), "v21": dict(nrelax_pre=2, nrelax_post=1)}
REPS, NCYC, NK = 3, 5, 6
NRHS = (2, 4, 8)
# nine-point: 9 of the 13 streams of a line as floats.  Five-point: 0.78 is the figure this work was planned with; counting
# the kernel's streams (KS of two rows and three factors as floats, qf, two q rows and the store as doubles) gives 52 / 72 = 0.72
BYTE_MODEL = {"varcoef9": 68.0 / 104.0, "poisson2": 0.78}


def median(v):
    return sorted(v)[len(v) // 2]


def verdict(fp64, switched):
    """ratio of the medians, the spreads, and whether the switched leg wins by more than either spread"""
    m0, m1 = median(fp64), median(switched)
    s0, s1 = max(fp64) - min(fp64), max(switched) - min(switched)
    return {"ratio": m1 / m0, "gain_ms": m0 - m1, "spread_fp64_ms": s0, "spread_switched_ms": s1,
            "faster": bool(m0 - m1 > max(s0, s1))}


def alternate(legs, fn, warm):
    """fn(handle) -> ms: warm both legs up, then alternate them REPS times; {leg: [ms, ...]}"""
    for s in legs.values():
        warm(s)
    out = {k: [] for k in legs}
    for _ in range(REPS):
        for k, s in legs.items():
            out[k].append(fn(s))
    out["verdict"] = verdict(out["fp64"], out["switched"])
    return out


def operator(capi, name, n):
    """(so, b) in HBM"""
    if name == "poisson2":
        return capi.gallery("poisson2", (n, n))
    import problems as pb
    so, b = capi.DeviceArray((5, n + 2, n + 2)), capi.DeviceArray((n + 2, n + 2))
    so.upload(pb.varcoef9(n, n))
    b.upload(pb.rhs2(n, n))
    return so, b


def pair(capi, so, n, relax, **kw):
    """an FP64 handle and one with level 0 alone switched, on one operator array"""
    legs = {"fp64": capi.Solver(so, relax=relax, share_operator=True, **kw),
            "switched": capi.Solver(so, relax=relax, share_operator=True, **kw)}
    got = legs["switched"].use_fp32_operator_lines(n)
    if got != 1 or legs["fp64"].fp32_levels() != 0:
        for s in legs.values():
            s.close()
        raise SystemExit("op32_lines_time: the switch did not take level 0 alone: %r" % got)
    return legs


def sweeps_alone(capi, n, so, b):
    """level-0 x sweep and y sweep alone: line-x and line-y handles of the same operator"""
    x = capi.DeviceArray((n + 2, n + 2))
    res = {}
    try:
        for relax in ("line-x", "line-y"):
            legs = pair(capi, so, n, relax, **CYCLES["v11"])
            try:
                x.zero()
                res[relax] = alternate(legs, lambda s: s.time_relax(x, b, NK) / NK, lambda s: s.time_relax(x, b, 2))
            finally:
                for s in legs.values():
                    s.close()
    finally:
        x.free()
    return res


def one_size(capi, name, n, so, b, cyc, depth):
    g = (n + 2, n + 2)
    kw = dict(relax="line-xy", share_operator=True, **CYCLES[cyc])
    legs = pair(capi, so, n, "line-xy", **CYCLES[cyc])
    x = capi.DeviceArray(g)
    res = {"levels": [list(legs["fp64"].dims(l)) for l in range(legs["fp64"].nlevels())], "fp32_levels": 1,
           "byte_model": BYTE_MODEL[name]}
    extra = []
    try:
        x.zero()
        res["vcycle_ms"] = alternate(legs, lambda s: s.time_vcycles(x, b, NCYC) / NCYC, lambda s: s.time_vcycles(x, b, 2))
        res["relax0_ms"] = alternate(legs, lambda s: s.time_relax(x, b, NK) / NK, lambda s: s.time_relax(x, b, 2))
        res["residual0_ms"] = alternate(legs, lambda s: s.time_op(x, b, "residual", NK) / NK, lambda s: s.time_op(x, b, "residual", 2))
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
        # min_rows one level down at a time: fresh switched handles against the same FP64 leg
        res["by_min_rows"] = {}
        rows = n
        for _ in range(depth):
            rows = (rows - 1) // 2 + 1
            if rows <= 64:
                break
            s = capi.Solver(so, **kw)
            extra.append(s)
            nl = s.use_fp32_operator_lines(rows)
            x.zero()
            r = alternate({"fp64": legs["fp64"], "switched": s}, lambda h: h.time_vcycles(x, b, NCYC) / NCYC,
                          lambda h: h.time_vcycles(x, b, 2))
            r["fp32_levels"] = nl
            res["by_min_rows"][str(rows)] = r
    finally:
        for s in list(legs.values()) + extra:
            s.close()
        x.free()
    return res


def batch(capi, n):
    g = (n + 2, n + 2)
    so, b = operator(capi, "varcoef9", n)
    legs = pair(capi, so, n, "line-xy", max_rhs=max(NRHS), **CYCLES["v11"])
    bb, xx = capi.DeviceArray((max(NRHS),) + g), capi.DeviceArray((max(NRHS),) + g)
    for m in range(max(NRHS)):
        capi.lib.cedar_amd_memcpy_d2d(bb.ptr + m * b.size * 8, b.ptr, b.size * 8)

    class View:  # the first nrhs items of a DeviceArray
        def __init__(self, d, nrhs):
            self.ptr, self.shape = d.ptr, (nrhs,) + g

    res = {"n": n, "cycle": "v11", "operator": "varcoef9", "fp32_levels": 1}
    try:
        for k in NRHS:
            xx.zero()
            res[str(k)] = alternate(legs, lambda s: s.time_vcycles_many(View(xx, k), View(bb, k), NCYC) / NCYC,
                                    lambda s: s.time_vcycles_many(View(xx, k), View(bb, k), 2))
    finally:
        for s in legs.values():
            s.close()
        for d in (bb, xx, so, b):
            d.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8192,4096,2048,1024,512")
    ap.add_argument("--operators", default="varcoef9,poisson2")
    ap.add_argument("--depth", type=int, default=2, help="levels below level 0 that by_min_rows adds, one at a time")
    ap.add_argument("--batch-size", type=int, default=2048, help="n of the batch handles (0: skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from cedar_amd import capi
    if capi.device_count() < 1:
        raise SystemExit("op32_lines_time: no GPU visible (there is no CPU fallback)")
    res = {"workload": "2D varcoef9 (nine-point) and poisson2 (five-point level 0) n^2, zebra line-xy, V(1,1) and V(2,1); two "
                       "handles on one operator, legs alternating; ms by HIP events, Krylov wall clock",
           "repetitions": REPS, "byte_model": BYTE_MODEL, "sizes": {}}

    def write():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            open(a.out, "w").write(json.dumps(res) + "\n")

    names = a.operators.split(",")
    for n in [int(v) for v in a.sizes.split(",")]:
        res["sizes"][str(n)] = {}
        for name in names:
            so, b = operator(capi, name, n)
            try:
                r = {cyc: one_size(capi, name, n, so, b, cyc, a.depth) for cyc in CYCLES}
                r["sweeps_alone_ms"] = sweeps_alone(capi, n, so, b)
                res["sizes"][str(n)][name] = r
            finally:
                so.free()
                b.free()
            print("op32_lines_time: %s %d^2 done" % (name, n), file=sys.stderr, flush=True)
            write()
    if a.batch_size:
        res["batch"] = batch(capi, a.batch_size)
        write()
    # the default: the smallest size from which every measured size at or above it wins on both cycles and operators
    wins = {int(n): all(r[name][c]["vcycle_ms"]["verdict"]["faster"] for name in names for c in CYCLES)
            for n, r in res["sizes"].items()}
    rows = None
    for n in sorted(wins, reverse=True):
        if not wins[n]:
            break
        rows = n
    res["default"] = {"wins": {str(k): v for k, v in wins.items()}, "min_rows": rows,
                      "rule": "median of the switched cycle (level 0 alone) below the FP64 median by more than the spread of "
                              "either leg, V(1,1) and V(2,1), both operators; null: the default switches nothing"}
    write()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
