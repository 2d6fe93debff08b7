#!/usr/bin/env python3
"""What single-precision interpolation weights are worth to the cycle's grid transfers
(cedar_amd_solver_use_fp32_interpolation), and from which level size the default (min_rows = 0) should switch.

    python tools/ci32_time.py [--sizes3 512,256,128] [--size2-point 4096,2048,1024] [--size2-lines 8192,2048] [--batch-size 256]
                              [--out profiles/ci32_time.json]

Workloads, device-resident vectors, V(1,1) and V(2,1):
  * 3D n^3: the 27-point fe operator and the 7-point gallery::poisson, each on FP64 operators ("fp64op") and on top of
    cedar_amd_solver_use_fp32_operator_all ("op32": both legs take that switch);
  * 2D: the nine-point varcoef9 with point relaxation (on top of nothing and of _2d) and with line-xy relaxation (on top of
    nothing and of _lines);
  * a pair of max_rhs = 8 handles of the 27-point operator: the batched cycle at 2, 4 and 8 right-hand sides.
Per workload two handles share ONE operator array, because a switch is never undone and the two legs are to alternate:
  * leg "fp64":     FP64 weights, the baseline;
  * leg "switched": after cedar_amd_solver_use_fp32_interpolation(min_rows) with an explicit min_rows.
A third handle, "control", is a second untouched FP64 handle: two handles of one operator differ in where their arrays lie,
and the cycle time of the control against the "fp64" leg measures that handle-to-handle spread in the same call.
Every shape is warmed up (graph capture, first touch), then the legs alternate within one call of this tool, three
repetitions each, all values kept:
  * ms per cycle (cedar_amd_solver_time_vcycles: HIP events around 5 replays of the captured cycle) with min_rows = n (the
    level-0 pair alone), then with min_rows stepped down one level at a time on fresh switched handles;
  * ms per level-0 restriction and interpolation-and-add (cedar_amd_solver_time_op ops 2 and 3, HIP events, 6 launches);
  * conjugate gradients to 1e-10 from x = 0 (pcg on V(1,1), fcg on V(2,1)): iterations and wall-clock ms.

The byte models (bytes per fine point, FP64 -> float weights) are written beside the measured ratios.

Decision written into the result ("default"), per dimension: the smallest fine-level size n such that at n and at every
larger measured size the switched cycle (level-0 pair alone) is not slower than the FP64 one beyond the spread -- the
larger of max - min of the repetitions of either leg and the distance between the medians of the two FP64 handles -- on
every workload of that dimension.  null: the default should switch nothing.
CI32_DEFAULT_MIN_ROWS_3D / _2D in solver.cpp are set by hand from this result.
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
BYTE_MODEL = {"restrict3": 22.0 / 35.0, "interp_add3": 54.0 / 67.0, "restrict2": 18.0 / 26.0, "interp_add2": 50.0 / 58.0,
              "restrict3_many": {str(n): (13.0 + 8 * n) / (26.0 + 8 * n) for n in NRHS},
              "interp_add3_many": {str(n): (13.0 + 41 * n) / (26.0 + 41 * n) for n in NRHS}}


def median(v):
    return sorted(v)[len(v) // 2]


def verdict(fp64, switched, control=None):
    """ratio of the medians, the spreads (control: a second FP64 handle; its distance from the first counts as spread),
    whether the switched leg wins by more than the spread, and whether it is not slower beyond it"""
    m0, m1 = median(fp64), median(switched)
    s0, s1 = max(fp64) - min(fp64), max(switched) - min(switched)
    out = {"ratio": m1 / m0, "gain_ms": m0 - m1, "spread_fp64_ms": s0, "spread_switched_ms": s1}
    spread = max(s0, s1)
    if control:
        out["control_ratio"] = median(control) / m0
        out["spread_handles_ms"] = abs(median(control) - m0)
        spread = max(spread, out["spread_handles_ms"], max(control) - min(control))
    out["faster"], out["not_slower"] = bool(m0 - m1 > spread), bool(m1 - m0 <= spread)
    return out


def alternate(legs, fn, warm):
    """fn(handle) -> ms: warm the legs up, then alternate them REPS times; {leg: [ms, ...]}"""
    for s in legs.values():
        warm(s)
    out = {k: [] for k in legs}
    for _ in range(REPS):
        for k, s in legs.items():
            out[k].append(fn(s))
    out["verdict"] = verdict(out["fp64"], out["switched"], out.get("control"))
    return out


def operator(capi, name, n):
    """(so, b) in HBM"""
    if name == "fe3":
        return capi.gallery("fe3", (n, n, n))
    if name == "poisson3":
        return capi.gallery("poisson3", (n, n, n))
    import problems as pb
    so, b = capi.DeviceArray((5, n + 2, n + 2)), capi.DeviceArray((n + 2, n + 2))
    so.upload(pb.varcoef9(n, n))
    b.upload(pb.rhs2(n, n))
    return so, b


def handle(capi, so, base, **kw):
    s = capi.Solver(so, share_operator=True, **kw)
    if base and getattr(s, base)(0) < 0:
        s.close()
        raise SystemExit("ci32_time: %s refused" % base)
    return s


def one(capi, n, so, b, cyc, base, depth, **kw):
    """one workload: FP64 weights against the level-0 pair switched, then one more level at a time"""
    g = tuple(b.shape)
    kw = dict(kw, **CYCLES[cyc])
    legs = {"fp64": handle(capi, so, base, **kw), "switched": handle(capi, so, base, **kw)}
    control = handle(capi, so, base, **kw)
    x = capi.DeviceArray(g)
    extra = [control]
    res = {"levels": [list(legs["fp64"].dims(l)) for l in range(legs["fp64"].nlevels())],
           "operator_levels_fp32": legs["fp64"].fp32_levels()}
    try:
        got = legs["switched"].use_fp32_interpolation(n)
        if got != 1 or legs["fp64"].fp32_interp_levels() != 0:
            raise SystemExit("ci32_time: the switch did not take the level-0 pair alone: %r" % got)
        x.zero()
        res["vcycle_ms"] = alternate(dict(legs, control=control), lambda s: s.time_vcycles(x, b, NCYC) / NCYC,
                                     lambda s: s.time_vcycles(x, b, 2))
        res["restrict0_ms"] = alternate(legs, lambda s: s.time_op(x, b, "restrict", NK) / NK, lambda s: s.time_op(x, b, "restrict", 2))
        res["interp_add0_ms"] = alternate(legs, lambda s: s.time_op(x, b, "interp_add", NK) / NK,
                                          lambda s: s.time_op(x, b, "interp_add", 2))
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
        # min_rows one level down at a time: fresh switched handles against the same FP64 leg; "step": against the handle
        # with one pair fewer
        res["by_min_rows"] = {}
        rows, prev = n, legs["switched"]
        for _ in range(depth):
            rows = (rows - 1) // 2 + 1
            if rows < 16:
                break
            s = handle(capi, so, base, **kw)
            extra.append(s)
            nl = s.use_fp32_interpolation(rows)
            x.zero()
            r = alternate({"fp64": legs["fp64"], "switched": s}, lambda h: h.time_vcycles(x, b, NCYC) / NCYC,
                          lambda h: h.time_vcycles(x, b, 2))
            r["step"] = alternate({"fp64": prev, "switched": s}, lambda h: h.time_vcycles(x, b, NCYC) / NCYC,
                                  lambda h: h.time_vcycles(x, b, 2))
            r["fp32_interp_levels"] = nl
            res["by_min_rows"][str(rows)] = r
            prev = s
    finally:
        for s in list(legs.values()) + extra:
            s.close()
        x.free()
    return res


def batch(capi, n):
    g = (n + 2, n + 2, n + 2)
    so, b = operator(capi, "fe3", n)
    kw = dict(max_rhs=max(NRHS), **CYCLES["v11"])
    legs = {"fp64": handle(capi, so, None, **kw), "switched": handle(capi, so, None, **kw)}
    bb, xx = capi.DeviceArray((max(NRHS),) + g), capi.DeviceArray((max(NRHS),) + g)
    for m in range(max(NRHS)):
        capi.lib.cedar_amd_memcpy_d2d(bb.ptr + m * b.size * 8, b.ptr, b.size * 8)

    class View:  # the first nrhs items of a DeviceArray
        def __init__(self, d, nrhs):
            self.ptr, self.shape = d.ptr, (nrhs,) + g

    res = {"n": n, "cycle": "v11", "operator": "fe3"}
    try:
        res["fp32_interp_levels"] = legs["switched"].use_fp32_interpolation(n)
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


def smallest_paying(wins):
    rows = None
    for n in sorted(wins, reverse=True):
        if not wins[n]:
            break
        rows = n
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes3", default="512,256,128")
    ap.add_argument("--size2-point", default="4096,2048,1024")
    ap.add_argument("--size2-lines", default="8192,2048")
    ap.add_argument("--depth", type=int, default=2, help="level pairs below the first that by_min_rows adds, one at a time")
    ap.add_argument("--batch-size", type=int, default=256, help="n of the batch handles (0: skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from cedar_amd import capi
    if capi.device_count() < 1:
        raise SystemExit("ci32_time: no GPU visible (there is no CPU fallback)")
    res = {"workload": "3D fe3 (27-point) and poisson3 (7-point level 0) n^3; 2D varcoef9 n^2, point and line-xy; V(1,1) and "
                       "V(2,1); on FP64 operators (fp64op) and on top of the operator switch (op32); two handles on one "
                       "operator, legs alternating; ms by HIP events, Krylov wall clock",
           "repetitions": REPS, "byte_model": BYTE_MODEL, "3d": {}, "2d": {}}

    def write():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            open(a.out, "w").write(json.dumps(res) + "\n")

    def run(dim, key, name, n, bases, **kw):
        so, b = operator(capi, name, n)
        try:
            r = {}
            for tag, base in bases:
                r[tag] = {cyc: one(capi, n, so, b, cyc, base, a.depth, **kw) for cyc in CYCLES}
            res[dim].setdefault(str(n), {})[key] = r
        finally:
            so.free()
            b.free()
        print("ci32_time: %s %d done" % (key, n), file=sys.stderr, flush=True)
        write()

    for n in [int(v) for v in a.sizes3.split(",") if v]:
        for name in ("fe3", "poisson3"):
            run("3d", name, name, n, (("fp64op", None), ("op32", "use_fp32_operator_all")))
    for n in [int(v) for v in a.size2_point.split(",") if v]:
        run("2d", "varcoef9-point", "varcoef9", n, (("fp64op", None), ("op32", "use_fp32_operator_2d")))
    for n in [int(v) for v in a.size2_lines.split(",") if v]:
        run("2d", "varcoef9-line-xy", "varcoef9", n, (("fp64op", None), ("op32", "use_fp32_operator_lines")), relax="line-xy")
    if a.batch_size:
        res["batch"] = batch(capi, a.batch_size)
        write()
    res["default"] = {"rule": "smallest fine-level size from which, at it and at every larger measured size, the switched "
                              "cycle (level-0 pair alone) is not slower than FP64 beyond the spread of either leg, on every "
                              "workload of the dimension; null: the default should switch nothing"}
    for dim in ("3d", "2d"):
        wins = {int(n): all(w[tag][c]["vcycle_ms"]["verdict"]["not_slower"] for w in r.values() for tag in w for c in CYCLES)
                for n, r in res[dim].items()}
        gains = {int(n): all(w[tag][c]["vcycle_ms"]["verdict"]["faster"] for w in r.values() for tag in w for c in CYCLES)
                 for n, r in res[dim].items()}
        res["default"][dim] = {"not_slower": {str(k): v for k, v in wins.items()}, "faster": {str(k): v for k, v in gains.items()},
                               "min_rows": smallest_paying(wins)}
    write()
    print(json.dumps(res["default"]))


if __name__ == "__main__":
    main()
