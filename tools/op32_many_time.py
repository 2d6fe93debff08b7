#!/usr/bin/env python3
"""What the single-precision 27-point operator is worth on a batch of right-hand sides
(cedar_amd_solver_use_fp32_operator_many).

    python tools/op32_many_time.py [--n 512] [--cycles 10] [--parent-root PARENT_CHECKOUT] [--out profiles/op32_many_time.json]
    python tools/op32_many_time.py --leg fp64 [--n 512] [--root CHECKOUT]   # the FP64 batched leg alone (what --parent-root runs)

Workload: 3D 27-point gallery::fe at n^3 (device gallery), V(2,1) point relaxation as in tools/many_time.py,
device-resident vectors, HIP-event time of `cycles` back-to-back batched cycles (cedar_amd_solver_time_vcycles_many), three
repetitions each, all values kept.  On ONE max_rhs = 8 handle in one process:
  * fp64_ms(nrhs) for nrhs in 1, 2, 4, 8, before the switch;
  * the switch level by level: min_rows = n (level 0 alone), then n/2, n/4, .., 1, all four nrhs timed after every step that
    added a level -- a switch is never undone, so the steps are cumulative and the difference of two neighbours is what the
    copy is worth on the level the step added;
  * with --parent-root: the fp64 leg of this tool on the package of another checkout (the commit before the feature, its
    library built), run as a child process on the same card with its own timeout -> parent_ms(nrhs), the baseline.
Reported: ratio(nrhs) = switched_ms(nrhs) / parent_ms(nrhs) (medians of three) at the step of the library's default
min_rows, and the same for every step.  Without --parent-root the baseline is this build's FP64 leg.
CEDAR_AMD_OP32_MIN_ROWS is not set here: every call passes its min_rows.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST = dict(nrelax_pre=2, nrelax_post=1)
NRHS = (1, 2, 4, 8)
DEFAULT_MIN_ROWS = 128  # solver.cpp OP32_DEFAULT_MIN_ROWS


def reps(fn, cycles, n=3):
    fn(2)  # records the graph
    return [fn(cycles) / cycles for _ in range(n)]


def median(v):
    return sorted(v)[len(v) // 2]


def spread(v):
    return (max(v) - min(v)) / median(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--cycles", type=int, default=10)
    ap.add_argument("--leg", choices=["all", "fp64"], default="all")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--parent-timeout", type=int, default=400, help="seconds the parent's child process may take")
    ap.add_argument("--root", default=ROOT, help="the checkout whose cedar_amd package is timed (default: this one)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    from cedar_amd import capi
    if capi.device_count() < 1:
        raise SystemExit("op32_many_time: no GPU visible (there is no CPU fallback)")
    n = a.n
    g = (n + 2,) * 3
    so, b = capi.gallery("fe3", (n, n, n))
    s = capi.Solver(so, share_operator=True, max_rhs=max(NRHS), **ST)
    bb, xx = capi.DeviceArray((max(NRHS),) + g), capi.DeviceArray((max(NRHS),) + g)
    for m in range(max(NRHS)):
        capi.lib.cedar_amd_memcpy_d2d(bb.ptr + m * b.size * 8, b.ptr, b.size * 8)

    class View:  # the first nrhs items of a DeviceArray
        def __init__(self, d, nrhs):
            self.ptr, self.shape = d.ptr, (nrhs,) + g

    def timed_all():
        out = {}
        for k in NRHS:
            xx.zero()
            out[str(k)] = reps(lambda c: s.time_vcycles_many(View(xx, k), View(bb, k), c), a.cycles)
        return out

    res = {"workload": f"3d27 fe {n}^3 V(2,1), batched cycle on one max_rhs = 8 handle; ms per cycle by HIP events",
           "cycles_per_repetition": a.cycles, "levels": [list(s.dims(l)) for l in range(s.nlevels())]}
    try:
        res["fp64_ms"] = timed_all()
        if a.leg == "fp64":
            print(json.dumps({"fp64_ms": res["fp64_ms"]}))
            return
        steps, m = [], n
        while m >= 1:
            levels = s.use_fp32_operator_many(m)
            if levels < 0:
                raise SystemExit("op32_many_time: the switch was refused")
            if not steps or levels != steps[-1]["fp32_levels"]:
                steps.append({"min_rows": m, "fp32_levels": levels, "ms": timed_all()})
                print("op32_many_time: min_rows %d done" % m, file=sys.stderr, flush=True)
            m = 1 if 1 < m < 16 else m // 2
        res["fp32_steps"] = steps
    finally:
        s.close()
        bb.free()
        xx.free()
    base = res["fp64_ms"]
    if a.parent_root:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "fp64", "--n", str(n), "--cycles", str(a.cycles),
                              "--root", a.parent_root], check=True, capture_output=True, text=True, timeout=a.parent_timeout).stdout
        res["parent_ms"] = base = json.loads(out.strip().splitlines()[-1])["fp64_ms"]
    res["baseline"] = "parent_ms" if a.parent_root else "fp64_ms"
    for st in steps:
        st["ratio"] = {k: median(v) / median(base[k]) for k, v in st["ms"].items()}
    # the step the library's default takes: the last one whose min_rows is not below the default
    dflt = [st for st in steps if st["min_rows"] >= DEFAULT_MIN_ROWS]
    if dflt:
        d = dflt[-1]
        res["default_min_rows"] = DEFAULT_MIN_ROWS
        res["ratio"] = d["ratio"]
        res["spread"] = {k: {"switched": spread(d["ms"][k]), "baseline": spread(base[k])} for k in d["ms"]}
        r4 = d["ratio"]["4"]
        res["break_even_at_4"] = bool(r4 < 1 and max(res["spread"]["4"].values()) < 1 - r4)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
