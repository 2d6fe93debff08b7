#!/usr/bin/env python3
"""Cycle time of several right-hand sides on one resident hierarchy (cedar_amd_solver_time_vcycles_many).

    python tools/many_time.py [--n 512] [--cycles 10] [--parent-root PARENT_CHECKOUT] [--out profiles/many_time.json]
    python tools/many_time.py --leg single [--n 512]      # the single-vector leg alone (what --parent-root runs)
    python tools/many_time.py --leg many4 [--n 512]       # a few nrhs = 4 cycles (the run to trace with rocprofv3)

Workload: 3D 27-point gallery::fe at n^3 (device gallery), V(2,1) point relaxation, device-resident vectors, HIP-event
time of `cycles` back-to-back cycles, three repetitions each, all values kept:
  * ms(nrhs) for nrhs in 1, 2, 4, 8 on a max_rhs = 8 handle;
  * the single-vector cycle (cedar_amd_solver_time_vcycles) on a plain handle in the same process;
  * with --parent-root: the single-vector leg of this tool on the package of another checkout (the commit before the
    feature, its library built), run as a child process on the same card -> parent_single_ms, the baseline of
    per_rhs_ratio(nrhs) = ms(nrhs) / (nrhs * parent_single_ms).  Without it the baseline is this build's single-vector cycle.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ST = dict(nrelax_pre=2, nrelax_post=1)


def free_bytes():
    try:
        hip = ctypes.CDLL("libamdhip64.so")
        fr, tot = ctypes.c_size_t(), ctypes.c_size_t()
        if hip.hipMemGetInfo(ctypes.byref(fr), ctypes.byref(tot)) == 0:
            return fr.value
    except OSError:
        pass
    return None


def reps(fn, cycles, n=3):
    fn(2)  # records the graph
    return [fn(cycles) / cycles for _ in range(n)]


def single_leg(capi, so, b, g, cycles):
    s = capi.Solver(so, share_operator=True, **ST)
    x = capi.DeviceArray(g)
    x.zero()
    try:
        return reps(lambda k: s.time_vcycles(x, b, k), cycles)
    finally:
        s.close()
        x.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--cycles", type=int, default=10)
    ap.add_argument("--leg", choices=["all", "single", "many4"], default="all")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--root", default=ROOT, help="the checkout whose cedar_amd package is timed (default: this one)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    from cedar_amd import capi
    if capi.device_count() < 1:
        raise SystemExit("many_time: no GPU visible (there is no CPU fallback)")
    n = a.n
    g = (n + 2,) * 3
    so, b = capi.gallery("fe3", (n, n, n))
    if a.leg == "single":
        print(json.dumps({"single_ms": single_leg(capi, so, b, g, a.cycles)}))
        return
    res = {"workload": f"3d27 fe {n}^3 V(2,1)", "cycles_per_repetition": a.cycles}
    f0 = free_bytes()
    s = capi.Solver(so, share_operator=True, max_rhs=8, **ST)
    f1 = free_bytes()
    if f0 is not None and f1 is not None:
        res["handle_max_rhs8_GiB"] = (f0 - f1) / 2.0 ** 30  # without the operator (shared) and the caller's x, b
    bb, xx = capi.DeviceArray((8,) + g), capi.DeviceArray((8,) + g)
    for m in range(8):
        capi.lib.cedar_amd_memcpy_d2d(bb.ptr + m * b.size * 8, b.ptr, b.size * 8)
    xx.zero()

    class View:  # the first nrhs items of a DeviceArray
        def __init__(self, d, nrhs):
            self.ptr, self.shape = d.ptr, (nrhs,) + g

    try:
        if a.leg == "many4":
            print(json.dumps({"many4_ms": s.time_vcycles_many(View(xx, 4), View(bb, 4), 3) / 3}))
            return
        res["many_ms"] = {str(k): reps(lambda c: s.time_vcycles_many(View(xx, k), View(bb, k), c), a.cycles) for k in (1, 2, 4, 8)}
    finally:
        s.close()
        bb.free()
        xx.free()
    res["single_ms"] = single_leg(capi, so, b, g, a.cycles)
    base = res["single_ms"]
    if a.parent_root:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "single", "--n", str(n), "--cycles", str(a.cycles),
                              "--root", a.parent_root], check=True, capture_output=True, text=True, timeout=600).stdout
        res["parent_single_ms"] = base = json.loads(out.strip().splitlines()[-1])["single_ms"]
    ref = sorted(base)[1]  # median of the three repetitions
    res["baseline"] = "parent_single_ms" if a.parent_root else "single_ms"
    res["per_rhs_ratio"] = {k: [v / (int(k) * ref) for v in vs] for k, vs in res["many_ms"].items()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
