#!/usr/bin/env python3
"""Iteration time of conjugate gradients on several right-hand sides at once (cedar_amd_solver_pcg_many).

    python tools/pcg_many_time.py [--n 512] [--parent-root PARENT_CHECKOUT] [--out profiles/pcg_many_time.json]
    python tools/pcg_many_time.py --leg single [--n 512]   # the single-vector leg alone (what --parent-root runs)
    python tools/pcg_many_time.py --leg many4 [--n 512]    # a few nrhs = 4 iterations (the run to trace with rocprofv3)

Workload: 3D 27-point gallery::fe at n^3 (device gallery), V(1,1) point relaxation, device-resident vectors, tol = 0 so
that every run does exactly max_iter iterations.  ms per iteration = (t(N2) - t(N1)) / (N2 - N1) of two wall-clock
timed runs (set-up, first residual and storage drop out), as tools/pcg_time.py does; three repetitions, all kept:
  * ms(nrhs) for nrhs in 1, 2, 4, 8 on a max_rhs = 8 handle (max_rhs = 4 with a note when the card has too little free
    memory: 5 vectors per item of Krylov storage beside the hierarchy's own batch vectors);
  * with --parent-root: cedar_amd_solver_pcg of another checkout (the commit before the feature, its library built), run
    as a child process on the same card -> parent_ms, the baseline of per_rhs_ratio(nrhs) = ms(nrhs) / (nrhs * parent_ms):
    what a caller would otherwise run nrhs times, partial-sum sweeps included.  Without it the baseline is this build's
    cedar_amd_solver_pcg.
Next to the measured ratios: the byte model of the direction pass on the row-interleaved copy, (120 + 32 n) / (152 n).
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ST = dict(nrelax_pre=1, nrelax_post=1)
N1, N2 = 3, 9


def free_bytes():
    try:
        hip = ctypes.CDLL("libamdhip64.so")
        fr, tot = ctypes.c_size_t(), ctypes.c_size_t()
        if hip.hipMemGetInfo(ctypes.byref(fr), ctypes.byref(tot)) == 0:
            return fr.value
    except OSError:
        pass
    return None


def per_iteration(capi, run, reps=3):
    """run(max_iter) solves from x = 0 with tol = 0; ms per iteration from the difference of two run lengths"""
    run(2)  # storage, captured cycles
    out = []
    for _ in range(reps):
        t = []
        for k in (N1, N2):
            capi.sync()
            t0 = time.perf_counter()
            run(k)
            capi.sync()
            t.append(time.perf_counter() - t0)
        out.append(1e3 * (t[1] - t[0]) / (N2 - N1))
    return out


def single_leg(capi, so, b, g):
    s = capi.Solver(so, share_operator=True, **ST)
    x = capi.DeviceArray(g)

    def run(k):
        x.zero()
        assert len(s.pcg(b, x, max_iter=k, tol=0.0)) == k + 1

    try:
        return per_iteration(capi, run)
    finally:
        s.close()
        x.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--leg", choices=["all", "single", "many4"], default="all")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--root", default=ROOT, help="the checkout whose cedar_amd package is timed (default: this one)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    from cedar_amd import capi
    if capi.device_count() < 1:
        raise SystemExit("pcg_many_time: no GPU visible (there is no CPU fallback)")
    n = a.n
    g = (n + 2,) * 3
    so, b = capi.gallery("fe3", (n, n, n))
    if a.leg == "single":
        print(json.dumps({"single_ms": single_leg(capi, so, b, g)}))
        return
    res = {"workload": f"3d27 fe {n}^3 V(1,1) pcg precon=mg tol=0", "iterations": [N1, N2]}
    # per item about twelve level-0 vectors: the hierarchy's batch vectors (~5), the Krylov storage (5), the caller's x and b
    item = 8 * (n + 2) ** 3
    cap = 8 if a.leg == "all" else 4
    fr = free_bytes()
    if fr is not None and fr < cap * item * 12:
        res["note"] = f"max_rhs dropped from {cap} to 4: {fr / 2.0 ** 30:.0f} GiB free"
        cap = 4
    res["max_rhs"] = cap
    f0 = free_bytes()
    s = capi.Solver(so, share_operator=True, max_rhs=cap, **ST)
    bb, xx = capi.DeviceArray((cap,) + g), capi.DeviceArray((cap,) + g)
    for m in range(cap):
        capi.lib.cedar_amd_memcpy_d2d(bb.ptr + m * b.size * 8, b.ptr, b.size * 8)

    class View:  # the first nrhs items of a DeviceArray
        def __init__(self, d, nrhs):
            self.ptr, self.shape = d.ptr, (nrhs,) + g

        def data_ptr(self):  # the pointer protocol of the handle API's front end
            return self.ptr

    def run_many(nrhs):
        def run(k):
            xx.zero()
            hist, iters = s.pcg_many(View(bb, nrhs), View(xx, nrhs), max_iter=k, tol=0.0)
            assert iters == [k] * nrhs, iters
        return run

    try:
        if a.leg == "many4":
            run_many(4)(2)
            run_many(4)(3)
            print(json.dumps({"many4": "2 + 3 iterations run"}))
            return
        res["many_ms"] = {}
        for k in (1, 2, 4, 8):
            if k <= cap:
                res["many_ms"][str(k)] = per_iteration(capi, run_many(k))
        f1 = free_bytes()
        if f0 is not None and f1 is not None:
            res["handle_and_vectors_GiB"] = (f0 - f1) / 2.0 ** 30  # hierarchy batch vectors, Krylov storage, x, b
    finally:
        s.close()
        bb.free()
        xx.free()
    res["single_ms"] = single_leg(capi, so, b, g)
    base = res["single_ms"]
    if a.parent_root:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "single", "--n", str(n), "--root", a.parent_root],
                             check=True, capture_output=True, text=True, timeout=600).stdout
        res["parent_ms"] = base = json.loads(out.strip().splitlines()[-1])["single_ms"]
    ref = sorted(base)[1]  # median of the three repetitions
    res["baseline"] = "parent_ms" if a.parent_root else "single_ms"
    res["per_rhs_ratio"] = {k: [v / (int(k) * ref) for v in vs] for k, vs in res["many_ms"].items()}
    res["direction_byte_model_ratio"] = {k: (120 + 32 * int(k)) / (152.0 * int(k)) for k in res["many_ms"]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
