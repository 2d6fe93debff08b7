"""The C++ mirror under include/cedar on the GPU, beyond tests/test_cxx_api.py:

1. every registered "hip" kernel as a single call through kman->setup<T> / kman->run<T> with the mirror's own types
   (tests/cxx/registry_server.cc): the kernel suites of tests/cases.py run through the registry, bit for bit against
   the direct C-ABI call (cedar_amd.capi.Kernels; a binding may add nothing -- no kernel of the library uses atomics,
   all are run-to-run deterministic), against the oracle and against the reference's goldens with the tolerances the
   C-ABI tests use for the same keys;
2. the orchestrated driver of include/cedar/multilevel.h (tests/cxx/orchestrated.cc): line smoothers, F-cycles,
   solver.num-levels, periodic grids, plane relaxation with a plane-config block, vcycle() off the resident path,
   against the oracle and against the resident solver, hierarchy included;
3. every abstract kernel class dispatches to a user's implementation, counted call by call;
4. a resident solve, a read of `levels`, then an orchestrated solve (multilevel::ready builds the smoothers and the
   coarse solver although the host arrays already exist).
"""
import json
import os
import select
import subprocess
import time

import numpy as np
import pytest

import cases
import problems as pb
import test_gpu_kernels as tgk
from test_oracle_periodic import check_kernels
from test_oracle_periodic3d import check_kernels3
from test_oracle_planes import DOWN, UP, varying_op

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FLAGS = ["-std=c++17", "-O1", "-Wall", f"-I{ROOT}/include", f"-L{ROOT}/cedar_amd/lib", "-lcedar_amd", "-L/opt/rocm/lib",
         f"-Wl,-rpath,{ROOT}/cedar_amd/lib", "-Wl,-rpath,/opt/rocm/lib"]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """both programs, built and linked against the headers and the library (no GPU needed for that)"""
    from cedar_amd import capi  # noqa: F401  (builds libcedar_amd.so if missing)
    d = tmp_path_factory.mktemp("cxx_registry")
    out = {}
    for name in ("registry_server", "orchestrated"):
        out[name] = str(d / name)
        subprocess.run(["g++", os.path.join(HERE, "cxx", name + ".cc")] + FLAGS + ["-o", out[name]], check=True)
    return out


def test_registry_programs_compile_and_link(programs, tmp_path):
    """tests/cxx/registry_server.cc and orchestrated.cc build here without a GPU; the server's request parser answers
    what needs no device: a request before any manager, an unknown request, a file of the wrong length"""
    for exe in programs.values():
        assert os.access(exe, os.X_OK)
    (tmp_path / "short.bin").write_bytes(b"\0" * 8)
    p = subprocess.run([programs["registry_server"]], input="residual 5 4 4 a b c d\nmanager 2 0\nnothing 5 4 4\n"
                       f"setup_recip 5 4 4 {tmp_path}/short.bin {tmp_path}/short.bin\nmanager 4 0\nquit\n",
                       capture_output=True, text=True, timeout=60, check=True)
    got = p.stdout.splitlines()
    assert got[0] == "error no manager yet" and got[1] == "ok" and got[2] == "error no request nothing"
    assert got[3].startswith("error ") and "does not hold 180 doubles" in got[3] and got[4] == "error dim must be 2 or 3"


# ---------------------------------------------------------------------------------------------------------------
# 1. the registry behind pyoracle's method names
# ---------------------------------------------------------------------------------------------------------------
MASK2 = {0: 0, 1: 2, 2: 1, 3: 3}  # boundary code of BMG_get_bc -> kernel_params::per_mask (bit 0 x, bit 1 y, bit 2 z)
MASK3 = {0: 0, 1: 2, 2: 1, 3: 3, 5: 4, 6: 5, 7: 6, 8: 7}
TROUBLE = []  # a child that died, hung or answered with an error: nothing more is started on the GPU by this module
PLANE_KEYS = (("relax", "solver.relaxation", "line-xy"), ("nrelax_pre", "solver.cycle.nrelax-pre", 2),
              ("nrelax_post", "solver.cycle.nrelax-post", 1), ("max_iter", "solver.max-iter", 1),
              ("min_coarse", "solver.min_coarse", 3), ("tol", "solver.tol", 1e-8))


class Registry:
    """pyoracle's method names over one registry_server process: every call writes its arrays to files, sends one request
    and reads the arrays the kernel writes back.  Every request has a deadline; a missed deadline, a dead server or an
    error answer fails the call and every later one -- the server is never restarted."""
    FIRST, EACH, GROUP = 60.0, 10.0, 120.0  # seconds: the request that initialises the device, any other, one group

    def __init__(self, exe, tmp):
        self.tmp = str(tmp)
        self.proc = subprocess.Popen([exe], stdin=subprocess.PIPE, stdout=subprocess.PIPE, bufsize=0)
        self.dead = None
        self.state = None
        self.first = True
        self.spent = {}
        self.group = "none"
        self.nfile = 0

    def close(self):
        if self.proc.poll() is None:
            try:
                self.proc.stdin.write(b"quit\n")
                self.proc.stdin.close()
                self.proc.wait(timeout=10)
            except Exception:
                self.proc.kill()
                self.proc.wait()

    def _fail(self, why):
        self.dead = why
        TROUBLE.append(why)
        if self.proc.poll() is None:
            self.proc.kill()
            self.proc.wait()
        raise RuntimeError(why)

    def _request(self, *words, gpu=True):
        if self.dead or TROUBLE:
            raise RuntimeError("registry server is gone: " + (self.dead or TROUBLE[0]))
        line = " ".join(str(w) for w in words)
        left = self.GROUP - self.spent.get(self.group, 0.0)
        limit = min(self.FIRST if (gpu and self.first) else self.EACH, left)
        if limit <= 0:
            self._fail(f"group {self.group} used up its {self.GROUP} s before: {line}")
        if gpu:
            self.first = False
        t0 = time.monotonic()
        try:
            self.proc.stdin.write(line.encode() + b"\n")
        except OSError:
            self._fail(f"server died (exit {self.proc.poll()}) before: {line}")
        buf = b""
        while not buf.endswith(b"\n"):
            wait = limit - (time.monotonic() - t0)
            if wait <= 0 or not select.select([self.proc.stdout], [], [], wait)[0]:
                self._fail(f"no answer within {limit:.0f} s to: {line}")
            chunk = os.read(self.proc.stdout.fileno(), 4096)
            if not chunk:
                self.proc.wait()
                self._fail(f"server died (exit {self.proc.returncode}) on: {line}")
            buf += chunk
        self.spent[self.group] = self.spent.get(self.group, 0.0) + time.monotonic() - t0
        if buf.strip() != b"ok":
            self._fail(f"{buf.decode().strip()!r} to: {line}")

    def _manager(self, dim, mask=None, plane="keep"):
        """mask None / plane 'keep': whatever the manager of that dimension has"""
        cur = self.state if self.state and self.state[0] == dim else None
        mask = (cur[1] if cur else 0) if mask is None else mask
        if isinstance(plane, str):
            key = cur[2] if cur else None
        else:
            key = None if plane is None else tuple(f"{k}={plane.get(p, dflt)}" for p, k, dflt in PLANE_KEYS)
        if (dim, mask, key) != self.state:
            self._request("manager", dim, mask, *(key or ()), gpu=False)
            self.state = (dim, mask, key)

    def _call(self, words, arrays, written):
        """arrays go out as files in the order given (their names end the request); those in `written` are read back"""
        paths = []
        for a in arrays:
            assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
            self.nfile += 1
            paths.append(os.path.join(self.tmp, f"a{self.nfile}.bin"))
            a.tofile(paths[-1])
        self._request(*words, *paths)
        for a, p in zip(arrays, paths):
            if any(a is w for w in written):
                a[...] = np.fromfile(p, dtype=np.float64).reshape(a.shape)
            os.remove(p)

    @staticmethod
    def _n(shape_g):
        return [m - 2 for m in shape_g[::-1]]

    # ---- 2D
    def setup_recip2(self, so, sor):
        self._manager(2)
        self._call(["setup_recip", so.shape[0]] + self._n(so.shape[1:]), [so, sor], [sor])

    def relax2(self, so, qf, q, sor, updown, ibc=0):
        self._manager(2, MASK2[ibc])
        self._call(["relax", so.shape[0]] + self._n(so.shape[1:]) + [updown], [so, qf, q, sor], [q])

    def setup_lines2(self, so, sor, d, ibc=0):
        self._manager(2, MASK2[ibc])
        self._call(["setup_lines", d, so.shape[0]] + self._n(so.shape[1:]), [so, sor], [sor])

    def relax_lines2(self, so, qf, q, sor, updown, d, ibc=0):
        self._manager(2, MASK2[ibc])
        self._call(["relax_lines", d, so.shape[0]] + self._n(so.shape[1:]) + [updown], [so, qf, q, sor], [q])

    def residual2(self, so, qf, q, res):
        self._manager(2, 0)
        self._call(["residual", so.shape[0]] + self._n(so.shape[1:]), [so, qf, q, res], [res])

    def restrict2(self, q, qc, ci, ibc=0):
        self._manager(2, MASK2[ibc])
        self._call(["restrict"] + self._n(q.shape) + self._n(qc.shape), [q, qc, ci], [qc, q])

    def interp_add2(self, q, qc, res, so, ci, ibc=0):
        self._manager(2, MASK2[ibc])
        self._call(["interp_add", so.shape[0]] + self._n(q.shape) + self._n(qc.shape), [q, qc, res, so, ci], [q, res])

    def setup_interp2(self, so, ci, ibc=0):
        self._manager(2, MASK2[ibc])
        self._call(["setup_interp", so.shape[0]] + self._n(so.shape[1:]) + self._n(ci.shape[1:]), [so, ci], [ci])

    def galerkin2(self, so, soc, ci, ibc=0):
        self._manager(2, MASK2[ibc])
        self._call(["galerkin", so.shape[0]] + self._n(so.shape[1:]) + self._n(ci.shape[1:]), [so, soc, ci], [soc])

    def setup_cg2(self, so, abd, ibc=0):
        self._manager(2, MASK2[ibc])
        self._call(["setup_cg", so.shape[0]] + self._n(so.shape[1:]) + [abd.shape[1], abd.shape[0]], [so, abd], [abd])

    def solve_cg2(self, q, qf, abd, ibc=0):
        self._manager(2, MASK2[ibc])
        self._call(["solve_cg"] + self._n(q.shape) + [abd.shape[1], abd.shape[0]], [q, qf, abd], [q])

    # ---- 3D
    def setup_recip3(self, so, sor):
        self._manager(3)
        self._call(["setup_recip", so.shape[0]] + self._n(so.shape[1:]), [so, sor], [sor])

    def relax3(self, so, qf, q, sor, updown, ibc=0):
        self._manager(3, MASK3[ibc])
        self._call(["relax", so.shape[0]] + self._n(so.shape[1:]) + [updown], [so, qf, q, sor], [q])

    def residual3(self, so, qf, q, res):
        self._manager(3, 0)
        self._call(["residual", so.shape[0]] + self._n(so.shape[1:]), [so, qf, q, res], [res])

    def restrict3(self, q, qc, ci, ibc=0):
        self._manager(3, MASK3[ibc])
        self._call(["restrict"] + self._n(q.shape) + self._n(qc.shape), [q, qc, ci], [qc, q])

    def interp_add3(self, q, qc, so, res, ci, ibc=0):
        self._manager(3, MASK3[ibc])
        self._call(["interp_add", so.shape[0]] + self._n(q.shape) + self._n(qc.shape), [q, qc, res, so, ci], [q, res])

    def setup_interp3(self, so, ci, ibc=0):
        self._manager(3, MASK3[ibc])
        self._call(["setup_interp", so.shape[0]] + self._n(so.shape[1:]) + self._n(ci.shape[1:]), [so, ci], [ci])

    def galerkin3(self, so, soc, ci, ibc=0):
        self._manager(3, MASK3[ibc])
        self._call(["galerkin", so.shape[0]] + self._n(so.shape[1:]) + self._n(ci.shape[1:]), [so, soc, ci], [soc])

    def setup_cg3(self, so, abd, ibc=0):
        self._manager(3, MASK3[ibc])
        self._call(["setup_cg", so.shape[0]] + self._n(so.shape[1:]) + [abd.shape[1], abd.shape[0]], [so, abd], [abd])

    def solve_cg3(self, q, qf, abd, ibc=0):
        self._manager(3, MASK3[ibc])
        self._call(["solve_cg"] + self._n(q.shape) + [abd.shape[1], abd.shape[0]], [q, qf, abd], [q])

    def relax_planes3(self, so, x, b, d, updown, plane=None, nsetup=1):
        """kman->setup<plane_relax<d>>(so), nsetup times; kman->run<plane_relax<d>>(so, x, b, updown); the plane
        settings reach the binding through the plane-config block of the manager's parameters"""
        self._manager(3, 0, plane)
        self._call(["planes", d, so.shape[0]] + self._n(so.shape[1:]) + [updown, nsetup], [so, x, b], [x])


@pytest.fixture(scope="module")
def K():
    from cedar_amd import capi
    assert capi.device_count() >= 1, "no GPU visible"
    return capi.Kernels()


@pytest.fixture(scope="module")
def R(programs, tmp_path_factory):
    r = Registry(programs["registry_server"], tmp_path_factory.mktemp("registry_files"))
    yield r
    r.close()


@pytest.fixture(scope="module")
def gper():
    return {2: np.load(os.path.join(HERE, "golden", "periodic2d.npz")), 3: np.load(os.path.join(HERE, "golden", "periodic3d.npz"))}


class _Gold(dict):
    """the oracle's outputs under the keys of a golden file, for the check helpers that take one"""
    @property
    def files(self):
        return list(self)


def _pick(table, names):
    by = {c[0]: c for c in table}
    return [by[n] for n in names]


REG_2D = _pick(cases.CASES_2D, ["r16x12_5", "r7x10_9", "r37x37_5", "r31x31_9"])
REG_3D = _pick(cases.CASES_3D, ["r8x6x10_7", "r12x7x9_27", "r13x13x13_27"])
REG_PER = _pick(cases.CASES_PER, ["p12x17_5_xy", "p17x12_9_x", "p31x20_9_y"])
REG_CG_PER = _pick(cases.CG_PER, ["c4x3_9_y", "c5x4_5_xy"])
REG_PER3 = _pick(cases.CASES_PER3, ["q8x9x11_27_x", "q6x4x8_27_xy", "q8x10x12_27_yz", "q4x4x4_7_xyz"])
REG_CG_PER3 = _pick(cases.CG_PER3, ["d3x4x4_z", "d4x4x3_xy"])


def _bit_equal(name, got, direct):
    assert set(got) == set(direct)
    for k in got:
        assert np.array_equal(got[k], direct[k]), f"{name}/{k}: the binding changes the C-ABI call's result, max diff {np.max(np.abs(got[k] - direct[k]))}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", REG_2D, ids=lambda c: c[0])
def test_registry_kernels_2d(R, K, oracle, golden, case):
    R.group = "2d"
    got, direct, want = (cases.kernel_suite_2d(impl, case) for impl in (R, K, oracle))
    _bit_equal(case[0], got, direct)
    assert set(got) == set(want) and ("solve_cg" in got) == (case[1] * case[2] <= 200)
    for k, v in got.items():
        tgk.check(f"{case[0]}/{k}", v, want[k])
        tgk.check(f"{case[0]}/{k}", v, golden["k2"][f"{case[0]}/{k}"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", REG_3D, ids=lambda c: c[0])
def test_registry_kernels_3d(R, K, oracle, golden, case):
    R.group = "3d"
    got, direct, want = (cases.kernel_suite_3d(impl, case) for impl in (R, K, oracle))
    _bit_equal(case[0], got, direct)
    assert set(got) == set(want) and ("solve_cg" in got) == (case[1] * case[2] * case[3] <= 500)
    for k, v in got.items():
        tgk.check(f"{case[0]}/{k}", v, want[k])
        tgk.check(f"{case[0]}/{k}", v, golden["k3"][f"{case[0]}/{k}"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", REG_PER + REG_CG_PER, ids=lambda c: c[0])
def test_registry_kernels_2d_periodic(R, K, oracle, gper, case):
    """grid.periodic through the registry: every binding turns per_mask into the boundary code itself"""
    R.group = "2d periodic"
    suite = cases.coarse_solve_per if case in REG_CG_PER else cases.kernel_suite_per
    got, direct, want = (suite(impl, case) for impl in (R, K, oracle))
    _bit_equal(case[0], got, direct)
    check_kernels(case[0], got, _Gold({f"{case[0]}/{k}": v for k, v in want.items()}))
    check_kernels(case[0], got, gper[2])


@pytest.mark.gpu
@pytest.mark.parametrize("case", REG_PER3 + REG_CG_PER3, ids=lambda c: c[0])
def test_registry_kernels_3d_periodic(R, K, oracle, gper, case):
    R.group = "3d periodic"
    suite = cases.coarse_solve_per3 if case in REG_CG_PER3 else cases.kernel_suite_per3
    got, direct, want = (suite(impl, case) for impl in (R, K, oracle))
    _bit_equal(case[0], got, direct)
    check_kernels3(case[0], got, _Gold({f"{case[0]}/{k}": v for k, v in want.items()}))
    check_kernels3(case[0], got, gper[3])


@pytest.mark.gpu
@pytest.mark.parametrize("d", ["xy", "xz", "yz"])
@pytest.mark.parametrize("nst", [4, 14])
@pytest.mark.parametrize("plane", [None, dict(relax="line-x", max_iter=2, tol=0.5)], ids=["default", "linex-tol"])
def test_registry_plane_relaxation(R, K, oracle, d, nst, plane):
    """plane_relax<xy|xz|yz> through the registry, the plane settings through a plane-config block: DOWN then UP on
    plane-dependent coefficients, 1e-11 against the oracle as in tests/test_gpu_planes.py and bit for bit like
    cedar_amd_planes_* called directly.  Every call sets the planes up again on an operator of the same shape, which
    replaces sets[key]; one case also calls setup twice before one run."""
    R.group = "planes"
    so = varying_op(21, 18, 15, nst, 31)
    b = pb.uniform(so.shape[1:], 33, -1, 1)
    x1 = pb.uniform(so.shape[1:], 32, -1, 1)
    x2, x3 = x1.copy(), x1.copy()
    twice = d == "xz" and nst == 14 and plane is None
    for ud in (DOWN, UP):
        R.relax_planes3(so, x1, b, d, ud, plane=plane, nsetup=2 if (twice and ud == UP) else 1)
        oracle.relax_planes3(so, x2, b, d, ud, plane=plane)
        K.relax_planes3(so, x3, b, d, ud, plane=plane)
        assert np.max(np.abs(x1 - x2)) <= 1e-11 * np.max(np.abs(x2)), (d, nst, ud, np.max(np.abs(x1 - x2)))
        assert np.array_equal(x1, x3), (d, nst, ud, np.max(np.abs(x1 - x3)))


# ---------------------------------------------------------------------------------------------------------------
# 2. - 4. the orchestrated driver
# ---------------------------------------------------------------------------------------------------------------
def _config(st, per, test):
    solver = {"relaxation": st.get("relax", "point"), "max-iter": cases.ORCHESTRATED_MAXITER,
              "cycle": {"nrelax-pre": st.get("nrelax_pre", 2), "nrelax-post": st.get("nrelax_post", 1), "type": st.get("cycle", "v")}}
    if "num_levels" in st:
        solver["num-levels"] = st["num_levels"]
    cfg = {"solver": solver, "test": test}
    if per:
        cfg["grid"] = {"periodic": [bool(p) for p in per]}
    if st.get("plane"):
        pl = {p: st["plane"].get(p, dflt) for p, _, dflt in PLANE_KEYS}
        cfg["plane-config"] = {"solver": {"relaxation": pl["relax"], "max-iter": pl["max_iter"], "min_coarse": pl["min_coarse"], "tol": pl["tol"],
                                          "cycle": {"nrelax-pre": pl["nrelax_pre"], "nrelax-post": pl["nrelax_post"]}}}
    return cfg


def _orchestrated(exe, d, so, b, st, per, mode, x0=None):
    """one process, 60 s; a non-zero exit, a signal or the time limit fails the test and every later one of the module"""
    assert not TROUBLE, f"not started after: {TROUBLE[0]}"
    so.tofile(d / "so.bin")
    b.tofile(d / "b.bin")
    if x0 is not None:
        x0.tofile(d / "x0.bin")
    test = {"mode": mode, "dim": so.ndim - 1, "n": [m - 2 for m in so.shape[:0:-1]], "nst": so.shape[0], "vcycle": int(x0 is not None)}
    json.dump(_config(st, per, test), open(d / "config.json", "w"))
    try:
        p = subprocess.run([exe, str(d)], capture_output=True, text=True, timeout=60)
    except subprocess.TimeoutExpired:
        TROUBLE.append(f"orchestrated ({mode}) did not end within 60 s")
        raise
    if p.returncode != 0:
        TROUBLE.append(f"orchestrated ({mode}) ended with {p.returncode}")
    assert p.returncode == 0, (p.returncode, p.stdout[-400:], p.stderr[-400:])
    return json.loads(p.stdout.strip().splitlines()[-1])


def _hist_tol(st):
    relax = st.get("relax", "point")
    if relax.startswith("plane"):
        return dict(rtol=1e-8, atol=1e-13)
    return dict(rtol=1e-10, atol=1e-12 if relax.startswith("line") else 1e-14)


def _vs_oracle(name, st, h, x, ho, xo):
    """history and x as tests/test_gpu_solver.py (cases.HIST_ATOL where lines are solved) and tests/test_gpu_planes.py
    hold the resident solver to the oracle"""
    print(name, "max |h - ho| / ho", np.max(np.abs(np.array(h) - ho) / ho) if len(h) == len(ho) else "length", "max |x - xo| / max |xo|",
          np.max(np.abs(x - xo)) / np.max(np.abs(xo)))
    assert len(h) == len(ho), (name, h, ho)
    np.testing.assert_allclose(h, ho, err_msg=name, **_hist_tol(st))
    if st.get("relax", "point").startswith("plane"):
        assert np.max(np.abs(x - xo)) <= 1e-10 * np.max(np.abs(xo)), name
    else:
        np.testing.assert_allclose(x, xo, err_msg=name, **_hist_tol(st))


VCYCLE = ("2d_aniso9_linexy", "3d_fe27_f11")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cases.ORCHESTRATED), ids=str)
def test_orchestrated_driver(programs, oracle, tmp_path, name):
    """tests/cxx/orchestrated.cc, mode case: a resident solve, the orchestrated solve on the same solver with `levels`
    untouched, the levels as the manager set them up, and the levels a second solver downloads -- against the oracle
    (level count, history, x, P and A of every level as tests/test_gpu_periodic.py compares them) and against each other"""
    mk_op, mk_rhs, st, per = cases.ORCHESTRATED[name]
    so, b = mk_op(), mk_rhs()
    relax = st.get("relax", "point")
    x0 = pb.uniform(b.shape, 77, -1, 1) * pb.interior_mask(b.shape) if name in VCYCLE else None
    got = _orchestrated(programs["orchestrated"], tmp_path, so, b, st, per, "case", x0)
    assert got["resident_before"] == 1
    ml = oracle.ml_create(so, **st)
    xo = np.zeros_like(b)
    ho = ml.solve(b, xo, maxiter=cases.ORCHESTRATED_MAXITER, tol=1e-8)
    nlev = ml.nlevels()
    assert got["nlevels"] == nlev
    x_orc = np.fromfile(tmp_path / "orc_x.bin").reshape(b.shape)
    x_res = np.fromfile(tmp_path / "res_x.bin").reshape(b.shape)
    _vs_oracle(name + " orchestrated", st, got["hist_orchestrated"], x_orc, ho, xo)
    # orchestrated against resident
    assert len(got["hist_resident"]) == len(got["hist_orchestrated"])
    if relax == "point":
        np.testing.assert_allclose(got["hist_orchestrated"], got["hist_resident"], rtol=1e-12)
    elif relax.startswith("plane"):
        np.testing.assert_allclose(got["hist_orchestrated"], got["hist_resident"], rtol=1e-10)
    else:
        # the resident solver solves the lines of levels up to 64 x 64 in DPTTRS order, the drop-in by a scan
        assert np.max(np.abs(x_orc - x_res)) <= 1e-11 * np.max(np.abs(x_res))
        _vs_oracle(name + " resident", st, got["hist_resident"], x_res, ho, xo)
    # hierarchies
    nsor = 2 if so.ndim == 3 else 1
    for lvl in range(nlev):
        g = tuple(m + 2 for m in ml.dims(lvl)[:so.ndim - 1][::-1])
        arr = lambda tag, what: np.fromfile(tmp_path / f"{tag}_L{lvl}_{what}.bin").reshape((-1,) + g)
        if lvl > 0:
            Po, Ao = ml.array(lvl, "P"), ml.array(lvl, "A")
            P, A, Pd, Ad = arr("mgr", "P"), arr("mgr", "A"), arr("dl", "P"), arr("dl", "A")
            assert P.shape == Po.shape and A.shape == Ao.shape
            assert np.array_equal(P, Po) or np.max(np.abs(P - Po)) <= 1e-13 * np.max(np.abs(Po)), lvl
            assert np.max(np.abs(A - Ao)) <= 1e-12 * np.max(np.abs(Ao)), lvl
            assert np.array_equal(Pd, P) or np.max(np.abs(Pd - P)) <= 1e-13 * np.max(np.abs(P)), lvl
            assert np.max(np.abs(Ad - A)) <= 1e-12 * np.max(np.abs(A)), lvl
        if relax == "point" and lvl + 1 < nlev:
            for s in range(nsor):
                S = arr("mgr", f"SOR{s}")
                assert S.shape[0] == 2 and (s > 0 or S.any()) and np.array_equal(S, arr("dl", f"SOR{s}")), (lvl, s)
    if x0 is not None:
        xv = x0.copy()
        ml.vcycle(xv, b)
        got_v = np.fromfile(tmp_path / "vc_x.bin").reshape(b.shape)
        print(name, "vcycle max |x - xo| / max |xo|", np.max(np.abs(got_v - xv)) / np.max(np.abs(xv)))
        np.testing.assert_allclose(got_v, xv, err_msg=name + " vcycle", **_hist_tol(st))
    ml.close()


COUNTED = {
    "2d": (lambda: pb.aniso9(38, 33), lambda: pb.rhs2(38, 33), dict(relax="line-xy"),
           ("residual", "restriction", "interp_add", "setup_interp", "coarsen_op", "solve_cg", "line_relax_x", "line_relax_y")),
    "3d": (lambda: pb.fe3(13, 12, 11), lambda: pb.rhs3(13, 12, 11), dict(relax="plane-xy"),
           ("residual", "restriction", "interp_add", "setup_interp", "coarsen_op", "solve_cg", "plane_relax_xy")),
}


@pytest.mark.gpu
@pytest.mark.parametrize("dim", list(COUNTED), ids=str)
def test_every_abstract_kernel_class_dispatches(programs, oracle, tmp_path, dim):
    """a counting wrapper for every abstract class, registered with add<T, impl>("user") and selected before the first
    solve: the driver calls each as often as the reference's loop does, and since the wrappers only count, the history is
    the all-"hip" orchestrated history bit for bit"""
    mk_op, mk_rhs, st, classes = COUNTED[dim]
    so, b = mk_op(), mk_rhs()
    got = _orchestrated(programs["orchestrated"], tmp_path, so, b, st, None, "count")
    assert got["resident_before"] == 0
    ml = oracle.ml_create(so, **st)
    L = ml.nlevels()
    ml.close()
    c = len(got["hist_user"]) - 1
    assert got["nlevels"] == L and L >= 3 and c >= 2
    want = {"setup_interp": [0, L - 1], "coarsen_op": [0, L - 1], "solve_cg": [1, c], "restriction": [0, (L - 1) * c],
            "interp_add": [0, (L - 1) * c], "residual": [0, (L - 1) * c + c + 1], "line_relax_x": [L - 1, 3 * (L - 1) * c],
            "line_relax_y": [L - 1, 3 * (L - 1) * c], "plane_relax_xy": [L - 1, 3 * (L - 1) * c]}
    assert got["counts"] == {k: want[k] for k in classes}
    assert got["hist_user"] == got["hist_hip"]


@pytest.mark.gpu
def test_orchestrated_solve_after_levels_were_downloaded(programs, oracle, tmp_path):
    """a resident solve, a read of levels.get(1).A (which downloads the hierarchy), then force_orchestrated and solve:
    multilevel::ready() must still set the smoothers and the coarse solver up through the manager"""
    so, b = pb.poisson2(20, 17), pb.rhs2(20, 17)
    got = _orchestrated(programs["orchestrated"], tmp_path, so, b, {}, None, "defect")
    ml = oracle.ml_create(so)
    xo = np.zeros_like(b)
    ho = ml.solve(b, xo, maxiter=cases.ORCHESTRATED_MAXITER, tol=1e-8)
    assert got["nlevels"] == ml.nlevels() and got["a1"] != 0.0
    ml.close()
    _vs_oracle("after download", {}, got["hist_orchestrated"], np.fromfile(tmp_path / "orc_x.bin").reshape(b.shape), ho, xo)
    np.testing.assert_allclose(got["hist_orchestrated"], got["hist_resident"], rtol=1e-12)


def test_periodic_2d_coarse_setup_refuses_band_storage(capfd):
    """the periodic coarsest operator is dense: BMG2_SymStd_SETUP_cg_LU indexes ABD(n, n), so the band-shaped array of the
    Dirichlet set-up is refused before anything is staged (no device needed), as the 3D entry point refuses it"""
    from cedar_amd import capi
    so = pb.random_op((7, 8), 5, 3, zero_ghost=False)
    abd = np.zeros((30, 8))
    capi.Kernels().setup_cg2(so, abd, ibc=2)
    assert "dense" in capfd.readouterr().err and not abd.any()
