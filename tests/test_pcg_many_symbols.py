"""CPU test of conjugate gradients on several right-hand sides: the built library exports the batched entry points, the
header declares them and no longer says they are not offered, the Python front end has the methods (no compute call
is made here)."""
import inspect
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

NEW = ["cedar_amd_solver_pcg_many", "cedar_amd_pcg_direction_many", "cedar_amd_pcg_update_many"]


def _header():
    return open(os.path.join(ROOT, "include", "cedar_amd.h")).read()


def test_library_exports_the_batched_pcg_entry_points():
    from cedar_amd import capi
    missing = [s for s in NEW if not hasattr(capi.lib, s)]
    assert not missing, missing


def test_header_declares_the_batched_pcg_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(cedar_amd_\w+)\s*\(", txt))
    assert not [s for s in NEW if s not in declared]


def test_header_no_longer_says_batch_pcg_is_not_offered():
    txt = " ".join(_header().split())
    assert not re.search(r"Not offered:[^.]*_pcg on several right-hand sides", txt)
    # the differences from solve_many and the cost of lockstep are stated where the call is declared
    doc = txt[txt.index("cedar_amd_solver_pcg on the first nrhs items"): txt.index("int cedar_amd_solver_pcg_many(")]
    for phrase in ("frozen", "cedar_amd_solver_solve_many", "block CG", "CEDAR_AMD_PSUM=0"):
        assert phrase in doc, phrase


def test_python_front_end_has_the_batched_pcg_methods():
    from cedar_amd import capi
    assert callable(getattr(capi.Solver, "pcg_many", None))
    par = inspect.signature(capi.Solver.pcg_many).parameters
    assert [par[k].default for k in ("max_iter", "tol", "stop", "precon", "nmg_cycles", "hist")] == [50, 1e-8, "rel_l2", "mg", 1, None]
    for m in ("pcg_direction_many", "pcg_update_many"):
        assert callable(getattr(capi.Kernels, m, None)), m


def test_batched_krylov_source_does_not_reference_oracle():
    """nothing under cedar_amd/ may import, link or call anything under oracle/ -- the unit with the new kernels included"""
    src = os.path.join(ROOT, "cedar_amd", "csrc", "krylov.hip")
    txt = open(src).read()
    for k in ("pcg_dir27_many", "pcg_dir7_many", "pcg_upd_many", "pcg_dir2_many", "pcg_alpha_many", "pcg_rho_many"):
        assert k in txt, k
    for f in (src, os.path.join(ROOT, "cedar_amd", "capi.py")):
        assert not re.search(r"(liboracle|pyoracle|orc[23]?_|oracle/)", open(f).read()), f
