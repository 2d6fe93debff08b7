"""CPU test of the several-right-hand-sides interface: the built library exports the batched entry points, the header
declares them, the Python front end has the methods (no compute call is made here)."""
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

MANY = ["cedar_amd_solver_create_many", "cedar_amd_solver_max_rhs", "cedar_amd_solver_vcycle_many",
        "cedar_amd_solver_solve_many", "cedar_amd_solver_time_vcycles_many",
        "cedar_amd_relax3_gs_many", "cedar_amd_residual3_many", "cedar_amd_restrict3_many", "cedar_amd_interp_add3_many"]


def test_library_exports_the_batched_entry_points():
    from cedar_amd import capi
    missing = [s for s in MANY if not hasattr(capi.lib, s)]
    assert not missing, missing


def test_header_declares_the_batched_entry_points():
    txt = open(os.path.join(ROOT, "include", "cedar_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(cedar_amd_\w+)\s*\(", txt))
    assert not [s for s in MANY if s not in declared]
    assert re.search(r"CEDAR_AMD_MAX_RHS\s*=\s*32", txt)


def test_python_front_end_has_the_batched_methods():
    from cedar_amd import capi
    import inspect
    for m in ("max_rhs", "vcycle_many", "solve_many", "time_vcycles_many"):
        assert callable(getattr(capi.Solver, m, None)), m
    for m in ("relax3_many", "residual3_many", "restrict3_many", "interp_add3_many"):
        assert callable(getattr(capi.Kernels, m, None)), m
    assert inspect.signature(capi.Solver.__init__).parameters["max_rhs"].default == 1


def test_batched_sources_do_not_reference_oracle():
    """nothing under cedar_amd/ may import, link or call anything under oracle/ -- the new unit included"""
    src = os.path.join(ROOT, "cedar_amd", "csrc", "many3d.hip")
    assert os.path.exists(src)
    for f in (src, os.path.join(ROOT, "cedar_amd", "capi.py")):
        assert not re.search(r"(liboracle|pyoracle|orc[23]?_|oracle/)", open(f).read()), f
