"""CPU test of the single-precision-operator interface: the built library exports the entry points, the header declares
them, the Python front end has the methods (no compute call is made here)."""
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

OP32 = ["cedar_amd_solver_use_fp32_operator", "cedar_amd_solver_fp32_levels", "cedar_amd_relax3_gs_op32",
        "cedar_amd_residual3_op32"]


def test_library_exports_the_op32_entry_points():
    from cedar_amd import capi
    missing = [s for s in OP32 if not hasattr(capi.lib, s)]
    assert not missing, missing


def test_header_declares_the_op32_entry_points():
    txt = open(os.path.join(ROOT, "include", "cedar_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(cedar_amd_\w+)\s*\(", txt))
    assert not [s for s in OP32 if s not in declared]


def test_python_front_end_has_the_op32_methods():
    from cedar_amd import capi
    import inspect
    for m in ("use_fp32_operator", "fp32_levels"):
        assert callable(getattr(capi.Solver, m, None)), m
    for m in ("relax3_op32", "residual3_op32"):
        assert callable(getattr(capi.Kernels, m, None)), m
    assert inspect.signature(capi.Solver.use_fp32_operator).parameters["min_rows"].default == 0
