"""CPU test of the interface of the single-precision operator and factors of 2D line-relaxed levels: the built library
exports the entry points, the header declares them, the Python front end and the C++ mirror have the methods (no compute
call is made here)."""
import inspect
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

OP32_LINES = ["cedar_amd_solver_use_fp32_operator_lines", "cedar_amd_relax2_lines_op32", "cedar_amd_relax2_lines_many_op32"]


def test_library_exports_the_lines_op32_entry_points():
    from cedar_amd import capi
    missing = [s for s in OP32_LINES if not hasattr(capi.lib, s)]
    assert not missing, missing


def test_header_declares_the_lines_op32_entry_points():
    txt = open(os.path.join(ROOT, "include", "cedar_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(cedar_amd_\w+)\s*\(", txt))
    assert not [s for s in OP32_LINES if s not in declared]


def test_python_front_end_has_the_lines_op32_methods():
    from cedar_amd import capi
    assert callable(getattr(capi.Solver, "use_fp32_operator_lines", None))
    for m in ("relax2_lines_op32", "relax2_lines_many_op32"):
        assert callable(getattr(capi.Kernels, m, None)), m
    assert inspect.signature(capi.Solver.use_fp32_operator_lines).parameters["min_rows"].default == 0


def test_cxx_mirror_has_the_method():
    txt = open(os.path.join(ROOT, "include", "cedar", "multilevel.h")).read()
    assert re.search(r"int\s+use_fp32_operator_lines\s*\(\s*int\s+min_rows\s*=\s*0\s*\)", txt)
