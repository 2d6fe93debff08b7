"""CPU test of the interface of the single-precision interpolation weights: the built library exports the entry points,
the header declares them, the Python front end and the C++ mirror have the methods (no compute call is made here)."""
import inspect
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

CI32 = ["cedar_amd_solver_use_fp32_interpolation", "cedar_amd_solver_fp32_interp_levels",
        "cedar_amd_restrict2_ci32", "cedar_amd_interp_add2_ci32", "cedar_amd_restrict3_ci32", "cedar_amd_interp_add3_ci32",
        "cedar_amd_restrict3_many_ci32", "cedar_amd_interp_add3_many_ci32"]


def test_library_exports_the_ci32_entry_points():
    from cedar_amd import capi
    missing = [s for s in CI32 if not hasattr(capi.lib, s)]
    assert not missing, missing


def test_header_declares_the_ci32_entry_points():
    txt = open(os.path.join(ROOT, "include", "cedar_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(cedar_amd_\w+)\s*\(", txt))
    assert not [s for s in CI32 if s not in declared]


def test_python_front_end_has_the_ci32_methods():
    from cedar_amd import capi
    assert callable(getattr(capi.Solver, "use_fp32_interpolation", None))
    assert callable(getattr(capi.Solver, "fp32_interp_levels", None))
    for m in ("restrict2_ci32", "interp_add2_ci32", "restrict3_ci32", "interp_add3_ci32", "restrict3_many_ci32",
              "interp_add3_many_ci32"):
        assert callable(getattr(capi.Kernels, m, None)), m
    assert inspect.signature(capi.Solver.use_fp32_interpolation).parameters["min_rows"].default == 0


def test_cxx_mirror_has_the_method():
    txt = open(os.path.join(ROOT, "include", "cedar", "multilevel.h")).read()
    assert re.search(r"int\s+use_fp32_interpolation\s*\(\s*int\s+min_rows\s*=\s*0\s*\)", txt)
