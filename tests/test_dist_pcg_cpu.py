"""CPU test: the preconditioned conjugate gradient of the domain-decomposed drivers is declared in include/cedar_amd.h,
exported by the library built for gfx950, and reachable from Python (DistSolver3 / DistSolver2).  No compute call."""
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ["cedar_amd_dist3_pcg", "cedar_amd_dist3_precondition", "cedar_amd_dist2_pcg", "cedar_amd_dist2_precondition"]


def test_declared_in_header():
    txt = open(os.path.join(ROOT, "include", "cedar_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt), name
    # the settings of the single-domain PCG are reused as they are
    assert re.search(r"cedar_amd_dist3_pcg\s*\([^)]*const cedar_amd_pcg_settings \*p, real_t \*hist\)", txt)
    assert re.search(r"cedar_amd_dist2_pcg\s*\([^)]*const cedar_amd_pcg_settings \*p, real_t \*hist\)", txt)


def test_exported_with_prototypes():
    import ctypes as C
    from cedar_amd import capi, dist3
    for name in NEW:
        assert hasattr(capi.lib, name), name
    for k in ("3", "2"):
        fn = getattr(capi.lib, f"cedar_amd_dist{k}_pcg")
        assert fn.restype is C.c_int
        assert fn.argtypes[3] is C.POINTER(capi.PcgSettings)
    assert dist3.lib is capi.lib


def test_python_methods():
    import inspect
    from cedar_amd import capi
    from cedar_amd.dist3 import DistSolver2, DistSolver3
    want = inspect.signature(capi.Solver.pcg)
    for cls in (DistSolver3, DistSolver2):
        assert inspect.signature(cls.pcg) == want, cls
        assert list(inspect.signature(cls.precondition).parameters) == ["self", "z", "r"]
