"""CPU test of flexible CG on periodic handles: the built library exports the two entry points, the header declares them
and says what they serve and refuse, the Python and C++ front ends have the methods, and the calls that refuse periodic
handles still say so (no compute call is made here)."""
import inspect
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

NEW = ["cedar_amd_solver_fcg_periodic", "cedar_amd_pcg_direction_periodic"]


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_library_exports_the_periodic_entry_points():
    from cedar_amd import capi
    missing = [s for s in NEW if not hasattr(capi.lib, s)]
    assert not missing, missing


def test_header_declares_the_periodic_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", _read("include", "cedar_amd.h"), flags=re.S)
    declared = set(re.findall(r"\b(cedar_amd_\w+)\s*\(", txt))
    assert not [s for s in NEW if s not in declared]
    flat = " ".join(txt.split())
    assert ("int cedar_amd_pcg_direction_periodic(const real_t *so, const real_t *z, const real_t *p, real_t *pn, real_t *w, "
            "len_t ii, len_t jj, len_t kk, int nstncl, int ibc, int first, real_t *sc, real_t *partial);") in flat
    assert ("int cedar_amd_solver_fcg_periodic(cedar_amd_solver *s, const real_t *b, real_t *x, "
            "const cedar_amd_pcg_settings *p, real_t *hist);") in flat


def test_header_states_the_contract():
    txt = " ".join(_read("include", "cedar_amd.h").split())
    doc = txt[txt.index("Flexible CG on a periodic handle"): txt.index("int cedar_amd_solver_fcg_periodic(")]
    for phrase in ("singular", "definite", "ghost layers", "forwards to cedar_amd_solver_fcg", "F-cycles",
                   "cedar_amd_solver_create_many", "keep refusing ibc != 0"):
        assert phrase in doc, phrase
    doc = txt[txt.index("The same pass on a level with periodic directions"): txt.index("int cedar_amd_pcg_direction_periodic(")]
    for phrase in ("opposite interior end", "NO ghost cell of z or p in a periodic direction contributes to any result", "Cedar planes",
                   "ibc = 0 forwards"):
        assert phrase in doc, phrase


def test_front_ends_have_the_methods():
    from cedar_amd import capi
    par = inspect.signature(capi.Solver.fcg_periodic).parameters
    assert list(par)[1:3] == ["b", "x"]
    assert [par[k].default for k in ("max_iter", "tol", "stop", "precon", "nmg_cycles")] == [50, 1e-8, "rel_l2", "mg", 1]
    assert callable(getattr(capi.Kernels, "pcg_direction_periodic", None))
    ml = _read("include", "cedar", "multilevel.h")
    assert re.search(r"void\s+fcg_periodic\s*\(\s*const grid_func\s*&\s*b\s*,\s*grid_func\s*&\s*x\s*\)", ml)
    assert "cedar_amd_solver_fcg_periodic" in ml


def test_the_other_calls_still_refuse_periodic_handles():
    """pcg_refused, fcg_refused (without the new call's flag), many_refused keep their ibc != 0 line"""
    src = _read("cedar_amd", "csrc", "solver.cpp")
    assert src.count('"periodic boundary conditions (ibc != 0) are not supported"') >= 7
    body = src[src.index("int cedar_amd_solver_fcg(cedar_amd_solver *s"):]
    body = body[: body.index("\n}\n")]
    assert "fcg_refused(s, p, who)" in body


def test_periodic_krylov_source_does_not_reference_oracle():
    src = os.path.join(ROOT, "cedar_amd", "csrc", "krylov.hip")
    txt = open(src).read()
    for k in ("pcg_dir2_per", "pcg_dir7_per", "pcg_dir27_per", "pcg_direction_periodic"):
        assert k in txt, k
    assert not re.search(r"(liboracle|pyoracle|orc[23]?_|oracle/)", txt)
