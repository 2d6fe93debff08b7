"""CPU test of the semidefinite entry points: the built library exports them, the header declares them and states their
contract, the Python and C++ front ends have the methods and the configuration key, and the calls that refuse periodic
handles keep their lines (no compute call is made here)."""
import inspect
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

NEW = ["cedar_amd_solver_create_semidefinite", "cedar_amd_solver_fcg_semidefinite", "cedar_amd_solver_fcg_semidefinite_many",
       "cedar_amd_project_mean"]


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_library_exports_the_semidefinite_entry_points():
    from cedar_amd import capi
    missing = [s for s in NEW if not hasattr(capi.lib, s)]
    assert not missing, missing


def test_header_declares_the_semidefinite_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", _read("include", "cedar_amd.h"), flags=re.S)
    declared = set(re.findall(r"\b(cedar_amd_\w+)\s*\(", txt))
    assert not [s for s in NEW if s not in declared]
    flat = " ".join(txt.split())
    assert ("cedar_amd_solver *cedar_amd_solver_create_semidefinite(int nd, len_t nx, len_t ny, len_t nz, int nstencil, "
            "const real_t *so, int own_device_so, const cedar_amd_settings *settings, int max_rhs);") in flat
    assert ("int cedar_amd_solver_fcg_semidefinite(cedar_amd_solver *s, const real_t *b, real_t *x, "
            "const cedar_amd_pcg_settings *p, real_t *hist);") in flat
    assert ("int cedar_amd_solver_fcg_semidefinite_many(cedar_amd_solver *s, int nrhs, const real_t *b, real_t *x, "
            "const cedar_amd_pcg_settings *p, real_t *hist, int *iters);") in flat
    assert ("int cedar_amd_project_mean(int nrhs, unsigned active, real_t *v, len_t ii, len_t jj, len_t kk, "
            "real_t *mean);") in flat


def test_header_states_the_contract():
    txt = " ".join(_read("include", "cedar_amd.h").split())
    doc = txt[txt.index("Singular problems: a symmetric positive SEMIdefinite operator"):
              txt.index("cedar_amd_solver *cedar_amd_solver_create_semidefinite(")]
    for phrase in ("null space is the constants", "codes below zero stay refused", "LAST unknown is doubled",
                   "removes the mean", "SETUP_cg_LU", "SOLVE_cg", "1024 eps", "plane relaxation", "ALL its ghost cells",
                   "COMPATIBLE b", "does not project", "names cedar_amd_solver_fcg_semidefinite", "Not offered",
                   "drop-ins"):
        assert phrase in doc, phrase
    doc = txt[txt.index("Flexible CG on a semidefinite handle"): txt.index("int cedar_amd_solver_fcg_semidefinite(")]
    for phrase in ("A x = P b", "mean(x) = 0", "hist[0] = |P (b - A x0)|_2", "b itself is not written", "applied as P M P",
                   "not made by cedar_amd_solver_create_semidefinite"):
        assert phrase in doc, phrase
    doc = txt[txt.index("The projection as a kernel of its own"): txt.index("int cedar_amd_project_mean(")]
    for phrase in ("Ghost cells", "without atomics", "not on nrhs", "8 bytes per point", "nrhs outside 1 .. 32"):
        assert phrase in doc, phrase
    # the periodic block now points here, and keeps the words tests/test_fcg_periodic_symbols.py looks for
    doc = txt[txt.index("Flexible CG on a periodic handle"): txt.index("int cedar_amd_solver_fcg_periodic(")]
    for phrase in ("singular", "definite", "cedar_amd_solver_create_semidefinite"):
        assert phrase in doc, phrase


def test_front_ends_have_the_methods():
    from cedar_amd import capi
    assert inspect.signature(capi.Solver.__init__).parameters["semidefinite"].default is False
    for name in ("fcg_semidefinite", "fcg_semidefinite_many"):
        par = inspect.signature(getattr(capi.Solver, name)).parameters
        assert list(par)[1:3] == ["b", "x"]
        assert [par[k].default for k in ("max_iter", "tol", "stop", "precon", "nmg_cycles")] == [50, 1e-8, "rel_l2", "mg", 1]
    assert callable(getattr(capi.Kernels, "project_mean", None))
    ml = _read("include", "cedar", "multilevel.h")
    assert re.search(r"void\s+fcg_semidefinite\s*\(\s*const grid_func\s*&\s*b\s*,\s*grid_func\s*&\s*x\s*\)", ml)
    assert re.search(r"void\s+fcg_semidefinite_many\s*\(", ml)
    assert "cedar_amd_solver_fcg_semidefinite" in ml and "cedar_amd_solver_fcg_semidefinite_many" in ml
    for d in ("2d", "3d"):
        sv = _read("include", "cedar", d, "solver.h")
        assert '"solver.semidefinite", false' in sv and "cedar_amd_solver_create_semidefinite(" + d[0] + "," in sv


def test_the_other_calls_still_refuse_periodic_and_semidefinite_handles():
    src = _read("cedar_amd", "csrc", "solver.cpp")
    assert src.count('"periodic boundary conditions (ibc != 0) are not supported"') >= 7
    assert src.count("semidef_refused(s, who") >= 9 and 'semidef_refused(s, "cedar_amd_solver_precondition")' in src
    body = src[src.index("static bool semidef_refused("):]
    assert "cedar_amd_solver_fcg_semidefinite" in body[: body.index("\n}\n")]


def test_negative_codes_stay_refused_in_the_source():
    """ibc is not touched: the semidefinite creation call refuses codes below zero itself, solver_create's periodic
    check still admits positive codes only"""
    src = _read("cedar_amd", "csrc", "solver.cpp")
    assert "s->st.ibc >= 1 && s->st.ibc <= 3" in src and "s->st.ibc > 0 && periodic3_code_ok(s->st.ibc)" in src
    body = src[src.index("cedar_amd_solver *cedar_amd_solver_create_semidefinite("):]
    assert "st.ibc < 0" in body[: body.index("\n}\n")]
