"""CPU test of batches on periodic 2D handles: the built library exports the six entry points, the header declares them and
states what is served, forwarded and refused, the 3D block above it is as it was, the Python and C++ front ends have the
methods, and the new unit does not lean on the oracle (no compute call is made here)."""
import inspect
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

NEW = ["cedar_amd_solver_create_many_periodic2", "cedar_amd_relax2_gs_periodic_many", "cedar_amd_restrict2_periodic_many",
       "cedar_amd_interp_add2_periodic_many", "cedar_amd_solve_cg2_periodic_many", "cedar_amd_pcg_direction2_periodic_many"]


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_library_exports_the_entry_points():
    from cedar_amd import capi
    missing = [s for s in NEW if not hasattr(capi.lib, s)]
    assert not missing, missing


def test_header_declares_the_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", _read("include", "cedar_amd.h"), flags=re.S)
    declared = set(re.findall(r"\b(cedar_amd_\w+)\s*\(", txt))
    assert not [s for s in NEW if s not in declared]
    flat = " ".join(txt.split())
    for decl in (
            "cedar_amd_solver *cedar_amd_solver_create_many_periodic2(len_t nx, len_t ny, int nstencil, const real_t *so, "
            "int own_device_so, const cedar_amd_settings *settings, int max_rhs);",
            "int cedar_amd_relax2_gs_periodic_many(int nrhs, real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, "
            "int nstncl, int updown, int ibc);",
            "int cedar_amd_restrict2_periodic_many(int nrhs, real_t *q, real_t *qc, real_t *ci, len_t ii, len_t jj, len_t iic, "
            "len_t jjc, int ibc);",
            "int cedar_amd_interp_add2_periodic_many(int nrhs, real_t *q, real_t *qc, real_t *res, real_t *so, real_t *ci, "
            "len_t iic, len_t jjc, len_t ii, len_t jj, int nstncl, int ibc);",
            "int cedar_amd_solve_cg2_periodic_many(int nrhs, real_t *q, real_t *qf, len_t ii, len_t jj, real_t *abd, real_t *bbd, "
            "len_t nabd1, int ibc);",
            "int cedar_amd_pcg_direction2_periodic_many(int nrhs, unsigned active, const real_t *so, const real_t *z, "
            "const real_t *p, real_t *pn, real_t *w, len_t ii, len_t jj, int nstncl, int ibc, int first, real_t *sc);"):
        assert decl in flat, decl


def test_header_states_the_contract():
    txt = " ".join(_read("include", "cedar_amd.h").replace("\n *", "\n").split())  # (a comment's line breaks do not count)
    start =txt.index("Several right-hand sides at once on a PERIODIC 2D handle")
    doc = txt[start: txt.index("cedar_amd_solver *cedar_amd_solver_create_many_periodic2(")]
    for phrase in ("served by a call of its own, cedar_amd_solver_create_many_periodic2", "still holds one item",
                   "keeps refusing nd == 2", "ibc 1..3", "5- and 9-point", "max_rhs 1 .. 32", "8190",
                   "line-x, line-y, line-xy", "cedar_amd_solver_fcg_periodic_many", "wrapped before the first residual",
                   "nrhs == 1 runs the single-vector path", "exactly the launches",
                   "ibc == 0 goes to cedar_amd_solver_create_many(2, ...)", "goes to cedar_amd_solver_fcg_many",
                   "an F-cycle", "max_rhs outside 1 .. 32", "a boundary code 2D does not define",
                   "its message first, then a line that names this call", "nrhs < 1 or nrhs > max_rhs",
                   "cedar_amd_solver_pcg_many", "cedar_amd_solver_fcg_many", "cedar_amd_solver_fcg_periodic when max_rhs > 1",
                   "every single-precision switch", "has the bits of the single-vector periodic call on item m alone",
                   "no partial-sum sweep and no float view", "a batched periodic y-line pipeline"):
        assert phrase in doc, phrase
    doc = txt[txt.index("The batched periodic 2D kernels one at a time"): txt.index("int cedar_amd_relax2_gs_periodic_many(")]
    for phrase in ("stride ii*jj", "nrhs outside 1 .. 32", "NULL array", "3 | 5", "ibc outside 0 .. 3",
                   "forwards to cedar_amd_pcg_direction_many", "refuse it", "8192", "512 interior points", "one lane per item",
                   "side effect on res per item", "a masked item is neither read nor written",
                   "cedar_amd_pcg_direction_periodic_many keeps refusing nstncl 3 | 5"):
        assert phrase in doc, phrase
    # the new block comes after the 3D one, which is as it was
    d3 = txt.index("Several right-hand sides at once on a PERIODIC 3D handle")
    assert d3 < txt.index("int cedar_amd_pcg_direction_periodic_many(") < start
    doc3 = txt[d3: txt.index("cedar_amd_solver *cedar_amd_solver_create_many_periodic(")]
    for phrase in ("cedar_amd_solver_create_many itself is unchanged", "still holds one item", "ibc 1..3 and 5..8",
                   "ibc == 0 goes to cedar_amd_solver_create_many", "nd == 2 with ibc != 0", "an F-cycle", "relaxation",
                   "max_rhs outside 1 .. 32", "odd periodic extent", "2048", "nrhs > max_rhs", "cedar_amd_solver_pcg_many",
                   "cedar_amd_solver_fcg_many", "cedar_amd_solver_fcg_periodic when max_rhs > 1",
                   "has the bits of the single-vector periodic call on item m alone", "no partial-sum", "2D periodic batches"):
        assert phrase in doc3, phrase


def test_front_ends_have_the_methods():
    from cedar_amd import capi
    par = inspect.signature(capi.Solver.__init__).parameters
    assert par["periodic_batch2d"].default is False and par["periodic_batch"].default is False and par["max_rhs"].default == 1
    for m in ("relax2_periodic_many", "restrict2_periodic_many", "interp_add2_periodic_many", "solve_cg2_periodic_many",
              "pcg_direction2_periodic_many"):
        assert callable(getattr(capi.Kernels, m, None)), m
    sv = _read("include", "cedar", "2d", "solver.h")
    assert "solver.periodic-batch" in sv and "cedar_amd_solver_create_many_periodic2(" in sv
    ml = _read("include", "cedar", "multilevel.h")
    at = ml.index("void fcg_periodic_many(")
    assert "a 3D solver" not in ml[ml.rindex("\n\n", 0, at): at]


def test_the_old_calls_are_as_before():
    """cedar_amd_solver_create_many is a range check plus solver_create with no flag; the 3D periodic call still turns a
    2D operator away; many_refused is word for word what it was"""
    src = _read("cedar_amd", "csrc", "solver.cpp")
    body = src[src.index("cedar_amd_solver *cedar_amd_solver_create_many(int nd"):]
    body = body[: body.index("\n}\n")]
    assert "return solver_create(nd, nx, ny, nz, nstencil, so, own_device_so, settings, max_rhs);" in body
    body = src[src.index("cedar_amd_solver *cedar_amd_solver_create_many_periodic(int nd"):]
    body = body[: body.index("\n}\n")]
    assert 'else if (nd != 3) why = "periodic batches are served in 3D only";' in body
    body = src[src.index("static bool many_refused("):]
    body = body[: body.index("\n}\n")]
    for line in ('if (nrhs < 1) why = "nrhs must be at least 1";',
                 'else if (s->st.ibc != 0 && !s->per_batch) why = "periodic boundary conditions (ibc != 0) are not supported";',
                 'else if (s->st.cycle != 0) why = "only the V-cycle is supported";',
                 'else if (s->nd == 3 && s->st.relaxation != CEDAR_AMD_RELAX_POINT) why = "3D plane relaxation is not supported";',
                 'else if (nrhs > s->nb_alloc) why = "nrhs exceeds the handle\'s max_rhs (cedar_amd_solver_create_many)";'):
        assert line in body, line


def test_new_unit_is_built_and_does_not_reference_the_oracle():
    unit = os.path.join(ROOT, "cedar_amd", "csrc", "periodic_many2d.hip")
    assert os.path.exists(unit)
    txt = open(unit).read()
    for k in ("relax2_per_many", "relax2_gs_per_many"):
        assert k in txt, k
    # the transfers and the coarsest solve of a batch are periodic2d.hip's own, which take the batch: the wraps get its item
    # count as planes, and the solve kernel takes its item from blockIdx.x
    p2 = _read("cedar_amd", "csrc", "periodic2d.hip")
    body = p2[p2.index("void restrict2_per(real_t *q"):]
    body = body[: body.index("\n}\n")]
    assert "Batch bf" in body and "wrap2(q, Nx, Ny, bf.n," in body and "restrict2(q, qc, ci, Nx, Ny, Nxc, Nyc, st, bf, bc);" in body
    body = p2[p2.index("void interp_add2_per(real_t *q"):]
    body = body[: body.index("\n}\n")]
    assert "Batch bf" in body and "wrap2(q, IIF, JJF, bf.n," in body and "IIF, JJF, st, bf, bc);" in body
    body = p2[p2.index("void solve_cg2_per_kernel("):]
    body = body[: body.index("\n}\n")]
    for k in ("q += (size_t)blockIdx.x * stride;", "qf += (size_t)blockIdx.x * stride;", "bbd += (size_t)blockIdx.x * (size_t)n;",
              "if (pd.x && pd.y) {"):
        assert k in body, k
    assert "dim3(bt.n), dim3(64)" in p2[p2.index("void solve_cg2_per(real_t *q"):]
    kry = _read("cedar_amd", "csrc", "krylov.hip")
    assert "pcg_dir2_per_many" in kry and "no 2D level here" not in kry
    mk = _read("cedar_amd", "csrc", "Makefile")
    assert "periodic_many2d.o" in mk
    for t in (txt, _read("cedar_amd", "capi.py")):
        assert not re.search(r"(liboracle|pyoracle|orc[23]?_|oracle/)", t)
