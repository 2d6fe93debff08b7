"""CPU test of batches on periodic 3D handles: the built library exports the seven entry points, the header declares them
and states what is served, refused and forwarded, the Python and C++ front ends have the methods, and the new sources do
not lean on the oracle (no compute call is made here)."""
import inspect
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

NEW = ["cedar_amd_solver_create_many_periodic", "cedar_amd_solver_fcg_periodic_many", "cedar_amd_relax3_gs_periodic_many",
       "cedar_amd_restrict3_periodic_many", "cedar_amd_interp_add3_periodic_many", "cedar_amd_solve_cg3_periodic_many",
       "cedar_amd_pcg_direction_periodic_many"]


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
    assert ("cedar_amd_solver *cedar_amd_solver_create_many_periodic(int nd, len_t nx, len_t ny, len_t nz, int nstencil, "
            "const real_t *so, int own_device_so, const cedar_amd_settings *settings, int max_rhs);") in flat
    assert ("int cedar_amd_solver_fcg_periodic_many(cedar_amd_solver *s, int nrhs, const real_t *b, real_t *x, "
            "const cedar_amd_pcg_settings *p, real_t *hist, int *iters);") in flat
    assert ("int cedar_amd_relax3_gs_periodic_many(int nrhs, real_t *so, real_t *qf, real_t *q, real_t *sor, len_t ii, len_t jj, "
            "len_t kk, int nstncl, int updown, int ibc, int ghosts_consistent);") in flat
    assert ("int cedar_amd_pcg_direction_periodic_many(int nrhs, unsigned active, const real_t *so, const real_t *z, "
            "const real_t *p, real_t *pn, real_t *w, len_t ii, len_t jj, len_t kk, int nstncl, int ibc, int first, real_t *sc);") in flat


def test_header_states_the_contract():
    txt = " ".join(_read("include", "cedar_amd.h").split())
    doc = txt[txt.index("Several right-hand sides at once on a PERIODIC 3D handle"):
              txt.index("cedar_amd_solver *cedar_amd_solver_create_many_periodic(")]
    for phrase in ("cedar_amd_solver_create_many itself is unchanged", "still holds one item", "ibc 1..3 and 5..8",
                   "ibc == 0 goes to cedar_amd_solver_create_many", "nd == 2 with ibc != 0", "an F-cycle", "relaxation",
                   "max_rhs outside 1 .. 32", "odd periodic extent", "2048", "nrhs > max_rhs", "cedar_amd_solver_pcg_many",
                   "cedar_amd_solver_fcg_many", "cedar_amd_solver_fcg_periodic when max_rhs > 1",
                   "has the bits of the single-vector periodic call on item m alone", "no partial-sum", "2D periodic batches"):
        assert phrase in doc, phrase
    doc = txt[txt.index("cedar_amd_solver_fcg_periodic on the first nrhs items in lockstep"):
              txt.index("int cedar_amd_solver_fcg_periodic_many(")]
    for phrase in ("cedar_amd_solver_fcg_many", "bit for bit", "nrhs == 1 runs the single-vector path", "is forwarded", "is refused"):
        assert phrase in doc, phrase
    doc = txt[txt.index("The batched periodic 3D kernels one by one"): txt.index("int cedar_amd_relax3_gs_periodic_many(")]
    for phrase in ("nrhs outside 1 .. 32", "a NULL array", "4 | 14", "a boundary code 3D does not define",
                   "ibc = 0 forwards to the Dirichlet _many call", "ghosts_consistent", "one workgroup per item",
                   "a masked item is neither read nor written"):
        assert phrase in doc, phrase


def test_front_ends_have_the_methods():
    from cedar_amd import capi
    par = inspect.signature(capi.Solver.__init__).parameters
    assert par["periodic_batch"].default is False and par["max_rhs"].default == 1
    par = inspect.signature(capi.Solver.fcg_periodic_many).parameters
    want = inspect.signature(capi.Solver.fcg_many).parameters
    assert list(par) == list(want) and [par[k].default for k in par] == [want[k].default for k in want]
    for m in ("relax3_periodic_many", "restrict3_periodic_many", "interp_add3_periodic_many", "solve_cg3_periodic_many",
              "pcg_direction_periodic_many"):
        assert callable(getattr(capi.Kernels, m, None)), m
    ml = _read("include", "cedar", "multilevel.h")
    assert re.search(r"void\s+fcg_periodic_many\s*\(\s*const std::vector<grid_func>\s*&\s*b\s*,\s*std::vector<grid_func>\s*&\s*x\s*\)", ml)
    assert "krylov_many(cedar_amd_solver_fcg_periodic_many" in ml
    sv = _read("include", "cedar", "3d", "solver.h")
    assert "solver.periodic-batch" in sv and "cedar_amd_solver_create_many_periodic" in sv


def test_create_many_and_the_refusals_are_as_before():
    """cedar_amd_solver_create_many is a range check plus solver_create with no flag; many_refused tells the two kinds of
    periodic handle apart by the flag the new call sets"""
    src = _read("cedar_amd", "csrc", "solver.cpp")
    body = src[src.index("cedar_amd_solver *cedar_amd_solver_create_many(int nd"):]
    body = body[: body.index("\n}\n")]
    assert "return solver_create(nd, nx, ny, nz, nstencil, so, own_device_so, settings, max_rhs);" in body
    body = src[src.index("static bool many_refused("):]
    body = body[: body.index("\n}\n")]
    assert 's->st.ibc != 0 && !s->per_batch) why = "periodic boundary conditions (ibc != 0) are not supported"' in body
    body = src[src.index("int cedar_amd_solver_fcg_periodic(cedar_amd_solver *s"):]
    body = body[: body.index("\n}\n")]
    assert "s->nb_alloc > 1" in body


def test_new_sources_do_not_reference_the_oracle():
    unit = os.path.join(ROOT, "cedar_amd", "csrc", "periodic_many3d.hip")
    assert os.path.exists(unit)
    txt = open(unit).read()
    for k in ("relax3_gs_per_many", "restrict3_per_many", "interp_add3_per_many"):
        assert k in txt, k
    # the x-periodic row task is the batched row task of many3d.hip under a PERX template parameter ...
    m3 = _read("cedar_amd", "csrc", "many3d.hip")
    assert re.search(r"template <[^>]*\bbool PERX\b[^>]*>\s*__device__ __forceinline__ void relax27_row_task_many\(", m3)
    assert re.search(r"template <[^>]*\bbool PERX\b[^>]*>\s*__global__ __launch_bounds__\(BS\) void relax27_rows_many\(", m3)
    assert "relax3_class27_many(A, qf, q, II, JJ, KK, jb, kb, up, st, bt, px)" in txt
    # ... and the coarsest solve of a batch is the one kernel of periodic3d.hip, which takes its item from blockIdx.x
    p3 = _read("cedar_amd", "csrc", "periodic3d.hip")
    body = p3[p3.index("void solve_cg3_per_kernel("):]
    body = body[: body.index("\n}\n")]
    for k in ("q += (size_t)blockIdx.x * stride;", "qf += (size_t)blockIdx.x * stride;", "bbd += (size_t)blockIdx.x * (size_t)N;"):
        assert k in body, k
    assert "dim3(bt.n), dim3(1024)" in p3[p3.index("void solve_cg3_per(real_t *q"):]
    kry = _read("cedar_amd", "csrc", "krylov.hip")
    for k in ("pcg_dir7_per_many", "pcg_dir27_per_many", "pcg_direction_periodic_many"):
        assert k in kry, k
    mk = _read("cedar_amd", "csrc", "Makefile")
    assert "periodic_many3d.o" in mk
    for t in (txt, _read("cedar_amd", "capi.py")):
        assert not re.search(r"(liboracle|pyoracle|orc[23]?_|oracle/)", t)
