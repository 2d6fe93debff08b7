"""Every kernel entry point between poisoned guard bands (tests/guarded.py).

TABLE has one row per entry point and variant: the arrays it takes (name, shape, in / out), a callable (K, views) and the
shapes it runs at.  For every row, the three placements (host views that the library stages, device views at 16-byte
and at 8-byte-only alignment) and the two poisons:

1. the call on plain numpy arrays with the same seeded inputs -- the path the rest of the suite pins to the oracle and
   the golden vectors -- gives the expected arrays and return value;
2. the call on the arena's views, then capi.sync();
3. every array that is not an input equals the expected one as uint64, every input still has its bits, the bands hold
   their poison, the return value is the plain call's.

Bit-identity is the derived expectation: the same code on the same inputs.  The two alignment-dependent paths are moves
(transpose2) or asserted bit-identical elsewhere (CEDAR_AMD_GALERKIN_PAIRS).  The reductions of the Krylov passes have
one fixed order (test_gpu_krylov.py::test_passes_are_deterministic).

A batched (_many) row hands arrays of NRHS + 1 items and asks for NRHS: the last item must keep its bits.

Shapes are the smallest at which a path changes: a 3-point grid, an odd and an even row length (the pair paths), one
row longer than a workgroup pass; the line kernels also at 512+ and 2048+ unknowns per line (scan-ordered factor copy,
scan tile).  test_every_kernels_method_is_in_the_table keeps the table complete.
"""
import contextlib
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import boundary_first as bf
import guarded as gd
import problems as pb

pytestmark = pytest.mark.gpu

NRHS = 2
DOWN, UP = 0, 1
S2 = [(3, 3), (10, 3), (9, 4), (258, 3), (257, 4)]
S3 = [(3, 3, 3), (4, 5, 3), (9, 4, 5), (130, 3, 4), (129, 4, 3)]
S2_LINES = S2 + [(600, 4), (4, 600), (2050, 3), (3, 2050)]
S2_PSUM = [(10, 3), (258, 33), (257, 34)]      # the nine-point partial-sum sweep wants nx > 128 and ny >= 8 * run length
S3_PSUM = [(4, 5, 3), (9, 17, 4), (130, 19, 3), (129, 16, 4)]  # the 27-point one ny >= 4 * run length
S3_PER = [(4, 4, 4), (6, 4, 8), (130, 4, 4)]   # periodic 3D: even extents, ny <= nz (cases.CASES_PER3)
S2_PER = [(4, 4), (10, 3), (9, 4), (258, 4)]
# coarse solves: two below and one above the LDS staging limit of test_gpu_coarse_solve.py (LDS_DOUBLES = 60 KiB / 8:
# (49, 3) is the last 2D shape staged, (50, 3) the first that is not; (6, 6, 4) and (7, 6, 4) in 3D)
S2_CG = [(3, 3), (49, 3), (50, 3)]
S3_CG = [(3, 3, 3), (6, 6, 4), (7, 6, 4)]
S2_CGPER = [(3, 3), (4, 3), (5, 4)]
S3_CGPER = [(3, 3, 3), (4, 3, 4)]
# Krylov passes: the smallest shapes of test_gpu_krylov.py (DIR27 / DIR7 / DIR2 / UPD) and one odd long row each
S3_KRY = [(3, 3, 3), (4, 5, 6), (129, 3, 3)]
S2_KRY = [(3, 3), (256, 3), (257, 4)]


@pytest.fixture(scope="module")
def capi():
    from cedar_amd import capi
    assert capi.device_count() >= 1, "no GPU visible"
    return capi


@pytest.fixture(scope="module")
def K(capi):
    return capi.Kernels()


def G(s):
    return tuple(v + 2 for v in reversed(s))


def GC(s):
    return pb.coarse_shape(G(s))


class Row:
    def __init__(self, method, tag, shapes, make, call, ins, nd=None, batched=(), device_only=False, env=None, took=None):
        """env: run-time switches set for the row's calls (the default switches take the partial-sum sweeps on large levels
        only); took(s): the return value that says which path ran at shape s"""
        self.method, self.tag, self.shapes, self.make, self.call = method, tag, shapes, make, call
        self.ins, self.batched, self.device_only = set(ins), tuple(batched), device_only
        self.env, self.took = dict(env or {}), took
        self.nd = nd or len(shapes[0])

    @property
    def id(self):
        return self.method + (f"[{self.tag}]" if self.tag else "")


TABLE = []
FAMILY = {}


def row(family, method, tag, shapes, make, call, ins, **kw):
    r = Row(method, tag, shapes, make, call, ins, **kw)
    TABLE.append(r)
    FAMILY.setdefault(family, []).append(r)


_CACHE = {}


def cached(key, fn):
    """set-up products computed once on plain arrays and shared (never modified: every use copies)"""
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def U(shape, seed, lo=-1.0, hi=1.0):
    return pb.uniform(shape, seed, lo, hi)


def stack(g, seed, n=NRHS + 1):
    return np.stack([U(g, seed + 17 * m) for m in range(n)])


# ---------------------------------------------------------------- shared inputs
def op(s, nst, ghosts=True, per=None):
    """ghosts: non-zero ghost entries (sweeps, residuals, transfers read none or must ignore them); per: the periodic
    image in the wrapped ghost layers, zeros on the Dirichlet sides"""
    g = G(s)
    if per is not None:
        return (pb.periodic_random_op(s[0], s[1], nst, per, 31) if len(s) == 2
                else pb.periodic_random_op3(s[0], s[1], s[2], nst, per, 31))
    return pb.random_op(g, nst, 31 + nst, zero_ghost=not ghosts)


PER2 = {1: (False, True), 2: (True, False), 3: (True, True)}


def the_op(s, nst, ibc):
    if not ibc:
        return op(s, nst)
    return op(s, nst, per=PER2[ibc] if len(s) == 2 else pb.per3_of(ibc))


def sig(so):
    """names an operator in a cache key"""
    return so.shape, hash(so.tobytes())


def recip(K, so):
    def f():
        sor = np.zeros((2,) + so.shape[1:])
        (K.setup_recip2 if so.ndim == 3 else K.setup_recip3)(so, sor)
        return sor
    return cached(("recip", sig(so)), f)


def lines(K, so, d, ibc=0):
    def f():
        sl = np.zeros((2,) + so.shape[1:])
        K.setup_lines2(so, sl, d, ibc)
        return sl
    return cached(("lines", d, ibc, sig(so)), f)


def interp(K, so, s, ibc=0):
    def f():
        ci = np.zeros(((8 if len(s) == 2 else 26),) + GC(s))
        (K.setup_interp2 if len(s) == 2 else K.setup_interp3)(so, ci, ibc)
        return ci
    return cached(("interp", ibc, sig(so)), f)


# ---------------------------------------------------------------- 2D and 3D point kernels
def mk_relax(nst, ibc=0, many=False, setup=recip):
    def make(K, s):
        so = the_op(s, nst, ibc)
        g = G(s)
        return dict(so=so, qf=stack(g, 41) if many else U(g, 41), q=stack(g, 42) if many else U(g, 42), sor=setup(K, so))
    return make


def mk_resid(nst, many=False):
    def make(K, s):
        g = G(s)
        return dict(so=op(s, nst), qf=stack(g, 41) if many else U(g, 41), q=stack(g, 42) if many else U(g, 42),
                    res=stack(g, 43) if many else np.zeros(g))
    return make


def both(f):
    """a DOWN and an UP sweep in one call; the return values as a tuple"""
    return lambda K, v: (f(K, v, DOWN), f(K, v, UP))


for nst in (3, 5):
    t = f"{2 * nst - 1}pt"
    row("point2", "setup_recip2", t, S2, lambda K, s, nst=nst: dict(so=op(s, nst), sor=np.zeros((2,) + G(s))),
        lambda K, v: K.setup_recip2(v["so"], v["sor"]), ["so"])
    for ibc in (0, 3):
        row("point2", "relax2", f"{t},ibc{ibc}", S2 if not ibc else S2_PER, mk_relax(nst, ibc),
            both(lambda K, v, ud, ibc=ibc: K.relax2(v["so"], v["qf"], v["q"], v["sor"], ud, ibc)), ["so", "qf", "sor"])
    row("point2", "relax2_op32", t, S2, mk_relax(nst),
        both(lambda K, v, ud: K.relax2_op32(v["so"], v["qf"], v["q"], v["sor"], ud)), ["so", "qf", "sor"])
    row("point2", "residual2", t, S2, mk_resid(nst), lambda K, v: K.residual2(v["so"], v["qf"], v["q"], v["res"]),
        ["so", "qf", "q"])
    row("point2", "residual2_op32", t, S2, mk_resid(nst), lambda K, v: K.residual2_op32(v["so"], v["qf"], v["q"], v["res"]),
        ["so", "qf", "q"])
    row("point2", "matvec2", t, S2, mk_resid(nst), lambda K, v: K.matvec2(v["so"], v["q"], v["res"]), ["so", "qf", "q"])
    row("many2", "relax2_many_op32", t, S2, mk_relax(nst, many=True),
        both(lambda K, v, ud: K.relax2_many_op32(v["so"], v["qf"], v["q"], v["sor"], ud, nrhs=NRHS)), ["so", "qf", "sor"],
        batched=["q"])
    row("many2", "residual2_many_op32", t, S2, mk_resid(nst, many=True),
        lambda K, v: K.residual2_many_op32(v["so"], v["qf"], v["q"], v["res"], nrhs=NRHS), ["so", "qf", "q"], batched=["res"])
    for ibc in (1, 3):
        row("many2", "relax2_periodic_many", f"{t},ibc{ibc}", S2_PER, mk_relax(nst, ibc, many=True),
            both(lambda K, v, ud, ibc=ibc: K.relax2_periodic_many(v["so"], v["qf"], v["q"], v["sor"], ud, ibc, nrhs=NRHS)),
            ["so", "qf", "sor"], batched=["q"])
row("point2", "relax2_psum", "", S2_PSUM, mk_relax(5),
    both(lambda K, v, ud: K.relax2_psum(v["so"], v["qf"], v["q"], v["sor"], ud)), ["so", "qf", "sor"])
row("point2", "relax2_psum_op32", "", S2_PSUM, mk_relax(5),
    both(lambda K, v, ud: K.relax2_psum_op32(v["so"], v["qf"], v["q"], v["sor"], ud)), ["so", "qf", "sor"])

for nst in (4, 14):
    t = f"{2 * nst - 1}pt"
    row("point3", "setup_recip3", t, S3, lambda K, s, nst=nst: dict(so=op(s, nst), sor=np.zeros((2,) + G(s))),
        lambda K, v: K.setup_recip3(v["so"], v["sor"]), ["so"])
    for ibc in (0, 3, 8):
        row("point3", "relax3", f"{t},ibc{ibc}", S3 if not ibc else S3_PER, mk_relax(nst, ibc),
            both(lambda K, v, ud, ibc=ibc: K.relax3(v["so"], v["qf"], v["q"], v["sor"], ud, ibc)), ["so", "qf", "sor"])
    row("point3", "residual3", t, S3, mk_resid(nst), lambda K, v: K.residual3(v["so"], v["qf"], v["q"], v["res"]),
        ["so", "qf", "q"])
    row("point3", "matvec3", t, S3, mk_resid(nst), lambda K, v: K.matvec3(v["so"], v["q"], v["res"]), ["so", "qf", "q"])
    row("many3", "relax3_many", t, S3, mk_relax(nst, many=True),
        both(lambda K, v, ud: K.relax3_many(v["so"], v["qf"], v["q"], v["sor"], ud, nrhs=NRHS)), ["so", "qf", "sor"],
        batched=["q"])
    row("many3", "residual3_many", t, S3, mk_resid(nst, many=True),
        lambda K, v: K.residual3_many(v["so"], v["qf"], v["q"], v["res"], nrhs=NRHS), ["so", "qf", "q"], batched=["res"])
    for ibc, gc in ((1, 0), (1, 1), (8, 0)):
        row("many3", "relax3_periodic_many", f"{t},ibc{ibc},gc{gc}", S3_PER, mk_relax(nst, ibc, many=True),
            both(lambda K, v, ud, ibc=ibc, gc=gc: K.relax3_periodic_many(v["so"], v["qf"], v["q"], v["sor"], ud, ibc, gc,
                                                                        nrhs=NRHS)),
            ["so", "qf", "sor"], batched=["q"])
# the same sweeps with the run lengths set as the existing tests set them (test_gpu_kernels.py: CEDAR_AMD_FRUN2 /
# CEDAR_AMD_FRUN = 2): the band-fused and partial-sum kernels, which the default switches keep for levels of 4096 rows
# (2D) and 160 rows (3D).  took: relax2_psum ran iff ny >= 8 * 2 and nx > 128, relax3_psum iff ny >= 4 * 2
# (test_partial_sum_relax9_... and test_partial_sum_relax_matches_... assert the same)
# relax2, relax3 and relax3_many return nothing, so for their rows the path is assumed, not asserted: the launchers'
# own rules (relax2d.hip band_frun: runs of 2 rows from ny >= 16 on rows of more than 128 points; relax3d.hip: the
# plane-fused walk from ny >= 8) name the fused kernels at (258, 33), (257, 34) and at (9, 17, 4), (130, 19, 3),
# (129, 16, 4) -- the second and third are shapes of test_gpu_kernels.py::test_plane_fused_relax_matches_four_pass_order
FRUN2, FRUN3 = {"CEDAR_AMD_FRUN2": "2"}, {"CEDAR_AMD_FRUN": "2"}
took2 = lambda s: (1, 1) if s[1] >= 16 and s[0] > 128 else (0, 0)
took3 = lambda s: (1, 1) if s[1] >= 8 else (0, 0)
row("point2", "relax2", "9pt,frun2=2", S2_PSUM, mk_relax(5),
    both(lambda K, v, ud: K.relax2(v["so"], v["qf"], v["q"], v["sor"], ud)), ["so", "qf", "sor"], env=FRUN2)
row("point2", "relax2_psum", "frun2=2", S2_PSUM, mk_relax(5),
    both(lambda K, v, ud: K.relax2_psum(v["so"], v["qf"], v["q"], v["sor"], ud)), ["so", "qf", "sor"], env=FRUN2, took=took2)
row("point2", "relax2_psum_op32", "frun2=2", S2_PSUM, mk_relax(5),
    both(lambda K, v, ud: K.relax2_psum_op32(v["so"], v["qf"], v["q"], v["sor"], ud)), ["so", "qf", "sor"], env=FRUN2, took=took2)
row("point3", "relax3", "27pt,frun=2", S3_PSUM, mk_relax(14),
    both(lambda K, v, ud: K.relax3(v["so"], v["qf"], v["q"], v["sor"], ud)), ["so", "qf", "sor"], env=FRUN3)
row("point3", "relax3_psum", "frun=2", S3_PSUM, mk_relax(14),
    both(lambda K, v, ud: K.relax3_psum(v["so"], v["qf"], v["q"], v["sor"], ud)), ["so", "qf", "sor"], env=FRUN3, took=took3)
row("many3", "relax3_many", "27pt,frun=2", S3_PSUM, mk_relax(14, many=True),
    both(lambda K, v, ud: K.relax3_many(v["so"], v["qf"], v["q"], v["sor"], ud, nrhs=NRHS)), ["so", "qf", "sor"],
    batched=["q"], env=FRUN3)
for name, nst, frun in (("relax3_psum", 14, None), ("relax3_op32", 14, 0), ("relax3_op32", 14, 2), ("relax7_op32", 4, None)):
    def call(K, v, ud, name=name, frun=frun):
        f = getattr(K, name)
        return f(v["so"], v["qf"], v["q"], v["sor"], ud) if frun is None else f(v["so"], v["qf"], v["q"], v["sor"], ud, frun)
    row("point3", name, "" if frun is None else f"frun{frun}", S3 + S3_PSUM if nst == 14 else S3, mk_relax(nst), both(call),
        ["so", "qf", "sor"])
for name, nst in (("residual3_op32", 14), ("residual7_op32", 4)):
    row("point3", name, "", S3, mk_resid(nst),
        lambda K, v, name=name: getattr(K, name)(v["so"], v["qf"], v["q"], v["res"]), ["so", "qf", "q"])
for name, nst in (("relax3_many_op32", 14), ("relax7_many_op32", 4)):
    row("many3", name, "", S3, mk_relax(nst, many=True),
        both(lambda K, v, ud, name=name: getattr(K, name)(v["so"], v["qf"], v["q"], v["sor"], ud, nrhs=NRHS)),
        ["so", "qf", "sor"], batched=["q"])
for name, nst in (("residual3_many_op32", 14), ("residual7_many_op32", 4)):
    row("many3", name, "", S3, mk_resid(nst, many=True),
        lambda K, v, name=name: getattr(K, name)(v["so"], v["qf"], v["q"], v["res"], nrhs=NRHS), ["so", "qf", "q"],
        batched=["res"])


# ---------------------------------------------------------------- line kernels
for nst in (3, 5):
    t = f"{2 * nst - 1}pt"
    for d in "xy":
        for ibc in (0, 3):
            shapes = S2_LINES if not ibc else S2_PER
            row("lines", "setup_lines2", f"{t},{d},ibc{ibc}", shapes,
                lambda K, s, nst=nst, ibc=ibc: dict(so=the_op(s, nst, ibc), sor=np.zeros((2,) + G(s))),
                lambda K, v, d=d, ibc=ibc: K.setup_lines2(v["so"], v["sor"], d, ibc), ["so"])
            row("lines", "relax_lines2", f"{t},{d},ibc{ibc}", shapes,
                mk_relax(nst, ibc, setup=lambda K, so, d=d, ibc=ibc: lines(K, so, d, ibc)),
                both(lambda K, v, ud, d=d, ibc=ibc: K.relax_lines2(v["so"], v["qf"], v["q"], v["sor"], ud, d, ibc)),
                ["so", "qf", "sor"])
        dd = "xy".index(d)
        row("lines", "relax2_lines_op32", f"{t},{d}", S2_LINES, mk_relax(nst, setup=lambda K, so, d=d: lines(K, so, d)),
            both(lambda K, v, ud, dd=dd: K.relax2_lines_op32(v["so"], v["qf"], v["q"], v["sor"], dd, ud)), ["so", "qf", "sor"])
        row("lines", "relax2_lines_many_op32", f"{t},{d}", S2_LINES,
            mk_relax(nst, many=True, setup=lambda K, so, d=d: lines(K, so, d)),
            both(lambda K, v, ud, dd=dd: K.relax2_lines_many_op32(v["so"], v["qf"], v["q"], v["sor"], dd, ud, nrhs=NRHS)),
            ["so", "qf", "sor"], batched=["q"])


# ---------------------------------------------------------------- grid transfers and set-up
def mk_transfer(nst, ibc=0, many=False):
    def make(K, s):
        g, gc = G(s), GC(s)
        so = the_op(s, nst, ibc)
        ci = interp(K, so, s, ibc)
        mk = (lambda shp, sd: np.stack([U(shp, sd + 17 * m) for m in range(NRHS + 1)])) if many else U
        return dict(q=mk(g, 51), qc=mk(gc, 52), res=mk(g, 53), so=so, ci=ci)
    return make


for nd, S, SP, stencils, ibcs in ((2, S2, S2_PER, (3, 5), (0, 3)), (3, S3, S3_PER, (4, 14), (0, 1, 8))):
    fam = f"transfer{nd}"
    for nst in stencils:
        t = f"{2 * nst - 1}pt"
        for ibc in ibcs:
            shapes = S if not ibc else SP
            tt = f"{t},ibc{ibc}"
            # the periodic restriction refreshes the ghosts of the fine vector first: q is written too
            row(fam, f"restrict{nd}", tt, shapes, mk_transfer(nst, ibc),
                lambda K, v, nd=nd, ibc=ibc: getattr(K, f"restrict{nd}")(v["q"], v["qc"], v["ci"], ibc),
                ["ci", "so", "res"] + ([] if ibc else ["q"]))
            if nd == 2:
                row(fam, "interp_add2", tt, shapes, mk_transfer(nst, ibc),
                    lambda K, v, ibc=ibc: K.interp_add2(v["q"], v["qc"], v["res"], v["so"], v["ci"], ibc), ["so", "ci"])
            else:
                row(fam, "interp_add3", tt, shapes, mk_transfer(nst, ibc),
                    lambda K, v, ibc=ibc: K.interp_add3(v["q"], v["qc"], v["so"], v["res"], v["ci"], ibc), ["so", "ci"])
            row(f"setup{nd}", f"setup_interp{nd}", tt, shapes,
                lambda K, s, nst=nst, ibc=ibc, nd=nd: dict(so=the_op(s, nst, ibc) if ibc else op(s, nst, ghosts=False),
                                                         ci=np.zeros(((8 if nd == 2 else 26),) + GC(s))),
                lambda K, v, nd=nd, ibc=ibc: getattr(K, f"setup_interp{nd}")(v["so"], v["ci"], ibc), ["so"])

            def mk_gal(K, s, nst=nst, ibc=ibc, nd=nd):
                so = the_op(s, nst, ibc) if ibc else op(s, nst, ghosts=False)
                return dict(so=so, soc=np.zeros(((5 if nd == 2 else 14),) + GC(s)), ci=interp(K, so, s, ibc))
            row(f"setup{nd}", f"galerkin{nd}", tt, shapes, mk_gal,
                lambda K, v, nd=nd, ibc=ibc: getattr(K, f"galerkin{nd}")(v["so"], v["soc"], v["ci"], ibc), ["so", "ci"])
        row(fam, f"restrict{nd}_ci32", t, S, mk_transfer(nst),
            lambda K, v, nd=nd: getattr(K, f"restrict{nd}_ci32")(v["q"], v["qc"], v["ci"]), ["ci", "so", "res", "q"])
        if nd == 2:
            row(fam, "interp_add2_ci32", t, S, mk_transfer(nst),
                lambda K, v: K.interp_add2_ci32(v["q"], v["qc"], v["res"], v["so"], v["ci"]), ["so", "ci"])
            for ibc in (2, 3):
                row("many2", "restrict2_periodic_many", f"{t},ibc{ibc}", S2_PER, mk_transfer(nst, ibc, many=True),
                    lambda K, v, ibc=ibc: K.restrict2_periodic_many(v["q"], v["qc"], v["ci"], ibc, nrhs=NRHS),
                    ["ci", "so", "res"], batched=["q", "qc"])
                row("many2", "interp_add2_periodic_many", f"{t},ibc{ibc}", S2_PER, mk_transfer(nst, ibc, many=True),
                    lambda K, v, ibc=ibc: K.interp_add2_periodic_many(v["q"], v["qc"], v["res"], v["so"], v["ci"], ibc,
                                                                      nrhs=NRHS), ["so", "ci"], batched=["q", "res"])
        else:
            row(fam, "interp_add3_ci32", t, S, mk_transfer(nst),
                lambda K, v: K.interp_add3_ci32(v["q"], v["qc"], v["so"], v["res"], v["ci"]), ["so", "ci"])
            for sfx in ("", "_ci32"):
                row("many3", "restrict3_many" + sfx, t, S3, mk_transfer(nst, many=True),
                    lambda K, v, sfx=sfx: getattr(K, "restrict3_many" + sfx)(v["q"], v["qc"], v["ci"], nrhs=NRHS),
                    ["ci", "so", "res", "q"], batched=["qc"])
                row("many3", "interp_add3_many" + sfx, t, S3, mk_transfer(nst, many=True),
                    lambda K, v, sfx=sfx: getattr(K, "interp_add3_many" + sfx)(v["q"], v["qc"], v["so"], v["res"], v["ci"],
                                                                               nrhs=NRHS), ["so", "ci"], batched=["q", "res"])
            for ibc in (1, 8):
                row("many3", "restrict3_periodic_many", f"{t},ibc{ibc}", S3_PER, mk_transfer(nst, ibc, many=True),
                    lambda K, v, ibc=ibc: K.restrict3_periodic_many(v["q"], v["qc"], v["ci"], ibc, nrhs=NRHS),
                    ["ci", "so", "res"], batched=["q", "qc"])
                row("many3", "interp_add3_periodic_many", f"{t},ibc{ibc}", S3_PER, mk_transfer(nst, ibc, many=True),
                    lambda K, v, ibc=ibc: K.interp_add3_periodic_many(v["q"], v["qc"], v["so"], v["res"], v["ci"], ibc,
                                                                      nrhs=NRHS), ["so", "ci"], batched=["q", "res"])


# ---------------------------------------------------------------- coarse factor and solve
def abd_shape(s, ibc):
    n = int(np.prod(s))
    if ibc:
        return (n, n)
    return (n, s[0] + 2) if len(s) == 2 else (n, s[0] * (s[1] + 1) + 2)


def cg_op(s, nst, ibc):
    if not ibc:
        return op(s, nst, ghosts=False)
    so = the_op(s, nst, ibc).copy()
    so[0] *= 4.0  # keeps the wrapped matrix positive definite (cases.coarse_solve_per)
    return so


def factor(K, so, s, ibc):
    def f():
        abd = np.zeros(abd_shape(s, ibc))
        (K.setup_cg2 if len(s) == 2 else K.setup_cg3)(so, abd, ibc)
        return abd
    return cached(("abd", ibc, sig(so)), f)


for nd, S, SP, stencils, ibcs in ((2, S2_CG, S2_CGPER, (3, 5), (0, 3)), (3, S3_CG, S3_CGPER, (4, 14), (0, 2))):
    for nst in stencils:
        for ibc in ibcs:
            if nd == 3 and ibc and nst == 4:
                continue  # the dense periodic 3D assembly is tested on the 27-point stencil (cases.CG_PER3)
            shapes = S if not ibc else SP
            tt = f"{2 * nst - 1}pt,ibc{ibc}"
            row("coarse", f"setup_cg{nd}", tt, shapes,
                lambda K, s, nst=nst, ibc=ibc: dict(so=cg_op(s, nst, ibc), abd=np.zeros(abd_shape(s, ibc))),
                lambda K, v, nd=nd, ibc=ibc: getattr(K, f"setup_cg{nd}")(v["so"], v["abd"], ibc), ["so"], nd=nd)

            def mk_solve(K, s, nst=nst, ibc=ibc, many=False):
                so = cg_op(s, nst, ibc)
                g = G(s)
                return dict(q=stack(g, 61) if many else U(g, 61), qf=stack(g, 62) if many else U(g, 62),
                            abd=factor(K, so, s, ibc))
            row("coarse", f"solve_cg{nd}", tt, shapes, mk_solve,
                lambda K, v, nd=nd, ibc=ibc: getattr(K, f"solve_cg{nd}")(v["q"], v["qf"], v["abd"], ibc), ["qf", "abd"], nd=nd)
            if ibc:
                row("coarse", f"solve_cg{nd}_periodic_many", tt, shapes,
                    lambda K, s, mk=mk_solve: mk(K, s, many=True),
                    lambda K, v, nd=nd, ibc=ibc: getattr(K, f"solve_cg{nd}_periodic_many")(v["q"], v["qf"], v["abd"], ibc,
                                                                                          nrhs=NRHS),
                    ["qf", "abd"], nd=nd, batched=["q"])


# ---------------------------------------------------------------- plane relaxation
for d in ("xy", "xz", "yz"):
    for nst in (4, 14):
        row("planes", "relax_planes3", f"{2 * nst - 1}pt,{d}", [(3, 3, 3), (4, 5, 3), (9, 4, 5)],
            lambda K, s, nst=nst: dict(so=op(s, nst, ghosts=False), x=U(G(s), 71), b=U(G(s), 72)),
            both(lambda K, v, ud, d=d: K.relax_planes3(v["so"], v["x"], v["b"], d, ud)), ["so", "b"])


# ---------------------------------------------------------------- Krylov passes
def sc_block(n=None):
    """the PCG_NSC = 8 scalars (common.h PCG_*: rho, sigma, alpha, beta, r.r, r.z, flag): marks in the slots a pass may
    leave alone, so that a pass that writes one it should not shows"""
    sc = np.array([3.0, 101.0, 0.5, 0.3717, 104.0, 105.0, 0.0, 0.0])
    if n is None:
        return sc
    return np.stack([sc * np.array([1.0 + m, 1.0, 1.0 - 0.25 * m, 1.0 + 0.5 * m, 1.0, 1.0, 1.0, 1.0]) for m in range(n)])


def mk_dir(nst, many=False, ibc=0):
    def make(K, s):
        g = G(s)
        mk = stack if many else U
        return dict(so=the_op(s, nst, ibc), z=mk(g, 81), p=mk(g, 82), pn=mk(g, 83), w=mk(g, 84),
                    sc=sc_block(NRHS + 1 if many else None))
    return make


def mk_upd(many=False):
    def make(K, s):
        g = G(s)
        mk = stack if many else U
        return dict(x=mk(g, 85), r=mk(g, 86), p=mk(g, 87), w=mk(g, 88), z=mk(g, 89), diag=U(g, 90, 1.0, 3.0),
                    sc=sc_block(NRHS + 1 if many else None))
    return make


DIRV = ["so", "z", "p"]
for nd, S, stencils, ibcs in ((2, S2_KRY, (3, 5), (3,)), (3, S3_KRY, (4, 14), (1, 8))):
    for nst in stencils:
        t = f"{2 * nst - 1}pt"
        for first in (0, 1):
            row("krylov", "pcg_direction", f"{t},first{first}", S, mk_dir(nst),
                lambda K, v, first=first: K.pcg_direction(v["so"], v["z"], v["p"], v["pn"], v["w"], first, v["sc"]), DIRV)
            row("krylov", "pcg_direction_many", f"{t},first{first}", S, mk_dir(nst, many=True),
                lambda K, v, first=first: K.pcg_direction_many(v["so"], v["z"], v["p"], v["pn"], v["w"], first, v["sc"],
                                                              nrhs=NRHS), DIRV, batched=["pn", "w", "sc"])
        for ibc in ibcs:
            SP = S2_PER if nd == 2 else S3_PER
            row("krylov", "pcg_direction_periodic", f"{t},ibc{ibc}", SP, mk_dir(nst, ibc=ibc),
                lambda K, v, ibc=ibc: K.pcg_direction_periodic(v["so"], v["z"], v["p"], v["pn"], v["w"], ibc, 0, v["sc"]), DIRV)
            name = "pcg_direction2_periodic_many" if nd == 2 else "pcg_direction_periodic_many"
            row("krylov", name, f"{t},ibc{ibc}", SP, mk_dir(nst, many=True, ibc=ibc),
                lambda K, v, ibc=ibc, name=name: getattr(K, name)(v["so"], v["z"], v["p"], v["pn"], v["w"], ibc, 0, v["sc"],
                                                                 nrhs=NRHS), DIRV, batched=["pn", "w", "sc"])
    for zmode, move in ((0, 1), (1, 1), (2, 0), (3, 1)):
        t = f"{nd}d,zmode{zmode},move{move}"

        def upd_args(v, zmode=zmode, move=move):
            """as test_gpu_krylov.py::check_update passes them: x, p, w only when moving, z for zmode 1 (written) and 2
            (read), the diagonal for zmode 1"""
            x, p, w = (v["x"], v["p"], v["w"]) if move else (None, None, None)
            return (zmode, move, x, v["r"], p, w, v["z"] if zmode in (1, 2) else None, v["diag"] if zmode == 1 else None)
        row("krylov", "pcg_update", t, S, mk_upd(), lambda K, v, a=upd_args: K.pcg_update(*a(v), 0, v["sc"]),
            ["p", "w", "diag"] + (["z"] if zmode == 2 else []))
        row("krylov", "pcg_update_many", t, S, mk_upd(many=True),
            lambda K, v, a=upd_args: K.pcg_update_many(*a(v), 0, v["sc"], nrhs=NRHS),
            ["p", "w", "diag"] + (["z"] if zmode == 2 else []), batched=["x", "r", "z", "sc"])
    row("krylov", "pcg_dots_wz", f"{nd}d", S, mk_upd(),
        lambda K, v: K.pcg_dots_wz(v["r"], v["z"], v["w"], 0, v["sc"]), ["r", "z", "w", "x", "p", "diag"])
    row("krylov", "pcg_dots_wz_many", f"{nd}d", S, mk_upd(many=True),
        lambda K, v: K.pcg_dots_wz_many(v["r"], v["z"], v["w"], 0, v["sc"], nrhs=NRHS), ["r", "z", "w", "x", "p", "diag"],
        batched=["sc"])
    row("krylov", "project_mean", f"{nd}d", S, lambda K, s: dict(v=U(G(s), 91)), lambda K, v: K.project_mean(v["v"]), [])
    row("krylov", "project_mean", f"{nd}d,many", S, lambda K, s: dict(v=stack(G(s), 91)),
        lambda K, v: K.project_mean(v["v"], nrhs=NRHS), [], batched=["v"])
    row("krylov", "l2", f"{nd}d", S, lambda K, s: dict(v=U(G(s), 92)), lambda K, v: K.l2(v["v"]), ["v"])
for world, stride in ((1, 1), (3, 2), (8, 2)):
    row("krylov", "pcg_rank_scalars", f"world{world},stride{stride}", [(world, stride)],
        lambda K, s: dict(g=np.abs(U((s[0] * s[1],), 93)) + 0.5, sc=sc_block()),
        lambda K, v, world=world, stride=stride: (K.pcg_rank_scalars(0, 0, v["g"], world, stride, 0, v["sc"]),
                                                 K.pcg_rank_scalars(1, 0, v["g"], world, stride, 0, v["sc"])), ["g"], nd=2)


def shell_boxes(s):
    """one-cell faces, an edge and two corners of the ghost shell of a grid of s = (nx, ny, nz) owned points: every
    face of the array and its last element (boxes: i0, j0, k0, ni, nj, nk)"""
    nx, ny, nz = s
    return [[0, 1, 1, 1, ny, nz], [nx + 1, 1, 1, 1, ny, nz], [1, 0, 1, nx, 1, nz], [1, ny + 1, 1, nx, 1, nz],
            [1, 1, 0, nx, ny, 1], [1, 1, nz + 1, nx, ny, 1], [0, 0, 1, 1, 1, nz], [0, 0, 0, 1, 1, 1],
            [nx + 1, ny + 1, nz + 1, 1, 1, 1]]


for first in (0, 1):
    row("krylov", "pcg_ghost_shell", f"first{first}", S3_KRY,
        lambda K, s: dict(z=U(G(s), 94), p=U(G(s), 95), pn=U(G(s), 96), sc=sc_block()),
        lambda K, v, first=first: K.pcg_ghost_shell(v["z"], v["p"], v["pn"], first, v["sc"],
                                                    shell_boxes(tuple(n - 2 for n in reversed(v["z"].shape)))),
        ["z", "p", "sc"])


# ---------------------------------------------------------------- gallery
def mk_gallery(name):
    nst = {"poisson2": 3, "diag_diffusion2": 3, "fe2": 5, "poisson3": 4, "diag_diffusion3": 4, "fe3": 14}[name]
    return lambda K, s: dict(so=np.zeros((nst,) + G(s)), b=np.zeros(G(s)))


def call_gallery(name):
    """the call capi.gallery makes, on so and b of the arena (capi.gallery allocates its own); the views are zeroed first:
    an entry the generator does not set must come back a zero, not poison"""
    def call(K, v):
        from cedar_amd import capi
        which, _ = capi.GALLERY[name]
        g = v["b"].shape
        n = tuple(m - 2 for m in reversed(g))
        params = {"diag_diffusion2": [1.0, 1e-2], "diag_diffusion3": [1.0, 1e-2, 0.5]}.get(name)
        pp = (C.c_double * len(params))(*params) if params else None
        capi.lib.cedar_amd_gallery(which, capi._vp(v["so"]), capi._vp(v["b"]), n[0], n[1], n[2] if len(n) == 3 else 1, pp)
    return call


for name in ("poisson2", "diag_diffusion2", "fe2", "poisson3", "diag_diffusion3", "fe3"):
    row("gallery", "gallery", name, S2 if name.endswith("2") else S3, mk_gallery(name), call_gallery(name), [])


# ---------------------------------------------------------------- raw pieces of the domain-decomposed drivers
VP, CU = C.c_void_p, C.c_uint


def cfun(capi, name, restype, *argtypes):
    """a prototype of its own: the shared library object keeps the argument types other callers rely on"""
    return C.CFUNCTYPE(restype, *argtypes)((name, capi.lib))


def raw_ptr(a):
    return a.ptr if hasattr(a, "ptr") else a.ctypes.data


def dims3(a):
    return tuple(CU(n) for n in reversed(a.shape[-3:]))


def call_pass_part(K, v):
    """as test_gpu_kernels.py::test_partial_row_class_passes_compose_to_the_full_pass: interior rows then shell rows of
    every row class, both i-colour orders, faces -y and -z with a neighbour"""
    from cedar_amd import capi
    f = cfun(capi, "cedar_amd_relax3_pass_part", None, VP, VP, VP, VP, CU, CU, CU, C.c_int, C.c_int, C.c_int, C.c_int)
    for jb in (0, 1):
        for kb in (0, 1):
            for efirst in (0, 1):
                for part in (1, 2):
                    f(*(raw_ptr(v[k]) for k in ("so", "qf", "q", "sor")), *dims3(v["q"]), jb, kb, efirst, part | (5 << 4))


def call_planes(K, v):
    """as test_gpu_kernels.py::test_plane_parity_passes_compose_to_the_sweep: the two k-parities in sweep order, whole
    and as interior + shell planes, both directions"""
    from cedar_amd import capi
    f = cfun(capi, "cedar_amd_relax3_planes", None, VP, VP, VP, VP, CU, CU, CU, C.c_int, C.c_int, C.c_int)
    for up in (0, 1):
        for parts in ((0,), (1 | (4 << 4), 2 | (4 << 4))):
            for c in range(2):
                for part in parts:
                    f(*(raw_ptr(v[k]) for k in ("so", "qf", "q", "sor")), *dims3(v["q"]), c if up else 1 - c, up, part)


row("raw", "cedar_amd_relax3_pass_part", "", S3, mk_relax(14), call_pass_part, ["so", "qf", "sor"])
row("raw", "cedar_amd_relax3_planes", "", S3 + [(9, 17, 4)], mk_relax(14), call_planes, ["so", "qf", "sor"])
row("raw", "cedar_amd_relax3_planes", "frun=1", S3 + [(9, 17, 4)], mk_relax(14), call_planes, ["so", "qf", "sor"],
    env={"CEDAR_AMD_FRUN": "1"})


def mk_affine(K, s):
    """three lines with ld = n + 3 (test_gpu_line_exact.py): the lines are not 16-byte aligned, the arrays end with the
    last line's last element"""
    nlines, n = s
    ld = n + 3
    size = (nlines - 1) * ld + n
    return dict(y=U((size,), 111), a=U((size,), 112, -0.9, 0.9), div=U((size,), 113, 1.0, 2.0))


def call_affine(K, v):
    from cedar_amd import capi
    f = cfun(capi, "cedar_amd_affine_lines", None, VP, VP, VP, C.c_int, C.c_int, C.c_int, C.c_int)
    size = v["y"].shape[0]
    nlines = 3
    n = (size - (nlines - 1) * 3) // nlines
    f(v["y"].ptr, v["a"].ptr, v["div"].ptr, nlines, n, n + 3, 0)
    f(v["y"].ptr, v["a"].ptr, None, nlines, n, n + 3, 1)


row("raw", "cedar_amd_affine_lines", "", [(3, 1), (3, 5), (3, 600), (3, 2050)], mk_affine, call_affine, ["a", "div"], nd=2,
    device_only=True)


def nlines_of(g, d, lb):
    JJ, II = g
    return ((JJ - 2 - lb + 1) // 2) if d == 0 else ((II - 2 - lb + 1) // 2), (II - 2 if d == 0 else JJ - 2)


for nst in (3, 5):
    for d in (0, 1):
        for lb in (0, 1):
            def mk_rhs(K, s, nst=nst, d=d, lb=lb):
                g = G(s)
                nl, n = nlines_of(g, d, lb)
                return dict(so=op(s, nst), qf=U(g, 121), q=U(g, 122), out=U((nl, n), 123), p=U((nl, n), 125), c=U((nl,), 124))

            def call_rhs(K, v, nst=nst, d=d, lb=lb):
                """right-hand sides of the lines of one colour, the carry added to them, and the lines stored back"""
                from cedar_amd import capi
                JJ, II = v["q"].shape
                nl, n = v["out"].shape
                cfun(capi, "cedar_amd_lines_rhs2", None, VP, VP, VP, VP, CU, CU, C.c_int, C.c_int, C.c_int)(
                    v["so"].ptr, v["qf"].ptr, v["q"].ptr, v["out"].ptr, II, JJ, nst, d, lb)
                cfun(capi, "cedar_amd_lines_carry", None, VP, VP, VP, C.c_int, C.c_int, C.c_int)(
                    v["out"].ptr, v["p"].ptr, v["c"].ptr, nl, n, n)  # y[l][i] += p[l][i] * c[l]
                cfun(capi, "cedar_amd_lines_store2", None, VP, VP, CU, CU, C.c_int, C.c_int)(v["out"].ptr, v["q"].ptr, II, JJ, d, lb)
            row("raw", "cedar_amd_lines_rhs2", f"{2 * nst - 1}pt,dir{d},lb{lb}", [(3, 3), (10, 3), (9, 4), (258, 3), (4, 257)],
                mk_rhs, call_rhs, ["so", "qf", "c", "p"], device_only=True)


def copy_boxes(s, strided):
    """boxes that touch every face of the array, its first and its last element"""
    nx, ny, nz = s
    II, JJ, KK = nx + 2, ny + 2, nz + 2
    boxes = [[0, 0, 0, 1, JJ, KK], [II - 1, 0, 0, 1, JJ, KK], [0, 0, 0, II, 1, KK], [0, JJ - 1, 0, II, 1, KK],
             [0, 0, 0, II, JJ, 1], [0, 0, KK - 1, II, JJ, 1], [II - 1, JJ - 1, KK - 1, 1, 1, 1], [1, 1, 1, nx, ny, nz]]
    if strided:  # rows j0 + j * sj, planes k0 + k * sk: every other row and plane, ending on the last ones
        boxes = [b + [1, 1] for b in boxes] + [[0, (JJ - 1) % 2, (KK - 1) % 2, II, (JJ + 1) // 2, (KK + 1) // 2, 2, 2]]
    return boxes


for strided in (0, 1):
    def mk_box(K, s, strided=strided):
        boxes = copy_boxes(s, strided)
        total = sum(b[3] * b[4] * b[5] for b in boxes)
        return dict(arr=U((2,) + G(s), 131), buf=U((2 * total,), 132), back=U((2,) + G(s), 133))

    def call_box(K, v, strided=strided):
        """pack two planes-stacks of arr into buf, unpack buf into another array"""
        from cedar_amd import capi
        KK, JJ, II = v["arr"].shape[-3:]
        boxes = copy_boxes((II - 2, JJ - 2, KK - 2), strided)
        sizes = [b[3] * b[4] * b[5] for b in boxes]
        offs = [sum(sizes[:i]) for i in range(len(sizes))]
        w = 8 if strided else 6
        tb = (C.c_int * (w * len(boxes)))(*[x for b in boxes for x in b])
        to = (C.c_ulonglong * len(boxes))(*offs)
        f = cfun(capi, "cedar_amd_box_copy_strided" if strided else "cedar_amd_box_copy", None, VP, CU, CU, CU, C.c_int, C.c_int,
                 VP, VP, VP, C.c_int)
        f(v["arr"].ptr, II, JJ, KK, 2, len(boxes), C.addressof(tb), C.addressof(to), v["buf"].ptr, 0)
        f(v["back"].ptr, II, JJ, KK, 2, len(boxes), C.addressof(tb), C.addressof(to), v["buf"].ptr, 1)
    row("raw", "cedar_amd_box_copy_strided" if strided else "cedar_amd_box_copy", "", S3, mk_box, call_box, ["arr"],
        device_only=True)


# ---------------------------------------------------------------- the runner
@contextlib.contextmanager
def switches(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run_row(capi, K, r, s, placement, poison):
    with switches(r.env):
        return _run_row(capi, K, r, s, placement, poison)


def _run_row(capi, K, r, s, placement, poison):
    """[] or the list of what is wrong with row r at shape s"""
    init = cached(("init", r.id, s), lambda: r.make(K, s))
    try:
        if r.device_only:  # the piece takes device pointers only: the plain call runs on plain DeviceArrays
            dev = {k: capi.DeviceArray.from_numpy(a) for k, a in init.items()}
            try:
                rc_want = r.call(K, dev)
                capi.sync()
                want = {k: d.numpy() for k, d in dev.items()}
            finally:
                for d in dev.values():
                    d.free()
        else:
            want = {k: a.copy() for k, a in init.items()}
            rc_want = r.call(K, want)
    except RuntimeError:
        return [f"{r.id} {s}: the plain call is refused -- the row must name a case the library serves"]
    if any(isinstance(c, int) and c < 0 for c in (rc_want if isinstance(rc_want, tuple) else (rc_want,))):
        return [f"{r.id} {s}: the plain call returned {rc_want!r} -- the row must name a case the library serves"]
    if r.took is not None and rc_want != r.took(s):
        return [f"{r.id} {s}: the plain call returned {rc_want!r}, not {r.took(s)!r}: another path ran than the row is for"]
    if len(r.ins) < len(init) and all(gd.same_bits(want[k], init[k]) for k in init):
        return [f"{r.id} {s}: the plain call changed no array -- the row checks nothing"]
    ar = gd.Arena([(k, a.shape) for k, a in init.items()], gd.POISONS[poison], placement, r.nd)
    bad = []
    try:
        for k, a in init.items():
            ar.fill(k, a)
        try:
            rc = r.call(K, ar.views)
        except RuntimeError as e:
            rc = e
        capi.sync()
        try:
            ar.check()
        except AssertionError as e:
            bad.append(str(e))
        for k in init:
            got = ar.array(k)
            if not gd.same_bits(got, want[k]):
                d = np.flatnonzero(gd.bits(got).ravel() != gd.bits(want[k]).ravel())
                bad.append(f"array '{k}' differs from the plain call at {d.size} of {got.size} elements, first at "
                           f"{np.unravel_index(int(d[0]), got.shape)}: {got.ravel()[d[0]]!r} for {want[k].ravel()[d[0]]!r}")
            if k in r.ins and not gd.same_bits(want[k], init[k]):
                bad.append(f"input '{k}' was written by the plain call")
            if k in r.batched and not gd.same_bits(got[NRHS:], init[k][NRHS:]):
                bad.append(f"item {NRHS} of '{k}' (beyond nrhs) lost its bits")
        same_rc = (gd.same_bits(np.asarray(rc, dtype=np.float64), np.asarray(rc_want, dtype=np.float64))
                   if not isinstance(rc, Exception) and rc is not None and rc_want is not None else rc is rc_want)
        if not same_rc:
            bad.append(f"returned {rc!r}, the plain call {rc_want!r}")
    finally:
        ar.close()
    return [f"{r.id} {s} {placement} {poison}: {b}" for b in bad]


@pytest.mark.parametrize("poison", sorted(gd.POISONS))
@pytest.mark.parametrize("placement", gd.PLACEMENTS)
@pytest.mark.parametrize("family", sorted(FAMILY))
def test_family_between_guard_bands(capi, K, family, placement, poison):
    bad = []
    for r in FAMILY[family]:
        if r.device_only and placement == "host":
            continue
        for s in r.shapes:
            bad += run_row(capi, K, r, s, placement, poison)
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:40])


# ---------------------------------------------------------------- the boundary-first pieces
@pytest.mark.parametrize("poison", sorted(gd.POISONS))
@pytest.mark.parametrize("placement", ["dev16", "dev8"])
@pytest.mark.parametrize("shape,strip", [((16, 24, 6), True), ((8, 16, 5), False)], ids=str)
def test_boundary_first_pieces_between_guard_bands(capi, K, monkeypatch, shape, strip, placement, poison):
    """cedar_amd_relax3_rows / _cols / _cols_strip / _planes_masked with cedar_amd_relax3_prepare on the view pointers, called
    as test_gpu_kernels.py::test_boundary_first_pieces_reorder_the_sweep_without_changing_it calls them (runs of two rows,
    neighbours on all four sides, both directions), and cedar_amd_relax3_strip_build into the caller's strips: q and the
    strips have the bits of the same calls on plain DeviceArrays, the inputs keep theirs, the bands their poison"""
    monkeypatch.setenv("CEDAR_AMD_FRUN", "2")
    nx, ny, nz = shape
    g = G(shape)
    II, JJ, KK = nx + 2, ny + 2, nz + 2
    I = C.c_int
    prepare = cfun(capi, "cedar_amd_relax3_prepare", I, VP, VP, CU, CU, CU)
    release = cfun(capi, "cedar_amd_relax3_release", None, VP)
    rows = cfun(capi, "cedar_amd_relax3_rows", None, VP, VP, VP, VP, CU, CU, CU, I, I, I, I, I)
    cols = cfun(capi, "cedar_amd_relax3_cols", None, VP, VP, VP, VP, CU, CU, CU, I, I, I, VP, I, I)
    cols_strip = cfun(capi, "cedar_amd_relax3_cols_strip", None, VP, VP, VP, VP, CU, CU, CU, I, I, I, VP, I, I)
    masked = cfun(capi, "cedar_amd_relax3_planes_masked", I, VP, VP, VP, VP, CU, CU, CU, I, I, CU, CU, VP)
    strip_doubles = cfun(capi, "cedar_amd_relax3_strip_doubles", C.c_size_t, CU, CU)
    strip_build = cfun(capi, "cedar_amd_relax3_strip_build", None, VP, VP, CU, CU, CU, I, VP)
    so = pb.random_op(g, 14, 91, zero_ghost=False)
    sor = recip(K, so)
    init = dict(so=so, sor=sor, qf=U(g, 92), q=U(g, 93))
    if strip:
        ns = int(strip_doubles(JJ, KK))
        init.update(strip_lo=np.zeros(ns), strip_hi=np.zeros(ns))

    def sweep(v):
        """boundary_first.chain_parity (dist3.cpp chain_parity without the exchanges), neighbours on -x, +x, -y, +y"""
        so_, sor_, qf_, q_ = (v[k].ptr for k in ("so", "sor", "qf", "q"))
        assert prepare(so_, sor_, II, JJ, KK) & 2
        try:
            if strip:
                for side, k in ((0, "strip_lo"), (1, "strip_hi")):
                    strip_build(so_, sor_, II, JJ, KK, side, v[k].ptr)

            def do_cols(jb, kb, cl, x0, x1):
                arr = (I * len(cl))(*cl)
                if strip:
                    cols_strip(v["strip_lo"].ptr, v["strip_hi"].ptr, qf_, q_, II, JJ, KK, jb, kb, len(cl), C.addressof(arr), x0, x1)
                else:
                    cols(so_, qf_, q_, sor_, II, JJ, KK, jb, kb, len(cl), C.addressof(arr), x0, x1)

            def do_rows(j0, jstep, nrj, kb, up):
                rows(so_, qf_, q_, sor_, II, JJ, KK, j0, jstep, nrj, kb, up)

            def do_masked(kb, up, mF, mS, skip):
                sk = (I * 3)(*skip)
                return masked(so_, qf_, q_, sor_, II, JJ, KK, kb, up, mF, mS, C.addressof(sk))

            for up in (False, True):
                for c in range(2):
                    assert bf.chain_parity(nx, ny, (1, 1, 1, 1), c if up else 1 - c, up, rows=do_rows, cols=do_cols,
                                           masked=do_masked) == 1
            capi.sync()
        finally:
            release(so_)

    dev = {k: capi.DeviceArray.from_numpy(a) for k, a in init.items()}
    try:
        sweep(dev)
        want = {k: d.numpy() for k, d in dev.items()}
    finally:
        for d in dev.values():
            d.free()
    assert not gd.same_bits(want["q"], init["q"])
    ar = gd.Arena([(k, a.shape) for k, a in init.items()], gd.POISONS[poison], placement, 3)
    try:
        for k, a in init.items():
            ar.fill(k, a)
        sweep(ar.views)
        ar.check()
        for k in init:
            assert gd.same_bits(ar.array(k), want[k]), f"'{k}' differs from the same calls on plain arrays"
        for k in ("so", "sor", "qf"):
            assert gd.same_bits(ar.array(k), init[k]), f"input '{k}' was written"
    finally:
        ar.close()


# ---------------------------------------------------------------- completeness
EXCLUDED = {}  # method name -> reason; a method that takes an array may not be excluded
# every parameter name of capi.Kernels' public methods, sorted into arrays and the rest; a name in neither set fails the
# test below until it is sorted, so a new array parameter cannot slip past the exclusion rule under another name
ARRAYS = {"abd", "b", "ci", "diag", "gathered", "p", "partial", "pn", "q", "qc", "qf", "r", "res", "sc", "so", "soc", "sor",
          "v", "w", "x", "z"}
NOT_ARRAYS = {"self", "updown", "ibc", "nrhs", "d", "dir", "frun", "plane", "first", "zmode", "move", "active", "which",
              "world", "stride", "boxes", "ghosts_consistent"}


def params(capi, name):
    return set(inspect.signature(getattr(capi.Kernels, name)).parameters)


def test_every_kernels_method_is_in_the_table():
    from cedar_amd import capi
    methods = [n for n, f in inspect.getmembers(capi.Kernels, callable) if not n.startswith("_")]
    assert len(methods) > 70
    in_table = {r.method for r in TABLE}
    missing = [n for n in methods if n not in in_table and n not in EXCLUDED]
    assert not missing, missing
    unsorted_ = {p for n in methods for p in params(capi, n)} - ARRAYS - NOT_ARRAYS
    assert not unsorted_, f"sort these parameter names into ARRAYS or NOT_ARRAYS: {sorted(unsorted_)}"
    assert all(params(capi, n) & ARRAYS for n in methods)  # today every method takes an array: none can be excluded
    for n in EXCLUDED:
        assert not params(capi, n) & ARRAYS, f"{n} takes an array: it may not be excluded"
    assert {r.tag for r in TABLE if r.method == "gallery"} == set(capi.GALLERY)
