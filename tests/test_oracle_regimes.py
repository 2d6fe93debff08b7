"""CPU tests on operators that reach every regime of the interpolation set-up's lumping switch
(problems.regime_op, cases.REGIME_*): the oracle against golden vectors from the reference's Fortran
(oracle/gen_golden.py regimes; tests/golden/regimes_*.npz), and checks that those inputs do leave the one regime
problems.random_op stays in.  Tolerances are those of test_oracle.py / test_oracle_periodic*.py: bit for bit where
the reference source fixes the arithmetic (the interpolation set-up among them), 1e-13 of max-abs for the rest."""
import numpy as np
import pytest

import cases
import problems as pb
from golden_io import load_split
from test_oracle import check
from test_oracle_periodic import check_kernels
from test_oracle_periodic3d import EXACT as EXACT_PER3


@pytest.fixture(scope="module")
def greg():
    return load_split("regimes_kernels")


def check_per3(name, got, gold):
    """the rules of test_oracle_periodic3d.check_kernels3 on a plain dict"""
    seen = 0
    for k, v in got.items():
        key = f"{name}/{k}"
        if key not in gold:  # interp_add for codes the reference leaves undefined
            assert k.startswith("interp_add"), key
            continue
        want = gold[key]
        seen += 1
        if k in EXACT_PER3:
            assert np.array_equal(v, want), (name, k, np.max(np.abs(v - want)))
        else:
            assert np.max(np.abs(v - want)) <= 1e-13 * np.max(np.abs(want)), (name, k)
    assert seen >= 2


def check_all(case, out, gold):
    """test_oracle.check on every array of a non-periodic suite; every golden array of the case is produced"""
    assert {k for k in gold if k.startswith(case[0] + "/")} == {f"{case[0]}/{k}" for k in out}
    for k, v in out.items():
        check(f"{case[0]}/{k}", v, gold[f"{case[0]}/{k}"])


@pytest.mark.parametrize("case", cases.REGIME_2D, ids=lambda c: c[0])
def test_regime_kernels_2d(oracle, greg, case):
    out = cases.regime_suite_2d(oracle, case)
    assert ("solve_cg" in out) == case[0].endswith(".spd")
    check_all(case, out, greg)


@pytest.mark.parametrize("case", cases.REGIME_3D, ids=lambda c: c[0])
def test_regime_kernels_3d(oracle, greg, case):
    check_all(case, cases.regime_suite_3d(oracle, case), greg)


@pytest.mark.parametrize("case", cases.REGIME_PER, ids=lambda c: c[0])
def test_regime_kernels_periodic(oracle, greg, case):
    with np.errstate(all="ignore"):  # the line factorisation of an indefinite operator stops early, as DPTTRF does
        out = cases.regime_suite_per(oracle, case)
    check_kernels(case[0], out, greg)


@pytest.mark.parametrize("case", cases.REGIME_PER3, ids=lambda c: c[0])
def test_regime_kernels_periodic3(oracle, greg, case):
    check_per3(case[0], cases.regime_suite_per3(oracle, case), greg)


# ---------------------------------------------------------------- the inputs do what they claim
ALL = cases.REGIME_2D + cases.REGIME_3D + cases.REGIME_PER + cases.REGIME_PER3


def layout(case):
    """(number of dimensions, ghosted shape, stencil size, periodic mask or None) of a case of any of the four lists"""
    nd = 3 if len(case) == 6 or (len(case) == 5 and case[0][0] == "g") else 2
    per = None
    if case[0][0] == "h":
        per = pb.per3_of(case[5]) if nd == 3 else {1: (0, 1), 2: (1, 0), 3: (1, 1)}[case[4]]
    return nd, tuple(m + 2 for m in case[1:nd + 1][::-1]), case[nd + 1], per


def interp_of(gold, name):
    return gold[f"{name}/interp"] if f"{name}/interp" in gold else gold[f"{name}/interp_interior"]


def xedge_shares(ci):
    """x-edge weight pairs (LL, LR / LXYL, LXYR) that are not both zero: (count, share with LL + LR within 1e-9 of 1,
    i.e. a row the switch treated as having zero row sum)"""
    a, b = ci[0].ravel(), ci[1].ravel()
    m = (a != 0) | (b != 0)
    return int(m.sum()), float(np.mean(np.abs((a + b)[m] - 1.0) <= 1e-9))


def test_every_golden_array_is_finite(greg):
    assert len(greg) > 400
    for k, v in greg.items():
        assert np.all(np.isfinite(v)), k
    for name in cases.REGIME_SOLVES:
        for k, v in load_split("regimes_hier_" + name.split(".")[0]).items():
            assert np.all(np.isfinite(v)), (name, k)


@pytest.mark.parametrize("case", [c for c in ALL if c[0].endswith(".mixed")], ids=lambda c: c[0])
def test_mixed_cases_have_lumped_and_dominant_rows(oracle, greg, case):
    """both branches of max(diag - (1+ep) S, 0) are taken by at least a tenth of the x-edge points (61 - 86 % are
    lumped on these cases); on problems.random_op at the same shape none is"""
    n, lumped = xedge_shares(interp_of(greg, case[0]))
    assert n >= 20
    assert 0.1 <= lumped <= 0.9, lumped
    nd, g, nst, _ = layout(case)
    so = pb.random_op(g, nst, cases._seed(case[0]))
    ci = np.zeros(((8 if nd == 2 else 26),) + pb.coarse_shape(g))
    (oracle.setup_interp2 if nd == 2 else oracle.setup_interp3)(so, ci)
    n0, lumped0 = xedge_shares(ci)
    assert n0 >= 20 and lumped0 == 0.0


@pytest.mark.parametrize("case", [c for c in cases.REGIME_3D if c[0].endswith("_27.scaled")], ids=lambda c: c[0])
def test_scale_decides_the_27_point_centre_minimum(greg, case):
    """two arguments of the 27-point centre minimum are not divided by the diagonal (as the reference has it), so
    scaling the operator by 2**-10 moves the eight corner weights at a good share of the cell centres (22 % and
    35 % here) and leaves the 18 edge and face slots alone"""
    ci, ci0 = greg[f"{case[0]}/interp"], greg[f"{case[0].replace('.scaled', '.mixed')}/interp"]
    centres = np.any(ci0[18:] != 0, axis=0)
    assert centres.sum() >= 200
    moved = np.max(np.abs(ci[18:] - ci0[18:]), axis=0)[centres] > 1e-6
    assert np.mean(moved) >= 0.1, np.mean(moved)
    assert np.max(np.abs(ci[:18] - ci0[:18])) < 1e-6


@pytest.mark.parametrize("case", [c for c in ALL if c[0].endswith(".signed")], ids=lambda c: c[0])
def test_signed_cases_have_a_negative_diagonal(greg, case):
    """read off the golden arrays: the reciprocal diagonal where there is one, else the operator that produced them"""
    if f"{case[0]}/recip" in greg:
        sor = greg[f"{case[0]}/recip"][1]  # SETUP_recip stores 1 / diagonal in the second plane (msor = 2)
        inner = sor[tuple(slice(1, -1) for _ in sor.shape)]
        assert np.any(inner < 0)
    nd, g, nst, per = layout(case)
    so = cases.regime_builder(case[0], per)(g, nst, cases._seed(case[0]))
    assert np.any(so[0][tuple(slice(1, -1) for _ in g)] < 0)


# ---------------------------------------------------------------- solves on the positive definite variant
@pytest.mark.parametrize("name", list(cases.REGIME_SOLVES), ids=str)
def test_regime_solve_history_and_hierarchy(oracle, name):
    """the oracle's V(2,1) solve against the history of the reference's kernels driven by gen_golden.RefML, at the
    rtol=1e-10, atol=1e-14 of test_oracle.test_solve_histories (largest relative deviation measured: 1.0e-9 at a
    relative residual of 2e-9, i.e. 2e-18 absolute, on g33x30x29_27), and its set-up products against the reference's.
    Measured deviation of the oracle from the reference hierarchy, as a share of the array's max-abs, largest over the
    levels (level-0 SOR0 and level-1 P are bit-identical in all three cases):
        g65x40_9      A 4.5e-16   P 1.9e-15   SOR0 4.0e-16
        g33x30x29_27  A 1.2e-15   P 1.3e-15   SOR0 5.5e-16
        g33x30x29_7   A 8.5e-16   P 2.8e-15   SOR0 1.4e-15
    All far below 2.5e-13, so tests/test_gpu_regimes.py holds the device hierarchy to the plain 1e-12 of
    test_hierarchy_vs_oracle.  Asserted here at 1e-13 (the Galerkin association, test_oracle.RTOL)."""
    mk_op, mk_rhs, st = cases.REGIME_SOLVES[name]
    fx = load_split("regimes_hier_" + name.split(".")[0])
    so, b = mk_op(), mk_rhs()
    ml = oracle.ml_create(so, **st)
    try:
        assert ml.nlevels() == int(fx["nlev"])
        for l in range(ml.nlevels()):
            nx, ny, nz = ml.dims(l)
            want = list(fx["level_dims"][l])
            assert [nx + 2, ny + 2, nz + 2][: len(want)] == want
        x = np.zeros_like(b)
        h = ml.solve(b, x, maxiter=10, tol=1e-8)
        assert len(h) == len(fx["hist"])
        np.testing.assert_allclose(h, fx["hist"], rtol=1e-10, atol=1e-14)
        assert abs(oracle.l2(x) - float(fx["x_l2"])) <= 1e-12 * float(fx["x_l2"])
        seen = 0
        for l in range(ml.nlevels()):
            for what, key in (("A", "A%d" % l), ("P", "P%d" % l), ("SOR0", "SOR0_%d" % l)):
                if key not in fx:
                    continue
                a, w = ml.array(l, what), fx[key]
                dev = np.max(np.abs(a - w)) / np.max(np.abs(w))
                print(name, l, what, "%.2e" % dev)
                assert dev <= 1e-13, (l, what, dev)
                seen += 1
        assert seen == 3 * (ml.nlevels() - 1)
    finally:
        ml.close()
