"""GPU tests on operators that reach every regime of the interpolation set-up's lumping switch (problems.regime_op,
cases.REGIME_*; tests/test_oracle_regimes.py shows that they do).  The four device copies of the switch
(setup_interp.hip 2D and 3D, periodic2d.hip, periodic3d.hip) and every kernel that consumes their weights, through
the C ABI:
  * against golden vectors from the reference's Fortran (tests/golden/regimes_kernels_*.npz), with the rules of
    test_gpu_kernels.py / test_gpu_periodic*.py: interpolation set-up, relaxation, residual, restriction and
    interpolate-and-add bit for bit, 1e-13 of max-abs for the Galerkin product and the band Cholesky, 1e-12 for the
    scanned line solves;
  * against the oracle where there is no golden: rows longer than one block of the set-up kernels (256 lanes in 2D,
    128 in 3D), so that the data regime crosses a launch boundary;
  * the resident solver on the positive definite variant: hierarchy against the oracle, history against the
    reference's."""
import numpy as np
import pytest

import cases
from golden_io import load_split
from test_gpu_kernels import check
from test_oracle_periodic import EXACT as EXACT_PER, check_kernels
from test_oracle_periodic3d import EXACT as EXACT_PER3
from test_oracle_regimes import check_per3

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    from cedar_amd import capi
    assert capi.device_count() >= 1, "no GPU visible"
    return capi.Kernels()


@pytest.fixture(scope="module")
def greg():
    return load_split("regimes_kernels")


def check_all(case, out, gold):
    assert {k for k in gold if k.startswith(case[0] + "/")} == {f"{case[0]}/{k}" for k in out}
    for k, v in out.items():
        check(f"{case[0]}/{k}", v, gold[f"{case[0]}/{k}"])


@pytest.mark.parametrize("case", cases.REGIME_2D, ids=lambda c: c[0])
def test_regime_kernels_2d_vs_golden(K, greg, case):
    check_all(case, cases.regime_suite_2d(K, case), greg)


@pytest.mark.parametrize("case", cases.REGIME_3D, ids=lambda c: c[0])
def test_regime_kernels_3d_vs_golden(K, greg, case):
    check_all(case, cases.regime_suite_3d(K, case), greg)


@pytest.mark.parametrize("case", cases.REGIME_PER, ids=lambda c: c[0])
def test_regime_kernels_periodic_vs_golden(K, greg, case):
    check_kernels(case[0], cases.regime_suite_per(K, case), greg)


@pytest.mark.parametrize("case", cases.REGIME_PER3, ids=lambda c: c[0])
def test_regime_kernels_periodic3_vs_golden(K, greg, case):
    check_per3(case[0], cases.regime_suite_per3(K, case), greg)


# the coarse row (265 and 131 points) is longer than one block of the interpolation set-up kernels
LONG_2D = [(f"{n}.{v}", *c) for n, *c in [("b530x5_9", 530, 5, 5), ("b5x530_5", 5, 530, 3)] for v in ("mixed", "signed")]
LONG_3D = [(f"{n}.{v}", *c) for n, *c in [("b262x5x6_27", 262, 5, 6, 14), ("b262x6x5_7", 262, 6, 5, 4)]
           for v in ("mixed", "signed")]
LONG_PER = [(f"{n}.{v}", *c) for n, *c in [("c530x6_9_x", 530, 6, 5, 2), ("c6x530_5_xy", 6, 530, 3, 3)] for v in ("mixed", "signed")]
LONG_PER3 = [(f"{n}.{v}", *c) for n, *c in [("c262x4x6_27_x", 262, 4, 6, 14, 2), ("c262x6x6_7_yz", 262, 6, 6, 4, 7)]
             for v in ("mixed", "signed")]


@pytest.mark.parametrize("case", LONG_2D, ids=lambda c: c[0])
def test_regime_kernels_2d_long_rows_vs_oracle(K, oracle, case):
    got, want = cases.regime_suite_2d(K, case), cases.regime_suite_2d(oracle, case)
    assert set(got) == set(want)
    for k in want:
        check(f"{case[0]}/{k}", got[k], want[k])


@pytest.mark.parametrize("case", LONG_3D, ids=lambda c: c[0])
def test_regime_kernels_3d_long_rows_vs_oracle(K, oracle, case):
    got, want = cases.regime_suite_3d(K, case), cases.regime_suite_3d(oracle, case)
    assert set(got) == set(want)
    for k in want:
        check(f"{case[0]}/{k}", got[k], want[k])


@pytest.mark.parametrize("case", LONG_PER, ids=lambda c: c[0])
def test_regime_kernels_periodic_long_rows_vs_oracle(K, oracle, case):
    """the rules of test_gpu_periodic.test_periodic_kernels_vs_oracle"""
    with np.errstate(all="ignore"):
        got, want = cases.regime_suite_per(K, case), cases.regime_suite_per(oracle, case)
    for k in want:
        if k in EXACT_PER:
            assert np.array_equal(got[k], want[k]), (case[0], k, np.max(np.abs(got[k] - want[k])))
        else:
            assert np.max(np.abs(got[k] - want[k])) <= 1e-13 * np.max(np.abs(want[k])), (case[0], k)


@pytest.mark.parametrize("case", LONG_PER3, ids=lambda c: c[0])
def test_regime_kernels_periodic3_long_rows_vs_oracle(K, oracle, case):
    """the rules of test_gpu_periodic3d.test_periodic3_kernels_vs_oracle"""
    got, want = cases.regime_suite_per3(K, case), cases.regime_suite_per3(oracle, case)
    for k in want:
        if k in EXACT_PER3:
            assert np.array_equal(got[k], want[k]), (case[0], k, np.max(np.abs(got[k] - want[k])))
        else:
            assert np.max(np.abs(got[k] - want[k])) <= 1e-13 * np.max(np.abs(want[k])), (case[0], k)


@pytest.mark.parametrize("name", list(cases.REGIME_SOLVES), ids=str)
def test_regime_resident_solver(oracle, name):
    """device-resident solver on the positive definite variant (65x40 nine-point; 33x30x29 27-point and seven-point,
    the latter with 27-point coarse levels): level count and dims, A / P / SOR0 of every level against the oracle,
    residual history against the reference's (gen_golden.RefML) at rtol=1e-10, atol=1e-14.
    Hierarchy tolerance: the 1e-12 of max-abs of test_gpu_solver.test_hierarchy_vs_oracle for every array.  The oracle
    itself is at most 2.8e-15 from the reference hierarchy on these cases (measured on the CPU, per level and array
    in test_oracle_regimes.test_regime_solve_history_and_hierarchy), far below the 2.5e-13 above which an array
    would have been given four times the measured figure; nothing here is derived from a device result."""
    from cedar_amd import capi
    mk_op, mk_rhs, st = cases.REGIME_SOLVES[name]
    fx = load_split("regimes_hier_" + name.split(".")[0])
    so, b = mk_op(), mk_rhs()
    s = capi.Solver(so, **st)
    ml = oracle.ml_create(so, **st)
    try:
        assert s.nlevels() == ml.nlevels() == int(fx["nlev"])
        seen = 0
        for l in range(s.nlevels()):
            assert s.dims(l) == ml.dims(l)
            want = list(fx["level_dims"][l])
            assert [d + 2 for d in s.dims(l)][: len(want)] == want
            for what in ("A", "P", "SOR0"):
                w = ml.array(l, what)
                if w is None or (l == s.nlevels() - 1 and what == "SOR0"):
                    continue  # coarsest level has no relaxation set-up
                a = s.array(l, what)
                scale = np.max(np.abs(w)) + 1e-300
                dev = np.max(np.abs(a - w)) / scale
                print(name, l, what, "%.2e" % dev)
                assert dev <= 1e-12, (l, what, dev)
                seen += 1
        assert seen >= 3 * (s.nlevels() - 1)
        x = np.zeros_like(b)
        h = s.solve(b, x)
        print(name, "history deviation", np.abs(np.array(h) - fx["hist"][: len(h)]) / fx["hist"][: len(h)])
        assert len(h) == len(fx["hist"])
        np.testing.assert_allclose(h, fx["hist"], rtol=1e-10, atol=1e-14)
    finally:
        s.close()
        ml.close()
