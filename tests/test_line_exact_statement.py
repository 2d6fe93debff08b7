"""The exact line-solve data of tests/line_exact.py, checked on the CPU: the sequential reference is the oracle bit for
bit on every case the GPU tests run (tests/test_gpu_line_exact.py), its exactness conditions hold, DPTTRF is exact on the
set-up operator, and a numpy restatement of the kernels' scan shows what the data is for: planted defects in the
multiplier half of the scan change values on this data and stay below the 1e-12 tolerance of the kernel tests on the
multipliers of problems.random_op."""
import numpy as np
import pytest

import line_exact as le
import problems as pb

DOWN, UP = 0, 1

# The lengths at which a planted defect can change a value at all.  Every line is entered with a zero carry, so a term
# that multiplies what came before is first non-trivial one step after the first non-zero value reaches it:
#   "ks"    from the third lane of a wavefront on: every length from 512 (64 lanes in use) is asserted
#   "wave"  the first hop of a chain multiplies the tile's incoming value, which is zero in the first tile, so the first
#           dropped non-zero term is the second hop of the third wavefront: unknowns from 1024 on, every length from
#           1025.  At 513 the one hop there is multiplies that zero
#   "tile"  what crossed a whole tile exists once a third tile does: unknowns from 4096 on, lengths 4097 and 4500
# Below these lengths the defective step multiplies an exact zero and no data can show it.
VISIBLE_FROM = {"ks": 512, "wave": 1025, "tile": 4097}


@pytest.mark.parametrize("dyadic", [False, True], ids=["unit", "dyadic"])
@pytest.mark.parametrize("d", ["x", "y"])
@pytest.mark.parametrize("n", le.LENGTHS)
def test_dirichlet_reference_is_the_oracle_bit_for_bit(oracle, n, d, dyadic):
    case = le.dirichlet_case(n, d, dyadic)
    assert case.nst == (5 if n <= 1030 else 3)
    f = le.factors_of(case)
    assert len(np.unique(f[0])) == (4 if dyadic else 1)
    for l in range(le.NLINES):
        assert np.array_equal(np.flatnonzero(f[1][l + 1, 2:n + 1] == 0.0), le.line_zeros(n, l))
    for ud in (DOWN, UP):
        want = le.sweep(case, ud)  # (asserts the exactness conditions)
        got = case.q0.copy()
        oracle.relax_lines2(case.so, case.qf, got, case.sor, ud, d)
        assert np.array_equal(got, want), (n, d, ud)
        assert not np.array_equal(want, case.q0)


@pytest.mark.parametrize("n", le.CYCLIC_LENGTHS)
@pytest.mark.parametrize("d,ibc", le.CYCLIC)
def test_cyclic_reference_is_the_oracle_bit_for_bit(oracle, d, ibc, n):
    for nst in (3, 5):
        case = le.cyclic_case(n, d, ibc, nst)
        stats = {}
        for ud in (DOWN, UP):
            want = le.sweep(case, ud, ibc, stats=stats)
            got = case.q0.copy()
            oracle.relax_lines2(case.so, case.qf, got, case.sor, ud, d, ibc)
            assert np.array_equal(got, want), (n, d, ibc, ud)
        assert stats["den"] > 0.0


@pytest.mark.parametrize("d", ["x", "y"])
@pytest.mark.parametrize("n", le.SETUP_LENGTHS)
def test_factorisation_is_exact_on_the_setup_operator(oracle, n, d):
    """pivots 2**k, multipliers -1, nothing else touched; and the sweep on those factors is the reference's"""
    case, want = le.setup_case(n, d)
    sor = np.zeros_like(want)
    oracle.setup_lines2(case.so, sor, d)
    assert np.array_equal(sor, want)
    f = le.factors_of(case._replace(sor=want))
    assert np.all(f[1][1:-1, 2:n + 1] == -1.0) and set(np.unique(f[0][1:-1, 1:n + 1])) == {0.5, 1.0, 2.0, 4.0}
    case = case._replace(sor=want)
    for ud in (DOWN, UP):
        got = case.q0.copy()
        oracle.relax_lines2(case.so, case.qf, got, want, ud, d)
        assert np.array_equal(got, le.sweep(case, ud))


@pytest.mark.parametrize("with_div", [False, True])
@pytest.mark.parametrize("n", le.AFFINE_LENGTHS)
def test_generic_recurrence_data_is_exact_under_the_scan(n, with_div):
    """the data of the cedar_amd_affine_lines test: the restated scan gives the sequential result on every line, and on the
    line without zero multipliers every planted defect changes a value from the length at which it can"""
    y, a, div = le.make_affine(n, 5000 + n, with_div)
    assert (np.any(a[2:, :n] == 0.0) or n < 512) and not np.any(a[0] == 0.0)
    for reverse in (0, 1):
        want = le.affine_reference(y, a, div, n, reverse)
        assert np.array_equal(want[:, n:], y[:, n:])
        for l in range(y.shape[0]):
            c = y[l, :n] / div[l, :n] if with_div else y[l, :n]
            cs, as_ = (c[::-1], a[l, :n][::-1]) if reverse else (c, a[l, :n])
            got = le.scan_restated(cs, as_, le.lanes_for(n))
            assert np.array_equal(got[::-1] if reverse else got, want[l, :n])
            if l == 0:
                for defect in le.DEFECTS:
                    bad = le.scan_restated(cs, as_, le.lanes_for(n), defect)
                    assert np.array_equal(bad, got) == (n < VISIBLE_FROM[defect]), (defect, n, reverse)


# ---------------------------------------------------------------- what the data is for
def test_restated_scan_is_the_sequential_recurrence_on_the_exact_data():
    for n in le.LENGTHS:
        case = le.dirichlet_case(n, "x")
        for fwd, bwd in le.sweep_recurrences(case):
            for c, a in (fwd, bwd):
                assert np.array_equal(le.scan_restated(c, a, le.lanes_for(n)), le.sequential(c, a)), n


@pytest.mark.parametrize("defect", le.DEFECTS)
def test_planted_defects_change_values_on_the_exact_data(defect):
    for n in le.LENGTHS:
        case = le.dirichlet_case(n, "x")
        recs = le.sweep_recurrences(case)
        for which in (0, 1):  # forward, backward
            changed = []
            for rec in recs:
                c, a = rec[which]
                got = le.scan_restated(c, a, le.lanes_for(n), defect)
                changed.append(not np.array_equal(got, le.sequential(c, a)))
            if n >= VISIBLE_FROM[defect]:
                # line 0 has no zero couplings; of the lines 2 and 4 at least the uncut sweep shows it too
                assert changed[0], (defect, n, which)
            else:
                assert not any(changed), (defect, n, which)


def test_carry_defects_are_invisible_on_random_op_multipliers(oracle):
    """the multipliers of problems.random_op, as the kernel tests build them (lines of 4500 unknowns, 256 lanes): the
    two carry defects move no unknown by 1e-12 of the largest, which is the tolerance of those tests"""
    n = 4500
    g = (3 + 2, n + 2)
    for nst in (3, 5):
        so = pb.random_op(g, nst, 871 + nst, zero_ghost=False)
        sor = np.zeros((2,) + g)
        oracle.setup_lines2(so, sor, "x")
        for row in (1, 2, 3):
            e = sor[1, row, 2:n + 1]
            assert np.max(np.abs(e)) < 0.15  # 0.5 .. 1.5 over a pivot of at least 12
            a = np.concatenate([[0.0], -e])
            c = pb.uniform((n,), 90 + row, -1, 1)
            ref = le.sequential(c, a)
            scale = np.max(np.abs(ref))
            assert np.max(np.abs(le.scan_restated(c, a, 256) - ref)) <= 1e-14 * scale
            for defect in ("wave", "tile"):
                dev = np.max(np.abs(le.scan_restated(c, a, 256, defect) - ref)) / scale
                assert dev < 1e-12, (defect, dev)
