"""The guard-band harness (tests/guarded.py) on the CPU: it passes what stays inside its arrays and it can fail.

1. The oracle's whole kernel set -- the 2D, 3D and periodic case suites of tests/cases.py -- run with every call's arrays
   inside a host arena, at both parities and with both poisons: bit-identical to the run on plain arrays, bands intact.
   So the reference order itself stays inside its arrays, and bit-identity is the right expectation for the device code.
2. numpy stand-ins with planted defects, written against a flat memory and element offsets the way a kernel sees its
   arguments: a store one element before an array, a store one row past the end, a load of the element after the last
   one times a zero coefficient, the same load dropped through a max.  The band check names each store by its array; the
   comparison with the plain call catches each consumed value under at least one poison -- the NaN is dropped by the max,
   which is why there are two.
"""
import numpy as np
import pytest

import cases
import guarded as gd
import problems as pb


# ---------------------------------------------------------------- 1. the oracle between guard bands
def _same(got, want, what):
    assert set(got) == set(want)
    for k in want:
        assert gd.same_bits(got[k], want[k]), f"{what}/{k}: differs from the run on plain arrays"


@pytest.mark.parametrize("placement", ["host", "host8"])
@pytest.mark.parametrize("poison", sorted(gd.POISONS))
def test_oracle_kernel_set_is_bit_identical_inside_an_arena(oracle, poison, placement):
    G = gd.GuardedImpl(oracle, gd.POISONS[poison], placement)
    for case in (("r9x9_5", 9, 9, 3), ("r7x10_9", 7, 10, 5), ("r16x12_9", 16, 12, 5)):
        _same(cases.kernel_suite_2d(G, case), cases.kernel_suite_2d(oracle, case), case[0])
    for case in (("r8x6x10_7", 8, 6, 10, 4), ("r8x6x10_27", 8, 6, 10, 14), ("r5x4x3_27", 5, 4, 3, 14)):
        _same(cases.kernel_suite_3d(G, case), cases.kernel_suite_3d(oracle, case), case[0])
    for case in (("p9x9_5_x", 9, 9, 3, 2), ("p6x7_9_xy", 6, 7, 5, 3), ("p8x8_5_y", 8, 8, 3, 1)):
        _same(cases.kernel_suite_per(G, case), cases.kernel_suite_per(oracle, case), case[0])
    for case in (("q6x4x8_27_xy", 6, 4, 8, 14, 3), ("q4x4x4_7_xyz", 4, 4, 4, 4, 8), ("q6x4x8_7_z", 6, 4, 8, 4, 5)):
        _same(cases.kernel_suite_per3(G, case), cases.kernel_suite_per3(oracle, case), case[0])
    for case in cases.CG_PER[:2]:
        _same(cases.coarse_solve_per(G, case), cases.coarse_solve_per(oracle, case), case[0])
    for case in cases.CG_PER3[:1]:
        _same(cases.coarse_solve_per3(G, case), cases.coarse_solve_per3(oracle, case), case[0])
    g = (5, 6, 7)
    so, x, b = pb.random_op(g, 14, 5), pb.uniform(g, 6, -1, 1), pb.uniform(g, 7, -1, 1)
    want = x.copy()
    oracle.relax_planes3(so, want, b, "xy", 0)
    G.relax_planes3(so, x, b, "xy", 0)
    assert gd.same_bits(x, want)
    assert G.calls > 100


def test_arena_layout():
    """band widths (two rows plus two in 2D, a plane plus a row plus two in 3D, of the larger neighbour, 64 at least) and
    the parity of every array's first element"""
    for placement, parity in (("host", 0), ("host8", 1)):
        for nd, specs in ((2, [("so", (5, 6, 40)), ("q", (6, 40)), ("sc", (8,))]),
                          (3, [("q", (3, 5, 9, 11)), ("so", (14, 5, 9, 11)), ("sc", (8,))])):
            ar = gd.Arena(specs, gd.POISON_NAN, placement, nd)
            need = 2 * specs[0][1][-1] + 2 if nd == 2 else specs[0][1][-2] * specs[0][1][-1] + specs[0][1][-1] + 2
            need = max(need, 64)
            names = [n for n, _ in specs]
            assert ar.start[names[0]] >= need
            assert ar.start[names[1]] - ar.stop[names[0]] >= need
            assert ar.start[names[2]] - ar.stop[names[1]] >= need
            assert ar.total - ar.stop[names[2]] >= 64
            for n in names:
                assert ar.start[n] % 2 == parity
            assert ar.clobbered() is None


# ---------------------------------------------------------------- 2. planted defects
# Stand-in "kernels" on a (JJ, II) grid, written against a flat memory and element offsets.  The sound ones:
#   "sum": res = qf - c q + coef * next(q), coef = 0 on the last point, which has no next neighbour and reads none;
#   "max": res = qf - c q + max(q, next(q)), the last point compared with itself.
def standin(mem, at, JJ, II, kind="sum", defect=None):
    n = JJ * II
    c, qf, q, res = (at[k] for k in ("c", "qf", "q", "res"))
    cur = mem[q:q + n]
    over = defect in ("load_after_times_zero", "load_after_through_max")
    nxt = mem[q + 1:q + n + 1] if over else np.concatenate([mem[q + 1:q + n], cur[-1:]])  # over: one element too many
    if kind == "sum":
        coef = np.ones(n)
        coef[-1] = 0.0
        out = mem[qf:qf + n] - mem[c:c + n] * cur + coef * nxt
    else:
        out = mem[qf:qf + n] - mem[c:c + n] * cur + np.where(nxt > cur, nxt, cur)  # a NaN falls through the comparison
    mem[res:res + n] = out
    if defect == "store_one_before":
        mem[res - 1] = 0.0
    if defect == "store_row_past_end":
        mem[res + n:res + n + II] = out[-II:]


KIND = {None: "sum", "store_one_before": "sum", "store_row_past_end": "sum", "load_after_times_zero": "sum",
        "load_after_through_max": "max"}
JJ, II = 5, 7
SPECS = [(k, (JJ, II)) for k in ("c", "qf", "q", "res")]


def _inputs():
    q = pb.uniform((JJ, II), 3, -1, 1)
    q[-1, -1] = 0.25  # positive: the zero that plain memory holds after the array loses the max, as a sound kernel's would
    return {"c": pb.uniform((JJ, II), 1, 0.5, 1.5), "qf": pb.uniform((JJ, II), 2, -1, 1), "q": q, "res": np.zeros((JJ, II))}


def _plain(defect, kind=None):
    """the call on plain arrays: what sits around them is zero, as in fresh device memory or heap padding"""
    n, pad = JJ * II, 3 * II
    mem = np.zeros(4 * (n + pad) + pad)
    at = {k: pad + i * (n + pad) for i, (k, _) in enumerate(SPECS)}
    for k, a in _inputs().items():
        mem[at[k]:at[k] + n] = a.ravel()
    standin(mem, at, JJ, II, kind or KIND[defect], defect)
    return mem[at["res"]:at["res"] + n].reshape(JJ, II).copy()


def _guarded(defect, poison, kind=None):
    ar = gd.Arena(SPECS, gd.POISONS[poison], "host", 2)
    for k, a in _inputs().items():
        ar.fill(k, a)
    standin(ar.buf, ar.start, JJ, II, kind or KIND[defect], defect)
    return ar


@pytest.mark.parametrize("poison", sorted(gd.POISONS))
@pytest.mark.parametrize("kind", ["sum", "max"])
def test_the_sound_standin_passes(poison, kind):
    ar = _guarded(None, poison, kind)
    ar.check()
    assert gd.same_bits(ar.array("res"), _plain(None, kind))
    for k, a in _inputs().items():
        if k != "res":
            assert gd.same_bits(ar.array(k), a)


@pytest.mark.parametrize("poison", sorted(gd.POISONS))
@pytest.mark.parametrize("defect,side,dist", [("store_one_before", "before", 1), ("store_row_past_end", "after", 1)])
def test_a_store_outside_is_reported_by_array_name(poison, defect, side, dist):
    ar = _guarded(defect, poison)
    with pytest.raises(AssertionError, match=rf"{dist} element\(s\) {side} array 'res'"):
        ar.check()
    name, where, d, count = ar.clobbered()
    assert (name, where, d) == ("res", side, dist) and count == (1 if defect == "store_one_before" else II)
    # the arrays themselves are what the plain call gives: only the bands show this defect
    assert gd.same_bits(ar.array("res"), _plain(defect))


def test_a_consumed_value_is_caught_by_one_poison_at_least():
    caught = {}
    for defect in ("load_after_times_zero", "load_after_through_max"):
        for poison in sorted(gd.POISONS):
            ar = _guarded(defect, poison)
            ar.check()  # nothing is stored outside: the bands cannot show a load
            caught[defect, poison] = not gd.same_bits(ar.array("res"), _plain(defect))
    # 0 * NaN is NaN, 0 * 2**1000 is 0
    assert caught["load_after_times_zero", "nan"] and not caught["load_after_times_zero", "big"]
    # NaN > x is false, so the max drops it; 2**1000 wins every comparison -- the reason for the second poison
    assert caught["load_after_through_max", "big"] and not caught["load_after_through_max", "nan"]


def test_plain_memory_hides_both_loads():
    """on plain arrays the defective stand-ins give the bits of the sound ones: what the suite could not see"""
    assert gd.same_bits(_plain("load_after_times_zero"), _plain(None, "sum"))
    assert gd.same_bits(_plain("load_after_through_max"), _plain(None, "max"))
