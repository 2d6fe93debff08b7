"""The fused Krylov kernels (cedar_amd/csrc/krylov.hip) one launcher at a time, through cedar_amd_pcg_direction /
_update / _rank_scalars / _ghost_shell (host arrays, staged by the library), against tests/krylov_statement.py.

Two kinds of data at every shape:

(a) small integers, everything bit for bit.  Operator entries are integers in [-4, 4] with a diagonal in [1, 4] (ghost
    entries non-zero), z, p, x, r, w integers in [-8, 8] (ghosts non-zero), beta in {0, 1, -2, 0.5}, alpha in
    {0.5, -2, 1}, diag (zmode 1) a power of two.  Then |p'| <= 8 + 2 * 8 = 24, |w| <= 26 * 4 * 24 + 4 * 24 = 2592 < 2^12,
    |p' w| < 2^17 per point, at most 2^21 points per case: every partial sum of a dot product, in any order, is below
    2^38 in units of the data's last bit (halves at most: 2^40), far below 2^53 -- an exact double.  So the dots have
    ONE correct bit pattern whatever the summation order, and with them alpha, beta (one correctly rounded division)
    and rho.  The update dots are smaller still.  Each case asserts sum |terms| < 2^53 on its own data.
(b) random reals (pb.random_op, pb.uniform, ghosts non-zero).  Arrays still bit for bit (the operation order of the
    kernels is fixed and the build does not contract to FMA); dots within the rigorous any-order bound
    2 n 2^-53 sum|t_i| of the exact sum (krylov_statement.any_order_bound).  A dropped or doubled term is ~ sum|t| / n:
    for the largest case here (1030 x 300 points, n = 3.1e5) the bound is 2 n 2^-53 = 6.9e-11 of sum|t| and one term is
    3.2e-6 of it, 4.7e4 times the bound.

Shapes are chosen for the branches of krylov.hip: the block-size switches of pcg_dir27 (pairs <= 64, <= 128, more) and
pcg_dir7 (nx <= 64, < 256, more), rows longer than one trip of the lane loops, odd nx (the half pair at the row end), row
counts that leave partial (j,k) tiles and grid padding, more than 1024 partials for slab_sum, more rows than pcg_upd has
workgroups, several workgroups per row in 2D.
"""
import ctypes as C
import math

import numpy as np
import pytest

import krylov_statement as ks
import problems as pb

pytestmark = pytest.mark.gpu

BETAS = [0.0, 1.0, -2.0, 0.5]
ALPHAS = [0.5, -2.0, 1.0]
MARKS = {ks.SIGMA: 101.0, ks.ALPHA: 102.0, ks.BETA: 103.0, ks.RR: 104.0, ks.RZ: 105.0}  # slots a pass must leave alone


@pytest.fixture(scope="module")
def K():
    from cedar_amd import capi
    assert capi.device_count() >= 1, "no GPU visible"
    return capi.Kernels()


def ints(shape, seed, lo, hi):
    return np.floor(pb.uniform(shape, seed, lo, hi + 1))


def int_op(g, nst, seed):
    so = ints((nst,) + g, seed, -4, 4)
    so[0] = ints(g, seed + 1000, 1, 4)
    return so


def scalars(**kw):
    sc = np.zeros(ks.NSC)
    for k, v in MARKS.items():
        sc[k] = v
    for k, v in kw.items():
        sc[getattr(ks, k.upper())] = v
    return sc


def shape_of(nx, ny, nz=None):
    return (ny + 2, nx + 2) if nz is None else (nz + 2, ny + 2, nx + 2)


def exact_dot(u, v, integer):
    """(value, bound): the one correct double and 0 on integer data, else the rounded exact sum and the any-order bound"""
    if integer:
        tot, sab, sh = ks.exact_dot_dyadic(u, v)
        assert sab < 2 ** 53, "the premise of the bit-for-bit dot no longer holds"
        return ks.dyadic_value(tot, sh), 0.0
    s, sab, n = ks.exact_dot_real(u, v)
    return s, ks.any_order_bound(n, sab)


# ---------------------------------------------------------------- direction
def direction_data(g, nst, integer, seed):
    if integer:
        return int_op(g, nst, seed), ints(g, seed + 1, -8, 8), ints(g, seed + 2, -8, 8)
    return pb.random_op(g, nst, seed, zero_ghost=False), pb.uniform(g, seed + 1, -1, 1), pb.uniform(g, seed + 2, -1, 1)


def check_direction(K, oracle, so, z, p, beta, first, integer, so_args=None, rho=3.0):
    """one-rank and rank-grid variant of the pass for every operator argument (host planes, registered device operator)"""
    g = z.shape
    pn0, w0 = pb.uniform(g, 77, 1, 2), pb.uniform(g, 78, 1, 2)  # what the pass must leave outside the interior
    sc0 = scalars(rho=rho, beta=beta)
    p_arg = np.full(g, np.nan) if first else p  # first: p is not read
    want_pn, want_w = ks.direction(oracle, so, z, p, pn0, w0, beta, first)
    sigma, bound = exact_dot(want_pn, want_w, integer)
    outs = []
    for so_arg in so_args or [so]:
        pn, w, sc = pn0.copy(), w0.copy(), sc0.copy()
        K.pcg_direction(so_arg, z, p_arg, pn, w, first, sc)
        what = (g, beta, first, integer, type(so_arg).__name__)
        assert np.array_equal(pn, want_pn), ("pn", what)
        assert np.array_equal(w, want_w), ("w", what, np.max(np.abs(w - want_w)))
        if integer:
            assert np.array_equal(sc, ks.set_alpha(sigma, sc0)), (what, sc, sigma)
        else:
            assert abs(sc[ks.SIGMA] - sigma) <= bound, (what, sc[ks.SIGMA], sigma, bound)
            assert np.array_equal(sc, ks.set_alpha(float(sc[ks.SIGMA]), sc0)) and sc[ks.FLAG] == 0.0, (what, sc)
        # rank-grid variant: the same sum into partial[0], sc only read
        pn2, w2, sc2, part = pn0.copy(), w0.copy(), sc0.copy(), np.array([55.0])
        K.pcg_direction(so_arg, z, p_arg, pn2, w2, first, sc2, part)
        assert np.array_equal(pn2, want_pn) and np.array_equal(w2, want_w), what
        assert np.array_equal(sc2, sc0) and part[0] == sc[ks.SIGMA], (what, sc2, part, sc[ks.SIGMA])
        outs.append(sc)
    for sc in outs[1:]:
        assert np.array_equal(sc, outs[0]), "the operator views differ"
    return outs[0]


def sweep_direction(K, oracle, g, nst, so_args_of=None):
    for integer in (True, False):
        so, z, p = direction_data(g, nst, integer, 300 + nst)
        args = so_args_of(so) if so_args_of else None
        try:
            for beta in BETAS if integer else [0.3717]:
                check_direction(K, oracle, so, z, p, beta, False, integer, args and args[0])
            check_direction(K, oracle, so, z, p, 0.625, True, integer, args and args[0])  # first: beta forced to 0
        finally:
            if args:
                args[1]()


# nx: both sides of the 64- and 128-pair switches, odd nx = half pair at the row end, nx > 512 = second trip of the pair
# loop; (ny, nz): 9, 30, 126, 297 rows -- partial (j,k) tiles and grid padding
DIR27 = [(3, 3, 3), (4, 5, 6), (127, 18, 7), (128, 33, 9), (129, 3, 3), (130, 5, 6), (255, 18, 7), (256, 33, 9),
         (257, 5, 6), (258, 18, 7), (513, 33, 9), (600, 5, 6), (600, 33, 9)]


@pytest.mark.parametrize("shape", DIR27, ids=str)
def test_direction_27pt_both_operator_views(K, oracle, monkeypatch, shape):
    """pcg_dir27<64|128|256> on the Cedar planes and on the row-interleaved copy of a registered operator"""
    from cedar_amd import capi
    monkeypatch.setenv("CEDAR_AMD_ILV", "1")  # a solve copy at any size
    g = shape_of(*shape)
    capi.lib.cedar_amd_relax3_prepare.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint]

    def views(so):
        so_d, sor_d = capi.DeviceArray.from_numpy(so), capi.DeviceArray((2,) + g)
        K.setup_recip3(so_d, sor_d)
        assert capi.lib.cedar_amd_relax3_prepare(so_d.ptr, sor_d.ptr, g[2], g[1], g[0]) & 1

        def done():
            so_d.free()  # drops the registration with it
            sor_d.free()
        return [so, so_d], done

    sweep_direction(K, oracle, g, 14, views)


# block size 64 / 128 / 256, a second trip of the lane loop; 33 x 40 rows: a second trip of slab_sum
DIR7 = [(3, 3, 3), (64, 5, 6), (65, 18, 7), (255, 5, 6), (256, 33, 9), (257, 18, 7), (600, 5, 6), (65, 33, 40)]


@pytest.mark.parametrize("shape", DIR7, ids=str)
def test_direction_7pt(K, oracle, shape):
    sweep_direction(K, oracle, shape_of(*shape), 4)


# 1 .. 5 workgroups per row with a ragged last one; 5 x 300 = 1500 partials
DIR2 = [(3, 3), (255, 40), (256, 3), (257, 40), (513, 300), (1030, 300), (1030, 3), (256, 300)]


@pytest.mark.parametrize("nst", [3, 5])
@pytest.mark.parametrize("shape", DIR2, ids=str)
def test_direction_2d(K, oracle, shape, nst):
    sweep_direction(K, oracle, shape_of(*shape), nst)


# ---------------------------------------------------------------- update
UPD = [(5, 2100), (600, 9), (1030, 7), (7, 50, 47), (130, 9, 8), (129, 6, 5), (600, 5, 4)]


def update_data(g, integer, seed):
    if integer:
        f = [ints(g, seed + t, -8, 8) for t in range(5)]
        diag = 2.0 ** ints(g, seed + 9, 0, 3)
    else:
        f = [pb.uniform(g, seed + t, -1, 1) for t in range(5)]
        diag = pb.uniform(g, seed + 9, 1, 3)
    return f, diag


def check_update(K, g, zmode, move, alpha, first, integer, data, rho=5.0):
    (x, r, p, w, zin), diag = data
    zmark = pb.uniform(g, 79, 1, 2)
    z0 = zin if zmode == 2 else zmark if zmode == 1 else None
    sc0 = scalars(rho=rho, alpha=alpha)
    a = (x, p, w) if move else (None, None, None)
    want_x, want_r, want_z = ks.update(zmode, move, a[0], r, a[1], a[2], z0, diag, alpha)
    rr, brr = exact_dot(want_r, want_r, integer)
    rz, brz = exact_dot(want_r, want_z, integer) if zmode in (1, 2) else (0.0, 0.0)
    what = (g, zmode, move, alpha, first, integer)

    def run(partial):
        xg, rg = (x.copy() if move else None), r.copy()
        zg = None if z0 is None else z0.copy()
        sc = sc0.copy()
        K.pcg_update(zmode, move, xg, rg, a[1], a[2], zg, diag if zmode == 1 else None, first, sc, partial)
        assert np.array_equal(rg, want_r), ("r", what)
        assert xg is None or np.array_equal(xg, want_x), ("x", what)
        assert zg is None or np.array_equal(zg, want_z), ("z", what)
        return sc

    sc = run(None)
    if integer:
        assert np.array_equal(sc, ks.update_scalars(zmode, rr, rz, first, sc0)), (what, sc, rr, rz)
    else:
        assert abs(sc[ks.RR] - rr) <= brr, (what, sc[ks.RR], rr, brr)
        if zmode in (1, 2):
            assert abs(sc[ks.RZ] - rz) <= brz, (what, sc[ks.RZ], rz, brz)
        assert np.array_equal(sc, ks.update_scalars(zmode, float(sc[ks.RR]), float(sc[ks.RZ]), first, sc0)), (what, sc)
    part = np.array([55.0, 56.0])
    sc2 = run(part)
    assert np.array_equal(sc2, sc0), (what, sc2)
    want_part = [sc[ks.RR] if zmode != 3 else 55.0, sc[ks.RZ] if zmode in (1, 2) else 56.0]
    assert part.tolist() == want_part, (what, part, want_part)
    return sc


@pytest.mark.parametrize("integer", [True, False], ids=["int", "real"])
@pytest.mark.parametrize("shape", UPD, ids=str)
def test_update_every_mode(K, shape, integer):
    """pcg_upd<zmode, move>: more rows than workgroups (the row dealing wraps), even / odd nx, a second trip of the pair
    loop, KK = 1 addressing; the one-rank and the rank-grid second stage.  r's ghost column next to a half pair is
    non-zero here: a kernel that loaded the whole pair at the row end and summed it would change r.r (ldpair hands back
    0 for the missing half, so the `if (two)` guards of the sums alone change nothing when removed)."""
    g = shape_of(*shape)
    data = update_data(g, integer, 500)
    n = 0
    for zmode in range(4):
        for move in (0, 1):
            for first in (False, True):
                alpha = ALPHAS[n % 3] if integer else -0.4142
                n += 1
                check_update(K, g, zmode, move, alpha, first, integer, data)


# ---------------------------------------------------------------- breakdown
def spd_int_op(g, nst, seed):
    so = int_op(g, nst, seed)
    so[0] = ints(g, seed + 1000, 109, 112)  # above the 26 * 4 of the off-diagonals: positive definite
    return so


@pytest.mark.parametrize("shape,nst", [((130, 9, 8), 14), ((65, 18, 7), 4), ((257, 40), 5), ((257, 40), 3)], ids=str)
def test_breakdown_of_the_direction_pass(K, oracle, shape, nst):
    g = shape_of(*shape)
    so, z, p = spd_int_op(g, nst, 700), ints(g, 701, -8, 8), ints(g, 702, -8, 8)
    # healthy: sigma > 0, no flag
    sc = check_direction(K, oracle, so, z, p, 1.0, False, True)
    assert sc[ks.SIGMA] > 0 and sc[ks.ALPHA] == 3.0 / sc[ks.SIGMA] and sc[ks.FLAG] == 0.0
    # (i) the operator negated: sigma < 0
    sc = check_direction(K, oracle, -so, z, p, 1.0, False, True)
    assert sc[ks.SIGMA] < 0 and sc[ks.ALPHA] == 0.0 and sc[ks.FLAG] == 1.0
    # (iii) rho = 0 on entry: sigma still stored
    sc = check_direction(K, oracle, so, z, p, 1.0, False, True, rho=0.0)
    assert sc[ks.SIGMA] > 0 and sc[ks.ALPHA] == 0.0 and sc[ks.FLAG] == 1.0
    # (ii) z of 1e200 on the interior, off-diagonals made non-negative (they enter with a minus sign: every row sum
    # is at least 109 - 104 > 0): every w is positive, every product p' w overflows to +inf, sigma = inf
    so = np.abs(so)
    z = 1e200 * pb.interior_mask(g).astype(np.float64)
    pn, w, sc = np.zeros(g), np.zeros(g), scalars(rho=3.0)
    with np.errstate(over="ignore", invalid="ignore"):
        want_pn, want_w = ks.direction(oracle, so, z, None, pn, w, 0.0, True)
    assert np.all(ks.inner(want_w) >= 1e200) and np.all(np.isfinite(want_w))
    K.pcg_direction(so, z, None, pn, w, True, sc)
    assert np.array_equal(pn, want_pn) and np.array_equal(w, want_w)
    assert sc[ks.SIGMA] == math.inf and sc[ks.ALPHA] == 0.0 and sc[ks.FLAG] == 1.0 and sc[ks.RHO] == 3.0, sc


@pytest.mark.parametrize("shape", [(129, 6, 5), (600, 9)], ids=str)
def test_update_after_breakdown_leaves_x_and_r(K, shape):
    """alpha = 0 with infinities and NaN in p and w: x, r bit for bit as they were, r.r the dot of the unchanged r"""
    g = shape_of(*shape)
    data = update_data(g, True, 800)
    (x, r, p, w, zin), diag = data
    p, w = p.copy(), w.copy()
    p.ravel()[::7], p.ravel()[3::11] = np.inf, np.nan
    w.ravel()[::5], w.ravel()[2::13] = -np.inf, np.nan
    for zmode in range(4):
        sc = check_update(K, g, zmode, 1, 0.0, False, True, ((x, r, p, w, zin), diag))
        assert np.isfinite(sc[ks.RR]) and sc[ks.RR] == exact_dot(r, r, True)[0] and sc[ks.FLAG] == 0.0


# ---------------------------------------------------------------- rank-order combine
def spread(n, seed):
    """mixed signs, magnitudes over 2^+-30: the order of a sum matters"""
    return pb.uniform((n,), seed, -1, 1) * 2.0 ** ints((n,), seed + 1, -30, 30)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_rank_order_combine(K, world, stride):
    g = spread(world * stride, 900 + world)
    g[::stride] = np.abs(g[::stride])  # sigma, r.r
    if world == 8:  # on this data the order matters: the reversed sum differs
        rev = 0.0
        for v in g[::stride][::-1].tolist():
            rev += v
        assert ks.rank_sum(g, world, stride, 0) != rev
    sc0 = scalars(rho=0.75)
    sc = sc0.copy()
    K.pcg_rank_scalars(0, 0, g, world, stride, False, sc)
    assert np.array_equal(sc, ks.rank_alpha(g, world, stride, sc0)) and sc[ks.FLAG] == 0.0, (sc, g)
    for zmode in ([0, 3] if stride == 1 else range(4)):  # has_rz 2, 1, 1, 0; r.z needs a second double per rank
        for first in (False, True):
            sc = sc0.copy()
            K.pcg_rank_scalars(1, zmode, g, world, stride, first, sc)
            assert np.array_equal(sc, ks.rank_rho(zmode, g, world, stride, first, sc0)), (zmode, first, sc, g)
    # breakdown on the summed value: the ranks' sigma cancel
    gz = np.zeros(world * stride)
    gz[0] = 1.0
    gz[(world - 1) * stride] += -1.0
    sc = sc0.copy()
    K.pcg_rank_scalars(0, 0, gz, world, stride, False, sc)
    assert sc[ks.SIGMA] == 0.0 and sc[ks.ALPHA] == 0.0 and sc[ks.FLAG] == 1.0 and sc[ks.RHO] == 0.75, sc
    with pytest.raises(RuntimeError):
        K.pcg_rank_scalars(1, 1, g, world, 1, False, sc0.copy())  # r.z does not fit one double per rank
    with pytest.raises(RuntimeError):
        K.pcg_rank_scalars(0, 0, g, 0, stride, False, sc0.copy())


@pytest.mark.parametrize("shape,nst", [((130, 9, 8), 14), ((257, 40), 5)], ids=str)
def test_one_rank_world_equals_the_one_rank_stage(K, oracle, shape, nst):
    """partials of the rank-grid variant, combined with world = 1, are the one-rank scalars bit for bit (common.h)"""
    g = shape_of(*shape)
    so, z, p = direction_data(g, nst, False, 950)
    sc0 = scalars(rho=3.0, beta=0.3)
    pn, w, sc1 = np.zeros(g), np.zeros(g), sc0.copy()
    K.pcg_direction(so, z, p, pn, w, False, sc1)
    part, sc2 = np.zeros(1), sc0.copy()
    K.pcg_direction(so, z, p, np.zeros(g), np.zeros(g), False, sc0.copy(), part)
    K.pcg_rank_scalars(0, 0, part, 1, 1, False, sc2)
    assert np.array_equal(sc1, sc2), (sc1, sc2)
    x, r = pb.uniform(g, 951, -1, 1), pb.uniform(g, 952, -1, 1)
    for zmode in (0, 1, 2):
        zz = pb.uniform(g, 953, -1, 1)
        d = pb.uniform(g, 954, 1, 3)
        outs = []
        for ranks in (False, True):
            xg, rg, zg, sc, part = x.copy(), r.copy(), zz.copy(), sc1.copy(), np.zeros(2)
            K.pcg_update(zmode, 1, xg, rg, pn, w, zg, d, False, sc, part if ranks else None)
            if ranks:
                K.pcg_rank_scalars(1, zmode, part, 1, 2, False, sc)
            outs.append((xg, rg, zg, sc))
        for a, b in zip(*outs):
            assert np.array_equal(a, b), (zmode, outs[0][3], outs[1][3])


# ---------------------------------------------------------------- ghost shell
def shell_boxes(n, split):
    """the receive boxes of a rank box of n = (nx, ny, nz) owned points with neighbours along the split directions, cut to
    the owned range along the others (dist_common.h krylov_alloc): faces, edges, corners, one cell wide"""
    boxes = []
    for ok in (-1, 0, 1):
        for oj in (-1, 0, 1):
            for oi in (-1, 0, 1):
                o = (oi, oj, ok)
                if o == (0, 0, 0) or any(o[t] and t not in split for t in range(3)):
                    continue
                lo = [0 if o[t] < 0 else n[t] + 1 if o[t] > 0 else 1 for t in range(3)]
                cnt = [1 if o[t] else n[t] for t in range(3)]
                boxes.append(lo + cnt)
    return boxes


@pytest.mark.parametrize("integer", [True, False], ids=["int", "real"])
@pytest.mark.parametrize("split", [(0,), (1, 2), (0, 1, 2)], ids=str)
def test_ghost_shell(K, split, integer):
    n = (20, 17, 9)
    g = shape_of(*n)
    boxes = shell_boxes(n, split)
    assert len(boxes) == 3 ** len(split) - 1
    mk = (lambda s: ints(g, s, -8, 8)) if integer else (lambda s: pb.uniform(g, s, -1, 1))
    z, p, pn0 = mk(960), mk(961), pb.uniform(g, 962, 1, 2)
    for beta, first in [(b, False) for b in (BETAS if integer else [0.3717])] + [(0.625, True)]:
        sc0 = scalars(beta=beta)
        pn, sc = pn0.copy(), sc0.copy()
        K.pcg_ghost_shell(z, np.full(g, np.nan) if first else p, pn, first, sc, boxes)
        want = ks.shell(z, p, pn0, beta, first, boxes)
        assert np.array_equal(pn, want) and np.array_equal(sc, sc0), (split, beta, first)
        assert np.array_equal(ks.inner(pn), ks.inner(pn0))  # the shell is ghost cells only


def test_ghost_shell_grid_stride_and_refusals(K):
    """one box of more than 256 * 1024 cells (a second trip of the grid-stride loop) beside a one-cell box; boxes that
    reach outside the array are refused before anything is launched"""
    g = (10, 200, 200)
    z, p, pn0 = pb.uniform(g, 970, -1, 1), pb.uniform(g, 971, -1, 1), pb.uniform(g, 972, 1, 2)
    boxes = [[1, 1, 1, 198, 198, 8], [0, 0, 9, 1, 1, 1]]
    assert 198 * 198 * 8 > 256 * 1024
    sc = scalars(beta=-0.77)
    pn = pn0.copy()
    K.pcg_ghost_shell(z, p, pn, False, sc, boxes)
    assert np.array_equal(pn, ks.shell(z, p, pn0, -0.77, False, boxes))
    pn = pn0.copy()
    K.pcg_ghost_shell(z, p, pn, False, sc, [])  # no box: nothing to do
    assert np.array_equal(pn, pn0)
    for bad in ([[0, 0, 0, 201, 1, 1]], [[199, 0, 0, 2, 1, 1]], [[0, 0, 10, 1, 1, 1]], [[-1, 0, 0, 1, 1, 1]],
                [[0, 0, 0, 0, 1, 1]], [[0, 0, 0, 1, 1, 1]] * 27):
        with pytest.raises(RuntimeError):
            K.pcg_ghost_shell(z, p, pn, False, sc, bad)
        assert np.array_equal(pn, pn0)


# ---------------------------------------------------------------- refusals and determinism
def test_pass_entry_points_refuse_what_they_do_not_serve(K):
    g = (5, 6, 7)
    f = pb.uniform(g, 1, -1, 1)
    so = pb.random_op(g, 14, 2)
    sc = scalars()
    for nst in (3, 5, 7):
        with pytest.raises(RuntimeError):
            K.pcg_direction(so[:nst].copy(), f, f, f.copy(), f.copy(), False, sc)
    with pytest.raises(RuntimeError):
        K.pcg_direction(so, f, None, f.copy(), f.copy(), False, sc)  # p is needed unless first
    with pytest.raises(RuntimeError):
        K.pcg_update(4, 0, None, f.copy(), None, None, None, None, False, sc)
    with pytest.raises(RuntimeError):
        K.pcg_update(1, 0, None, f.copy(), None, None, f.copy(), None, False, sc)  # zmode 1 needs the diagonal
    with pytest.raises(RuntimeError):
        K.pcg_update(0, 1, None, f.copy(), f, f, None, None, False, sc)  # move needs x
    with pytest.raises(RuntimeError):
        K.pcg_update(0, 0, None, np.zeros((2, 5)), None, None, None, None, False, sc)
    assert np.array_equal(sc, scalars())


def test_passes_are_deterministic(K, oracle):
    """the largest 27-point and 2D cases twice: identical scalars and arrays"""
    for shape, nst in (((600, 33, 9), 14), ((1030, 300), 5)):
        g = shape_of(*shape)
        so, z, p = direction_data(g, nst, False, 990)
        x, r = pb.uniform(g, 991, -1, 1), pb.uniform(g, 992, -1, 1)
        outs = []
        for _ in range(2):
            pn, w, sc = np.zeros(g), np.zeros(g), scalars(rho=3.0, beta=0.3717)
            K.pcg_direction(so, z, p, pn, w, False, sc)
            xg, rg, zg = x.copy(), r.copy(), np.zeros(g)
            K.pcg_update(1, 1, xg, rg, pn, w, zg, so[0].copy(), False, sc)
            outs.append((pn, w, xg, rg, zg, sc))
        for a, b in zip(*outs):
            assert np.array_equal(a, b)
        assert np.all(np.isfinite(outs[0][5])) and outs[0][5][ks.FLAG] == 0.0
