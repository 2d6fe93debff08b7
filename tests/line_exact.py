"""Line-solve data on which every operation is exact, and the plain sequential sweep on it (numpy only).

The zebra line kernels evaluate both sweeps of DPTTRS as first-order recurrences y_i = a_i y_(i-1) + c_i and
re-associate them (8-unknown chunks, a Kogge-Stone scan over a wavefront, a chain over the wavefronts of a workgroup, a
carry between tiles; cedar_amd/csrc/lines_dev.h).  On the operators of problems.random_op the multipliers a_i are about
0.04, so whatever the scan carries beyond a chunk is damped below every tolerance before it reaches an unknown.  Here
nothing is damped and nothing is rounded:

  factors    pivots d = 1, or drawn from {0.5, 1, 2, 4} ("dyadic"); multipliers e' drawn from {-1, +1}, zero at listed
             positions (a zero at position p decouples the unknowns p and p + 1 of the line)
  vectors    qf and q0 are small integers, ghost cells included
  operator   entries in {-1, 0, 1}; the closure couplings of cyclic lines (KW for x lines, KS for y lines) in {1, 2, 3}

Every value a sweep forms is then an integer multiple of a power of two 1 / g (g = 1 with unit pivots), every composite
of a sub-range of a recurrence is bounded by the sum of |c_k| over the line, and as long as that sum times g stays below
2**53 every association of the recurrence has the same, exactly representable, result.  `solve_lines` asserts this for
every line and both sweeps; it is a condition of the data, checked where the reference is computed, not a measurement
of a kernel.

The closure of a cyclic line is not exact (a division by 1 + alpha and a product with beta); it is computed with the
kernels' own three roundings, alpha = u_1 + u_n, beta = (y_1 + y_n) / (1 + alpha), x = y - beta * u, on exact y and u.
Cyclic cases have no cross-line couplings, so the second colour's right-hand sides do not read the first colour's
(rounded) results.

Layouts, as the kernels read them (arrays are C-ordered, the reversed Fortran shape, ghosts included):
  x lines    sor[0][j][i] is the pivot of point (i, j), sor[1][j][i + 1] couples the points i and i + 1 of row j
  y lines    the same in SOR(JJ,II,2): a numpy array of shape (2, II, JJ) handed over as shape (2, JJ, II)
"""
import collections
import functools

import numpy as np

KO, KW, KS, KSW, KNW = range(5)
DOWN, UP = 0, 1
CH, WAVE = 8, 64  # unknowns a lane owns, lanes of a wavefront
NLINES = 5  # lines of a case: the colours hold 3 and 2

# line lengths, each the smallest at which a step of the scan is first taken (one wavefront of 64 lanes up to 512
# unknowns, 256 lanes on tiles of 2048 unknowns beyond)
#   1, 9        chunk edge
#   512         one full 64-lane tile
#   513         256 lanes, the first value in a second wavefront
#   1025        two-hop chain over the wavefronts
#   2048, 2049  tile boundary
#   4097        a multiplier product through a whole middle tile
#   4500        the long case of the random_op line tests
LENGTHS = [1, 9, 512, 513, 1025, 2048, 2049, 4097, 4500]
CYCLIC_LENGTHS = [2, 9, 512, 513, 2049]
CYCLIC = [("x", 2), ("x", 3), ("y", 1), ("y", 3)]  # (direction, boundary code) with cyclic lines
AFFINE_LENGTHS = [1, 9, 512, 513, 2049, 4500]
SETUP_LENGTHS = [513, 2049]
NINE_POINT_UP_TO = 1030  # Dirichlet cases beyond this many unknowns couple the lines through KS / KW only

Case = collections.namedtuple("Case", "d n nst so qf q0 sor")


def line_zeros(n, line):
    """positions p at which the coupling e'_p of line `line` (0 .. 4) is zero.  The forward sweep multiplies the unknown
    at scan position i by -e'_(i-1), the backward sweep the one at reversed position r by -e'_(n-1-r); a tile is 2048
    scan positions.  Lines shorter than 4097 have none.
      line 0  none: the product of 2048 unit multipliers crosses the middle tile
      line 1  a run over [2046, 4096]: the forward composites of the whole middle tile and of the lanes next to it are
              (0, c); what tile 0 carries must not reach tile 2
      line 2  the same for the backward sweep, [n-1-4097, n-1-2046]
      line 3  both ends of the middle tile, forward and backward
      line 4  the couplings 2046 and 4096 alone: the unknowns 2047 .. 4096 are one run that enters tile 1 from the last
              lane of tile 0 and leaves it into the first lane of tile 2"""
    if n < 4097:
        return []
    z = {1: range(2046, 4097), 2: range(n - 1 - 4097, n - 1 - 2045),
         3: [2047, 4094, n - 1 - 2048, n - 1 - 4095], 4: [2046, 4096]}.get(line, [])
    return sorted({p for p in z if 0 <= p < n - 1})


def make_factors(rng, n, nl, dyadic, zeros):
    """(2, nl + 2, n + 2), line-major: [0, l, t + 1] is the pivot of unknown t of line l (1-based among the ghosts),
    [1, l, t + 2] the coupling e'_t of the unknowns t and t + 1.  zeros: line (0-based) -> positions"""
    f = np.empty((2, nl + 2, n + 2))
    f[0] = rng.choice([0.5, 1.0, 2.0, 4.0], f[0].shape) if dyadic else 1.0
    f[1] = rng.choice([-1.0, 1.0], f[1].shape)
    for l, pos in (zeros or {}).items():
        f[1, l + 1, np.asarray(pos, dtype=int) + 2] = 0.0
    return f


def as_sor(f, d, g):
    """line-major factors -> the array a kernel is handed, shape (2,) + g"""
    return np.ascontiguousarray(f).reshape((2,) + tuple(g))


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


def make_case(n, d, seed, cyclic=False, nst=None, nlines=NLINES, dyadic=False):
    """a line sweep's inputs: n unknowns a line, `nlines` lines along d ("x" | "y")"""
    rng = np.random.default_rng(seed)
    nx, ny = (n, nlines) if d == "x" else (nlines, n)
    g = (ny + 2, nx + 2)
    if nst is None:
        nst = 5 if n <= NINE_POINT_UP_TO else 3
    so = np.zeros((nst,) + g)
    if cyclic:
        so[KW if d == "x" else KS] = rng.integers(1, 4, g)  # every other coupling of a sweep is zero
        zeros = None
    else:
        for s in range(1, nst):
            so[s] = rng.integers(-1, 2, g)
        zeros = {l: line_zeros(n, l) for l in range(nlines)}
    qf = rng.integers(-4, 5, g).astype(np.float64)
    q0 = rng.integers(-4, 5, g).astype(np.float64)
    sor = as_sor(make_factors(rng, n, nlines, cyclic or dyadic, zeros), d, g)
    _freeze(so, qf, q0, sor)
    return Case(d, n, nst, so, qf, q0, sor)


def make_setup_case(n, d, seed, nlines=NLINES):
    """an operator on which DPTTRF is exact: along a line the coupling is 2**k, the diagonal 2**k at the first unknown and
    2 * 2**k elsewhere, k per line in {-1, 0, 1, 2}.  The factorisation has pivots 2**k and multipliers e' = -1 throughout.
    Returns (case with zero factors, the expected factor array)"""
    c = make_case(n, d, seed, nlines=nlines)
    rng = np.random.default_rng(seed + 1)
    so = c.so.copy()
    k = rng.integers(-1, 3, nlines + 2)
    assert nlines >= 4
    k[1:5] = [-1, 0, 1, 2]  # every exponent occurs
    p = 2.0 ** k
    along = KW if d == "x" else KS
    g = so.shape[1:]
    pl = p[:, None] * np.ones((nlines + 2, n + 2))  # line-major
    diag = 2.0 * pl
    diag[:, 1] = pl[:, 1]
    so[along] = pl if d == "x" else pl.T
    so[KO] = diag if d == "x" else diag.T
    want = np.zeros((2, nlines + 2, n + 2))
    want[0, 1:-1, 1:n + 1] = pl[1:-1, 1:n + 1]
    want[1, 1:-1, 1] = -pl[1:-1, 1]  # -coupling of the first unknown: stored, never factored or read
    want[1, 1:-1, 2:n + 1] = -1.0
    want = as_sor(want, d, g)
    _freeze(so, want)
    return c._replace(so=so, sor=np.zeros((2,) + g)), want


@functools.lru_cache(maxsize=None)
def dirichlet_case(n, d, dyadic=False):
    return make_case(n, d, 4000 + 2 * n + (d == "y"), dyadic=dyadic)


@functools.lru_cache(maxsize=None)
def cyclic_case(n, d, ibc, nst):
    # (with the seeds from 6000 one line of two unknowns has 1 + alpha = 0, which `sweep` refuses)
    return make_case(n, d, 6001 + 8 * n + 2 * ibc + (d == "y"), cyclic=True, nst=nst)


@functools.lru_cache(maxsize=None)
def setup_case(n, d):
    return make_setup_case(n, d, 7000 + 2 * n + (d == "y"))


def line_major(a, d):
    """view of a grid array (JJ, II) with the lines of direction d as rows"""
    return a if d == "x" else a.T


def factors_of(case):
    """line-major view (2, nl + 2, n + 2) of a case's factor array"""
    JJ, II = case.so.shape[1:]
    return case.sor if case.d == "x" else case.sor.reshape(2, II, JJ)


LIMIT = 2.0 ** 53


def grain(t):
    """the smallest power of two g for which every entry of t is an integer multiple of 1 / g"""
    g = 1.0
    while not np.array_equal(t * g, np.rint(t * g)):
        g *= 2.0
        assert g <= 2.0 ** 40
    return g


def scaled_sum(c):
    """largest sum of |c_k| over a row, in units of the rows' common grain: every composite of a sub-range of a recurrence
    with multipliers in {-1, 0, 1} is a multiple of that grain no larger than this sum"""
    return float(np.max(np.sum(np.abs(c), axis=1))) * grain(c)


def solve_lines(c, dd, e):
    """the DPTTRS recurrences, one unknown after the other, on the rows of c (lines, n): forward
    y_k = c_k - e_(k-1) y_(k-1), backward x_k = y_k / d_k - e_k x_(k+1).  Asserts the conditions under which every
    association of either recurrence is exact.  Returns (x, the largest scaled sum met)"""
    nl, n = c.shape
    assert dd.shape == (nl, n) and e.shape == (nl, max(n - 1, 0))
    assert np.all(np.isin(e, (-1.0, 0.0, 1.0))) and np.all(np.frexp(dd)[0] == 0.5)  # unit multipliers, pivots 2**k
    y = np.empty_like(c)
    v = c[:, 0].copy()
    y[:, 0] = v
    for k in range(1, n):
        v = c[:, k] - e[:, k - 1] * v
        y[:, k] = v
    z = y / dd
    x = np.empty_like(c)
    v = z[:, n - 1].copy()
    x[:, n - 1] = v
    for k in range(n - 2, -1, -1):
        v = z[:, k] - e[:, k] * v
        x[:, k] = v
    worst = max(scaled_sum(c), scaled_sum(z))
    assert worst < LIMIT, worst
    return x, worst


def line_rhs(case, q, rows):
    """right-hand sides of the lines `rows` (indices along the other direction), as relax_lines_x.f90 / _y.f90 form them,
    in their term order; (len(rows), n)"""
    so, qf = [line_major(p, case.d) for p in case.so], line_major(case.qf, case.d)
    q = line_major(q, case.d)
    cross = KS if case.d == "x" else KW  # couples a line with the one before it
    r = np.asarray(rows)[:, None]
    t = np.arange(1, case.n + 1)[None, :]
    terms = [qf[r, t], so[cross][r, t] * q[r - 1, t], so[cross][r + 1, t] * q[r + 1, t]]
    if case.nst == 5:
        # line-major (row r the line, column t the position) the four corner terms read the same in both directions:
        # KSW stored at a point couples it with (r-1, t-1), KNW stored at a point couples (r-1, t) with (r, t-1).  The
        # two files differ in the order of the middle two terms
        mid = [so[KNW][r, t + 1] * q[r - 1, t + 1], so[KNW][r + 1, t] * q[r + 1, t - 1]]
        terms += [so[KSW][r, t] * q[r - 1, t - 1]] + (mid if case.d == "x" else mid[::-1]) \
            + [so[KSW][r + 1, t + 1] * q[r + 1, t + 1]]
    terms = np.stack(terms)
    assert len(terms) * np.max(np.abs(terms)) * grain(terms) < LIMIT  # every partial sum is exact
    s = terms[0]
    for term in terms[1:]:
        s = s + term
    return s


def wrap(q, ibc):
    """ghost cells of the periodic directions from the interior: y first, then x"""
    JJ, II = q.shape
    if ibc in (1, 3):
        q[0, :] = q[JJ - 2, :]
        q[JJ - 1, :] = q[1, :]
    if ibc in (2, 3):
        q[:, 0] = q[:, II - 2]
        q[:, II - 1] = q[:, 1]


def sweep(case, ud, ibc=0, stats=None):
    """one zebra sweep of relax_lines_x / _y in the DOWN / UP colour order; ibc 0, or a code under which the lines of
    case.d are cyclic (x: 2, 3; y: 1, 3).  stats: dict that receives the largest scaled sum and the smallest |1 + alpha|"""
    d, n = case.d, case.n
    assert ibc == 0 or (d, ibc) in CYCLIC
    f = factors_of(case)
    q = case.q0.copy()
    ql = line_major(q, d)
    nl = ql.shape[0] - 2
    so = [line_major(p, d) for p in case.so]
    close = KW if d == "x" else KS
    if ibc:
        cross = [s for s in range(1, case.nst) if s != close]
        assert not any(np.any(case.so[s]) for s in cross)  # the colours stay independent
    worst, dens = 0.0, []
    for colour in range(2):
        b = 1 - colour if ud == DOWN else colour
        rows = list(range(1 + b, nl + 1, 2))
        if rows:
            dd, e = f[0][rows, 1:n + 1], f[1][rows, 2:n + 1]
            y, w = solve_lines(line_rhs(case, q, rows), dd, e)
            worst = max(worst, w)
            if ibc:
                u = np.zeros_like(y)
                u[:, 0] = -so[close][rows, 1]
                u[:, n - 1] = -so[close][rows, n + 1]  # n == 1: the second assignment wins, as in the reference
                u, w = solve_lines(u, dd, e)
                worst = max(worst, w)
                alpha = u[:, 0] + u[:, n - 1]
                den = 1.0 + alpha
                assert np.all(den != 0.0)
                dens.append(float(np.min(np.abs(den))))
                beta = (y[:, 0] + y[:, n - 1]) / den
                y = y - beta[:, None] * u
            ql[rows, 1:n + 1] = y
        if ibc:
            wrap(q, ibc)
    if stats is not None:
        stats["worst"] = max(stats.get("worst", 0.0), worst)
        if dens:
            stats["den"] = min([stats.get("den", np.inf)] + dens)
    return q


# ---------------------------------------------------------------- the generic recurrence (cedar_amd_affine_lines)
def make_affine(n, seed, with_div, nlines=3, pad=3):
    """y, a, div (or None) of shape (nlines, n + pad): a in {-1, +1}, y integers, div powers of two; the pad cells of each
    row hold integers that the kernel must leave alone.  Line 0 has no zero multiplier (products cross every wavefront
    and tile), line 1 one at each end of the second tile in either direction, the others one about every 300 entries"""
    rng = np.random.default_rng(seed)
    shp = (nlines, n + pad)
    y = rng.integers(-8, 9, shp).astype(np.float64)
    a = rng.choice([-1.0, 1.0], shp)
    a[2:][rng.random((nlines - 2, n + pad)) < 1.0 / 300.0] = 0.0
    ends = [p for p in (2048, 4095, n - 1 - 2048, n - 1 - 4095) if 0 <= p < n]
    a[1, ends] = 0.0
    div = rng.choice([0.5, 1.0, 2.0, 4.0], shp) if with_div else None
    _freeze(y, a)
    if div is not None:
        _freeze(div)
    return y, a, div


def affine_reference(y, a, div, n, reverse):
    """forward y_i = a_i y_(i-1) + c_i from y_(-1) = 0, or backward y_i = a_i y_(i+1) + c_i from y_n = 0, with c = y (/ div),
    one unknown after the other on the first n cells of each row; the exactness condition asserted"""
    out = y.copy()
    c = y[:, :n] / div[:, :n] if div is not None else y[:, :n].copy()
    assert np.all(np.isin(a, (-1.0, 0.0, 1.0))) and scaled_sum(c) < LIMIT
    v = np.zeros(y.shape[0])
    for r in range(n):
        i = n - 1 - r if reverse else r
        v = a[:, i] * v + c[:, i]
        out[:, i] = v
    return out


# ---------------------------------------------------------------- the scan, restated
def sequential(c, a):
    """y_i = a_i y_(i-1) + c_i, y_(-1) = 0"""
    y = np.empty(len(c))
    v = 0.0
    for i in range(len(c)):
        v = a[i] * v + c[i]
        y[i] = v
    return y


def lanes_for(n):
    return WAVE if n <= 512 else 256


DEFECTS = ("ks", "wave", "tile")


def scan_restated(c, a, bs, defect=None):
    """affine_scan and its caller's tile loop in numpy, in the kernel's association: lane t of a tile of bs * 8 unknowns
    composes its chunk, the composites are scanned by Kogge-Stone over each wavefront, the wavefronts are chained through
    their last lanes' composites (wa, wc), and the last lane's result is the carry into the next tile.  Planted defects:
      "ks"    the Kogge-Stone step updates c but not the multiplier product a
      "wave"  the chain over the wavefronts drops wa[u] * y at every hop (u runs over the wavefronts before w, never the
              last one)
      "tile"  the carry out of a tile is formed as if nothing had entered the tile: what crossed it whole is lost"""
    n = len(c)
    y = np.empty(n)
    carry = 0.0
    nw = bs // WAVE
    for base in range(0, n, bs * CH):
        m = min(n - base, bs * CH)
        am, cm = np.zeros(bs * CH), np.zeros(bs * CH)
        am[:m], cm[:m] = a[base:base + m], c[base:base + m]
        am, cm = am.reshape(bs, CH), cm.reshape(bs, CH)
        A, C = np.ones(bs), np.zeros(bs)
        for k in range(CH):
            C = am[:, k] * C + cm[:, k]
            A = am[:, k] * A
        A, C = A.reshape(nw, WAVE), C.reshape(nw, WAVE)
        off = 1
        while off < WAVE:
            An, Cn = A.copy(), C.copy()
            Cn[:, off:] = A[:, off:] * C[:, :-off] + C[:, off:]
            if defect != "ks":
                An[:, off:] = A[:, off:] * A[:, :-off]
            A, C = An, Cn
            off *= 2
        ae, ce = np.ones_like(A), np.zeros_like(C)
        ae[:, 1:], ce[:, 1:] = A[:, :-1], C[:, :-1]
        wa, wc = A[:, WAVE - 1], C[:, WAVE - 1]

        def entering(w, first, bad):
            v = first
            for u in range(w):
                v = wc[u] if bad else wa[u] * v + wc[u]
            return v
        cw = np.array([entering(w, carry, defect == "wave") for w in range(nw)])
        v = (ae * cw[:, None] + ce).reshape(bs)
        out = np.empty((bs, CH))
        for k in range(CH):
            v = am[:, k] * v + cm[:, k]
            out[:, k] = v
        y[base:base + m] = out.reshape(-1)[:m]
        last = cw[nw - 1] if defect != "tile" else entering(nw - 1, 0.0, False)
        carry = wa[nw - 1] * last + wc[nw - 1]
    return y


def sweep_recurrences(case, ud=UP):
    """(c, a) of the forward and of the backward recurrence of every line of the first colour of a Dirichlet sweep, the
    backward one in scan order (reversed positions)"""
    f = factors_of(case)
    nl = f.shape[1] - 2
    rows = list(range(2 if ud == DOWN else 1, nl + 1, 2))  # UP: the lines 0, 2, 4
    n = case.n
    rhs = line_rhs(case, case.q0, rows)
    out = []
    for k, r in enumerate(rows):
        dd, e = f[0][r, 1:n + 1], f[1][r, 2:n + 1]
        a_f = np.concatenate([[0.0], -e])
        y = sequential(rhs[k], a_f)
        a_b = np.concatenate([[0.0], -e[::-1]])
        out.append(((rhs[k], a_f), ((y / dd)[::-1].copy(), a_b)))
    return out
