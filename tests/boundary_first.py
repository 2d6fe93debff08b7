"""The order in which the boundary-first pieces of a 27-point sweep are called on one k-parity of planes (dist3.cpp
chain_parity without the exchanges), shared by the tests that run cedar_amd_relax3_rows / _cols / _cols_strip /
_planes_masked on a single box."""


def chain_parity(nx, ny, sides, kb, up, rows, cols, masked):
    """sides = (-x, +x, -y, +y): which faces of the box of nx x ny owned points per plane have a neighbour.  The columns
    and rows that such a neighbour would make chain points are relaxed ahead, stage by stage, the rest by the masked
    launch.  Calls, in order,
      rows(j0, jstep, nrj, kb, up)       cedar_amd_relax3_rows
      cols(jb, kb, columns, xrow0, xrow1) cedar_amd_relax3_cols or _cols_strip (never with an empty column list)
      masked(kb, up, cols_f, cols_s, skip_rows) cedar_amd_relax3_planes_masked
    and returns what masked returned."""
    jbF = 0 if up else 1
    c1, c2, colsS, fixc, mF, mS = [], [], [], [], 0, 0
    for side in (0, 1):
        if not sides[side]:
            continue
        col = (lambda d: nx - d) if side else (lambda d: 1 + d)
        bit = (lambda d: 1 << (7 - d)) if side else (lambda d: 1 << d)
        if (side == 0) == up:  # side P
            c1 += [col(0), col(2)]; c2 += [col(1)]; colsS += [col(0)]
            mF |= bit(0) | bit(1) | bit(2); mS |= bit(0)
        else:
            c1 += [col(1), col(3)]; c2 += [col(2), col(0)]; colsS += [col(1), col(0)]; fixc += [col(0)]
            mF |= bit(0) | bit(1) | bit(2) | bit(3); mS |= bit(0) | bit(1)
    rowsF, rowS = [], -1
    for side in (0, 1):
        if not sides[2 + side]:
            continue
        row = (lambda d: ny - d) if side else (lambda d: 1 + d)
        if (side == 0) == up:
            rowsF.append(row(0))
        else:
            rowsF.append(row(1)); rowS = row(0)
    skip = [rowsF[0] if rowsF else -1, rowsF[1] if len(rowsF) > 1 else -1, rowS]

    def some_cols(jb, cl, x0=-1, x1=-1):
        if cl:
            cols(jb, kb, cl, x0, x1)

    if rowsF:
        rows(rowsF[0], rowsF[1] - rowsF[0] if len(rowsF) > 1 else 2, len(rowsF), kb, int(up))
    some_cols(jbF, c1 + c2, skip[0], skip[1])
    some_cols(jbF, fixc)
    if rowS >= 0:
        rows(rowS, 2, 1, kb, int(up))
    some_cols(1 - jbF, colsS, rowS, -1)
    some_cols(1 - jbF, fixc)
    return masked(kb, int(up), mF, mS, skip)
