// The 2D periodic sweep on a batch of right-hand sides that share ONE operator (solver.cpp: handles of
// cedar_amd_solver_create_many_periodic2).  periodic2d.hip is the single-vector set; this unit keeps
// its launch order and serves all items inside a task, so that the operator entries of a task go to HBM once:
//   relax2_gs_per_many    relax2_gs_per's launches (row classes for nine-point, jo passes for five-point, DOWN / UP).  Rows
//                         of up to 512 interior points: one workgroup per grid row and all items in it; longer rows: one
//                         launch per i-colour, a lane per point, followed by the x wrap of those rows.  Then the y wrap of
//                         all items in one wrap2 launch
// (wrap2_kernel takes the plane from blockIdx.x with the stride of one level vector, so a batch must be stored with stride
// II*JJ -- every caller here does; any other stride walks the items through the single-vector launches.)
// The transfers and the dense coarsest solve of a batch are periodic2d.hip's own: restrict2_per, interp_add2_per and
// solve_cg2_per take the batch.
// Arithmetic: per item exactly the expressions and the operation order of the single-vector kernel (relax2_per_kernel),
// -ffp-contract=off: item m's result has the bits of the single-vector periodic call on item m alone.
#include "common.h"

namespace cedar_amd {

namespace {

// rows of at most this many interior points give a lane of the 256 at most one point per colour
constexpr int RELAX2_PER_MANY_ONE = 512;

// what a point of the sweep reads of the operator: the row-neighbour pair, the two (nine-point: six) entries towards the
// rows below and above, and 1/diag
template <bool NINE>
struct C2 {
	real_t w, e, s, n, sw, se, nw, ne, d;
};

template <bool NINE>
__device__ __forceinline__ C2<NINE> load_c2(const real_t *__restrict__ so, const real_t *__restrict__ sor, size_t PS, size_t sj,
                                            size_t x)
{
	C2<NINE> c;
	c.w = so[KW * PS + x];
	c.e = so[KW * PS + x + 1];
	c.s = so[KS * PS + x];
	c.n = so[KS * PS + x + sj];
	if (NINE) {
		c.sw = so[KSW * PS + x];
		c.se = so[KNW * PS + x + 1];
		c.nw = so[KNW * PS + x + sj];
		c.ne = so[KSW * PS + x + 1 + sj];
	} else {
		c.sw = c.se = c.nw = c.ne = 0.0;
	}
	c.d = sor[PS + x];
	return c;
}

// relax2_per_kernel's expression for the point at x: l / r are its row neighbours (from the LDS row there), the other
// rows are read from q
template <bool NINE>
__device__ __forceinline__ real_t relax_pt2(const C2<NINE> &c, real_t f, real_t l, real_t r, const real_t *q, size_t x,
                                            size_t sj)
{
	real_t s = f;
	s = s + c.w * l;
	s = s + c.e * r;
	s = s + c.s * q[x - sj];
	s = s + c.n * q[x + sj];
	if (NINE) {
		s = s + c.sw * q[x - 1 - sj];
		s = s + c.se * q[x + 1 - sj];
		s = s + c.nw * q[x - 1 + sj];
		s = s + c.ne * q[x + 1 + sj];
	}
	return s * c.d;
}

// the row's fresh value v of point i (1-based) goes to q, and with x periodic to the ghost cell that mirrors it: what
// relax2_per_kernel's row[0] = row[I1-1]; row[II-1] = row[1] after the last colour and its write-back of the whole row do
__device__ __forceinline__ void put_pt2(real_t *q, size_t r0, int i, int II, bool px, real_t v)
{
	q[r0 + (size_t)(i - 1)] = v;
	if (px && i == II - 1) q[r0] = v;
	if (px && i == 2) q[r0 + (size_t)(II - 1)] = v;
}

// relax2_per_kernel on all items of the task, for rows of at most 512 interior points (a lane of the 256 owns at most one
// point per colour): one workgroup per grid row j = jbeg + jstep * blockIdx.x.  NINE: both i-colours of the row (IBEG =
// first, then 5 - first); five point: the colour (j + first) % 2 + 2 of this pass.
// The x wrap after each colour is folded into the reads and the write-back: the second colour reads the row's ghost
// cells at the opposite interior end (the LDS row is not written after the first colour, so that is the value the wrap
// would have copied), and the last values of points I1 and 2 go to the two ghost cells of q as well.
// The coefficients and 1/diag of the lane's points stay in registers across the item loop; the first colour reads its old
// row neighbours from q, and LDS only carries the row from the first colour to the second -- two rows used in turn: item m
// writes xch[m & 1] before its barrier and reads it after, the row is next written two items later, behind the barrier of
// item m + 1, so one __syncthreads per item is enough.  All writes to q come after the item's barrier, all reads of the
// item's own row before.
template <bool NINE>
__global__ __launch_bounds__(256) void relax2_per_many(const real_t *__restrict__ so, const real_t *__restrict__ qf,
                                                        real_t *__restrict__ q, const real_t *__restrict__ sor, int II, int JJ,
                                                        int jbeg, int jstep, int first, int ipn, int nitems, size_t stride)
{
	extern __shared__ real_t xch[];
	const int j = jbeg + jstep * (int)blockIdx.x; // 1-based
	if (j > JJ - 1) return; // whole workgroup leaves together
	const size_t sj = II, PS = (size_t)II * JJ;
	const size_t r0 = sj * (size_t)(j - 1); // offset of Q(1,j)
	const int I1 = II - 1;
	const bool px = per_dirs(2, ipn).x;
	const int ib0 = NINE ? first : (j + first) % 2 + 2, ib1 = 5 - first; // the colours' first points (1-based)
	const int t = threadIdx.x;

	const int a = ib0 + 2 * t, b = ib1 + 2 * t;
	const bool a_ok = a <= I1, b_ok = NINE && b <= I1;
	const size_t xa = r0 + (size_t)(a - 1), xb = r0 + (size_t)(b - 1);
	C2<NINE> ca{}, cb{};
	if (a_ok) ca = load_c2<NINE>(so, sor, PS, sj, xa);
	if (b_ok) cb = load_c2<NINE>(so, sor, PS, sj, xb);
#pragma unroll 1
	for (int m = 0; m < nitems; m++) {
		const real_t *__restrict__ qfm = qf + (size_t)m * stride;
		real_t *__restrict__ qm = q + (size_t)m * stride;
		real_t *row = xch + (size_t)(m & 1) * II;
		real_t va = 0.0;
		if (a_ok) va = relax_pt2<NINE>(ca, qfm[xa], qm[xa - 1], qm[xa + 1], qm, xa, sj);
		if (NINE) { // the row as it stands after the first colour
			if (a_ok) row[a - 1] = va;
			if (b_ok) row[b - 1] = qm[xb];
			if (t == 0) {
				row[0] = qm[r0];
				row[II - 1] = qm[r0 + (size_t)(II - 1)];
			}
		}
		__syncthreads();
		if (b_ok) {
			const real_t l = row[px && b == 2 ? I1 - 1 : b - 2], r = row[px && b == I1 ? 1 : b];
			put_pt2(qm, r0, b, II, px, relax_pt2<NINE>(cb, qfm[xb], l, r, qm, xb, sj));
		}
		if (a_ok) put_pt2(qm, r0, a, II, px, va);
		if (!NINE && px && t == 0) { // a ghost whose mirror point is not of this pass' colour takes its standing value
			if ((I1 - ib0) & 1) qm[r0] = qm[r0 + (size_t)(I1 - 1)];
			if (ib0 != 2) qm[r0 + (size_t)(II - 1)] = qm[r0 + 1];
		}
	}
}

// Rows of more than 512 interior points: one i-colour of the rows j = jbeg + jstep * blockIdx.x per launch, a lane owns
// ONE point of it (256 points per workgroup, blockIdx.y the segment) and keeps its coefficients and 1/diag in registers
// across the item loop.  A point of the colour reads only points of the other colour in its row (nine-point: after the
// first colour's launch they are fresh, as in the LDS row of relax2_per_kernel) and other rows, none of which this launch
// writes, and no ghost cell is written here: no LDS, no barrier.  The x wrap the single kernel makes after each colour
// is the launch of wrapx_rows_many below on the same rows.
template <bool NINE>
__global__ __launch_bounds__(256) void relax2_per_many_colour(const real_t *__restrict__ so, const real_t *__restrict__ qf,
                                                               real_t *__restrict__ q, const real_t *__restrict__ sor, int II,
                                                               int JJ, int jbeg, int jstep, int first, int nitems, size_t stride)
{
	const int j = jbeg + jstep * (int)blockIdx.x; // 1-based
	if (j > JJ - 1) return;
	const int ib = NINE ? first : (j + first) % 2 + 2;
	const int i = ib + 2 * (int)(blockIdx.y * blockDim.x + threadIdx.x);
	if (i > II - 1) return;
	const size_t sj = II, PS = (size_t)II * JJ;
	const size_t x = sj * (size_t)(j - 1) + (size_t)(i - 1);
	const C2<NINE> c = load_c2<NINE>(so, sor, PS, sj, x);
#pragma unroll 1
	for (int m = 0; m < nitems; m++) {
		const real_t *__restrict__ qfm = qf + (size_t)m * stride;
		real_t *qm = q + (size_t)m * stride;
		qm[x] = relax_pt2<NINE>(c, qfm[x], qm[x - 1], qm[x + 1], qm, x, sj);
	}
}

// Q(1,j) = Q(I1,j), Q(II,j) = Q(2,j) on the rows j = jbeg + jstep * r, r < nrows, of every item
__global__ __launch_bounds__(256) void wrapx_rows_many(real_t *__restrict__ q, int II, int JJ, int jbeg, int jstep, int nrows,
                                                        size_t stride)
{
	const int r = blockIdx.x * blockDim.x + threadIdx.x;
	const int j = jbeg + jstep * r;
	if (r >= nrows || j > JJ - 1) return;
	real_t *row = q + (size_t)blockIdx.y * stride + (size_t)II * (size_t)(j - 1);
	row[0] = row[II - 2];
	row[II - 1] = row[1];
}

template <bool NINE>
void launch_relax2_per_many(int nrows, const real_t *so, const real_t *qf, real_t *q, const real_t *sor, int II, int JJ, int jbeg,
                            int jstep, int first, int ipn, hipStream_t st, Batch bt)
{
	if (nrows <= 0) return;
	const size_t rowb = (size_t)II * sizeof(real_t);
	if (II - 2 <= RELAX2_PER_MANY_ONE) {
		const size_t shm = NINE ? 2 * rowb : 0;
		hipLaunchKernelGGL(relax2_per_many<NINE>, dim3(nrows), dim3(256), shm, st, so, qf, q, sor, II, JJ, jbeg, jstep, first, ipn,
		                   bt.n, bt.stride);
		return;
	}
	const bool px = per_dirs(2, ipn).x;
	const int nseg = ((II - 2 + 1) / 2 + 255) / 256; // a colour has at most ceil((II-2)/2) points
	for (int c = 0; c < (NINE ? 2 : 1); c++) {
		hipLaunchKernelGGL(relax2_per_many_colour<NINE>, dim3(nrows, nseg), dim3(256), 0, st, so, qf, q, sor, II, JJ, jbeg, jstep,
		                   NINE && c == 1 ? 5 - first : first, bt.n, bt.stride);
		if (px) hipLaunchKernelGGL(wrapx_rows_many, dim3((nrows + 255) / 256, bt.n), dim3(256), 0, st, q, II, JJ, jbeg, jstep, nrows, bt.stride);
	}
}

} // namespace

// relax2_gs_per (periodic2d.hip) on a batch: its launch order, then the y wrap of every item in one launch
int relax2_gs_per_many(const real_t *so, const real_t *qf, real_t *q, const real_t *sor, int II, int JJ, int nstncl, int updown,
                       int ipn, hipStream_t st, Batch bt)
{
	if (II < 3 || JJ < 3 || bt.n < 1) return 0;
	if ((size_t)II * sizeof(real_t) > 64 * 1024) return 1; // what relax2_gs_per serves: the batch follows the single-vector handle
	if (bt.stride != (size_t)II * JJ) { // not the stride of wrap2's planes: item by item
		for (int m = 0; m < bt.n; m++)
			if (relax2_gs_per(so, qf + m * bt.stride, q + m * bt.stride, sor, II, JJ, nstncl, updown, ipn, st)) return 1;
		return 0;
	}
	const int J1 = JJ - 1;
	const bool down = updown == BMG_DOWN;
	if (nstncl == 5) {
		for (int c = 0; c < 2; c++) {
			const int jbeg = down ? 2 + c : 3 - c; // LSTART..LEND
			if (jbeg > J1) continue;
			launch_relax2_per_many<true>((J1 - jbeg) / 2 + 1, so, qf, q, sor, II, JJ, jbeg, 2, down ? 2 : 3, ipn, st, bt);
		}
	} else {
		for (int c = 0; c < 2; c++) launch_relax2_per_many<false>(J1 - 1, so, qf, q, sor, II, JJ, 2, 1, down ? 2 + c : 3 - c, ipn, st, bt);
	}
	if (per_dirs(2, ipn).y) wrap2(q, II, JJ, bt.n, 1, 0, st);
	return 0;
}

} // namespace cedar_amd
