// The 3D periodic solve-phase kernels on a batch of right-hand sides that share ONE operator (solver.cpp: handles of
// cedar_amd_solver_create_many_periodic).  periodic3d.hip is the Dirichlet kernels plus ghost
// refreshes; this unit is many3d.hip plus the same refreshes, taken for all items in one launch (wrap3_xy_kernel and
// wrap3_z_kernel take the array from blockIdx.y with the stride of one level vector, so a batch must be stored with
// stride II*JJ*KK -- every caller here does):
//   relax3_gs_per_many    27-point: the four row-class launches; with x periodic the row task refreshes the x ghosts of
//                         its row per item (relax27_row_task_many_perx below), else the class launch of many3d.hip; after
//                         each class the y refresh of the rows and planes it visited, at the end of the sweep the z
//                         refresh.  7-point: relax7_colour_many per colour, each followed by the x / y refresh.
//   restrict3_per_many    ghost refresh of the fine vectors (y, x, z), then restrict3_many
//   interp_add3_per_many  interp_add3_many, then the refresh
//   solve_cg3_per_many    the dense coarsest solve, one workgroup per item, the factor shared
// Arithmetic: per item exactly the expressions and the operation order of the single-vector periodic kernels
// (relax27_row_task<.., PERX>, solve_cg3_per_kernel), -ffp-contract=off: item m's result has the bits of the
// single-vector periodic call on item m alone.
#include "common.h"
#include "relax27_dev.h"

namespace cedar_amd {

// ------------------------------------------------------------------ 27-point sweep, x periodic
// relax27_row_task_many (many3d.hip) with the x-ghost refresh of relax27_row_task<.., PERX> (relax27_dev.h) per item: the
// row has an EVEN number of points; the last point of the second i-colour takes the fresh first point of the row from
// LDS (EFIRST; the other order: the first point takes the fresh last one), and the two ghost cells of the row are
// written.  Coefficients and reciprocals of the lane's pair stay in registers across the item loop.  xch: two LDS rows
// used in turn -- everything an item reads from its row (x[p+1], x[0], x[(II-2)/2]) is read between its own barrier
// and the next item's, and the row is next written two items later: one __syncthreads per item is enough.
template <int BS, bool EFIRST>
__device__ __forceinline__ void relax27_row_task_many_perx(const Op3 &A, const real_t *__restrict__ qf, real_t *__restrict__ q,
                                                           int II, size_t sj, size_t sk, size_t j, size_t k,
                                                           real_t (*xch)[BS + 2], int nitems, size_t stride)
{
	const size_t row = j * sj + k * sk, rowA = j * A.SJ + k * A.SK;
	const int p = threadIdx.x;
	const int ie = 2 * p + 1, io = 2 * p + 2;
	const bool e_ok = ie <= II - 2, o_ok = io <= II - 2;
	const bool two = io + 1 <= II - 1;

	C27 ce, co;
	real_t sre = 0, sro = 0;
	if (e_ok) {
		load_coef27<true, true, true>(A, rowA, ie, io, two, ce, co);
		real_t a_, b_;
		ldpair(A.sor + j * A.rSJ + k * A.rSK + ie, true, a_, b_); sre = a_; sro = b_;
	}
#pragma unroll 1
	for (int m = 0; m < nitems; m++) {
		const real_t *__restrict__ qfm = qf + (size_t)m * stride;
		real_t *__restrict__ qm = q + (size_t)m * stride;
		real_t *x = xch[m & 1];
		real_t e_new = 0.0, o_new = 0.0;
		real_t qe[3][3][3], qo[3][3][3];
		real_t qfe = 0, qfo = 0;
		if (e_ok) load_vec27<0>(qfm, qm, row, sj, sk, ie, io, two, qe, qo, qfe, qfo);
		if (EFIRST) {
			if (e_ok) {
				e_new = offdiag27(qfe, ce, qe) * sre;
				x[p] = e_new;
			}
			__syncthreads();
			if (o_ok) {
				qo[1][1][0] = e_new;
				if (io + 1 <= II - 2) qo[1][1][2] = x[p + 1]; // next pair's fresh e
				else qo[1][1][2] = x[0];                      // periodic: the ghost was refreshed with the row's first point
				o_new = offdiag27(qfo, co, qo) * sro;
			}
			if (o_ok && io == II - 2) { // the two ghost cells: left = last point, right = first point
				qm[row] = o_new;
				qm[row + II - 1] = x[0];
			}
		} else {
			if (o_ok) {
				o_new = offdiag27(qfo, co, qo) * sro;
				x[p + 1] = o_new;
			}
			__syncthreads();
			if (e_ok) {
				if (p > 0) qe[1][1][0] = x[p];       // previous pair's fresh o
				else qe[1][1][0] = x[(II - 2) / 2];  // periodic: the ghost was refreshed with the row's last point
				if (o_ok) qe[1][1][2] = o_new;
				e_new = offdiag27(qfe, ce, qe) * sre;
			}
			if (p == 0 && e_ok) {
				qm[row] = x[(II - 2) / 2];
				qm[row + II - 1] = e_new;
			}
		}
		if (e_ok) {
			if (o_ok) {
				d2u v; v.x = e_new; v.y = o_new;
				*reinterpret_cast<d2u *>(qm + row + ie) = v;
			} else {
				qm[row + ie] = e_new;
			}
		}
	}
}

// one workgroup = one grid row of the class (jb,kb), all items (relax27_rows_many of many3d.hip)
template <int BS, bool EFIRST>
__global__ __launch_bounds__(BS) void relax27_rows_many_perx(const Op3 A, const real_t *__restrict__ qf, real_t *__restrict__ q,
                                                              int II, int JJ, int KK, int jb, int kb, int nrj, int nrk,
                                                              TileShape ts, int nitems, size_t stride)
{
	__shared__ real_t xch[2][BS + 2];
	const unsigned nblk = tile_blocks((unsigned)nrj, (unsigned)nrk, ts);
	const unsigned L = xcd_remap(blockIdx.x, nblk);
	unsigned jr, kr;
	if (L >= nblk || !tile_rows(L, (unsigned)nrj, (unsigned)nrk, ts, jr, kr)) return; // whole workgroup leaves together
	const size_t j = (size_t)(1 + jb + 2 * (int)jr), k = (size_t)(1 + kb + 2 * (int)kr);
	relax27_row_task_many_perx<BS, EFIRST>(A, qf, q, II, (size_t)II, (size_t)II * JJ, j, k, xch, nitems, stride);
}

template <int BS>
static void launch_rows_many_perx(bool efirst, const Op3 &A, const real_t *qf, real_t *q, int II, int JJ, int KK, int jb, int kb,
                                  hipStream_t st, Batch bt)
{
	const int nrj = (JJ - 2 - jb + 1) / 2, nrk = (KK - 2 - kb + 1) / 2;
	if (nrj <= 0 || nrk <= 0) return;
	const TileShape ts = tile_shape_relax();
	const unsigned grid = xcd_grid(tile_blocks((unsigned)nrj, (unsigned)nrk, ts));
	if (efirst) hipLaunchKernelGGL((relax27_rows_many_perx<BS, true>), dim3(grid), dim3(BS), 0, st, A, qf, q, II, JJ, KK, jb, kb, nrj, nrk, ts, bt.n, bt.stride);
	else hipLaunchKernelGGL((relax27_rows_many_perx<BS, false>), dim3(grid), dim3(BS), 0, st, A, qf, q, II, JJ, KK, jb, kb, nrj, nrk, ts, bt.n, bt.stride);
}

// relax3_gs_per (relax3d.hip) on a batch.  The conditions of the row-class path are its own: 27-point, even extents in
// the periodic directions, y ghosts consistent on entry when y is periodic, at most 512 pairs per row.  Where they do
// not hold the items walk through the single-vector colour launches one by one (relax3_gs_per itself: the first
// pre-smoothing sweep on a caller's x with y periodic, odd periodic extents, rows longer than 1024 points).
void relax3_gs_per_many(const real_t *so, const real_t *qf, real_t *q, const real_t *sor, int II, int JJ, int KK, int nstncl,
                        int updown, int ipn, hipStream_t st, int ghosts_consistent, Batch bt)
{
	if (II < 3 || JJ < 3 || KK < 3 || bt.n < 1) return;
	const bool up = (updown == BMG_UP);
	const PerDirs pd = per_dirs(3, ipn); // the one table of the boundary codes (common.h)
	const bool px = pd.x, py = pd.y, pz = pd.z;
	const bool batched = bt.stride == (size_t)II * JJ * KK; // the refresh kernels' array stride
	if (nstncl != 14 && batched) {
		for (int c = 0; c < 2; c++) {
			relax3_colour7_many(so, qf, q, sor, II, JJ, KK, up ? c : 1 - c, st, bt);
			wrap3_colour(q, II, JJ, KK, -1, -1, ipn, st, bt.n);
		}
		wrap3_sweep_end(q, II, JJ, KK, ipn, st, bt.n);
		return;
	}
	if (nstncl == 14 && batched && !(px && (II & 1)) && (!py || ghosts_consistent) && !(py && (JJ & 1)) && !(pz && (KK & 1))
	    && (II - 2 + 1) / 2 <= 512) {
		const Op3 A = op3_cedar(so, sor, II, JJ, KK);
		const int npairs = (II - 2 + 1) / 2;
		const int ycode = (py ? 1 : 0) + (pz ? (py ? 6 : 5) : 0); // the code without x (the row task did x): 0, 1 y, 5 z, 7 yz
		for (int c = 0; c < 4; c++) {
			const int cc = up ? c : 3 - c, jb = cc & 1, kb = cc >> 1;
			if (!px) relax3_class27_many(A, qf, q, II, JJ, KK, jb, kb, up, st, bt);
			else if (npairs <= 64) launch_rows_many_perx<64>(up, A, qf, q, II, JJ, KK, jb, kb, st, bt);
			else if (npairs <= 128) launch_rows_many_perx<128>(up, A, qf, q, II, JJ, KK, jb, kb, st, bt);
			else if (npairs <= 256) launch_rows_many_perx<256>(up, A, qf, q, II, JJ, KK, jb, kb, st, bt);
			else launch_rows_many_perx<512>(up, A, qf, q, II, JJ, KK, jb, kb, st, bt);
			wrap3_colour(q, II, JJ, KK, jb, kb, ycode, st, bt.n);
		}
		wrap3_sweep_end(q, II, JJ, KK, ipn, st, bt.n);
		return;
	}
	for (int m = 0; m < bt.n; m++)
		relax3_gs_per(so, qf + m * bt.stride, q + m * bt.stride, sor, II, JJ, KK, nstncl, updown, ipn, st, ghosts_consistent);
}

// ------------------------------------------------------------------ transfers
void restrict3_per_many(real_t *q, real_t *qc, const real_t *ci, int II, int JJ, int KK, int IIC, int JJC, int KKC, int ipn,
                        hipStream_t st, Batch bf, Batch bc)
{
	wrap3(q, II, JJ, KK, bf.n, ipn, st);
	restrict3_many(q, qc, ci, II, JJ, KK, IIC, JJC, KKC, st, bf, bc);
}

void interp_add3_per_many(real_t *q, const real_t *qc, const real_t *so, real_t *res, const real_t *ci, int IIC, int JJC,
                          int KKC, int IIF, int JJF, int KKF, int ipn, hipStream_t st, Batch bf, Batch bc)
{
	interp_add3_many(q, qc, so, res, ci, IIC, JJC, KKC, IIF, JJF, KKF, st, bf, bc);
	wrap3(q, IIF, JJF, KKF, bf.n, ipn, st);
}

// ------------------------------------------------------------------ coarsest grid
#define ABD(r, c) abd[(size_t)(r) + (size_t)nabd1 * (size_t)(c)]

// solve_cg3_per_kernel (periodic3d.hip) with the item in blockIdx.x: DPOTRS 'U' in dtrsm.f's operation order, the
// sequential mean sum by one lane, then the three ghost phases with their barriers.  The factor is shared; item m
// works on q + m * stride, qf + m * stride and its own bbd segment of N doubles.
__global__ __launch_bounds__(1024) void solve_cg3_per_many_kernel(real_t *__restrict__ q, const real_t *__restrict__ qf,
                                                                  int II, int JJ, int KK, const real_t *__restrict__ abd,
                                                                  real_t *__restrict__ bbd, int nabd1, PerDirs pd, size_t stride)
{
	const int nx = II - 2, ny = JJ - 2, nz = KK - 2, N = nx * ny * nz;
	const int tid = threadIdx.x, nt = blockDim.x;
	q += (size_t)blockIdx.x * stride;
	qf += (size_t)blockIdx.x * stride;
	bbd += (size_t)blockIdx.x * (size_t)N;
#define XOF(r) ((size_t)(1 + (r) % nx) + (size_t)II * ((size_t)(1 + ((r) / nx) % ny) + (size_t)JJ * (size_t)(1 + (r) / (nx * ny))))
	for (int r = tid; r < N; r += nt) bbd[r] = qf[XOF(r)];
	__syncthreads();
	// forward: b_i = (b_i - sum_{k<i} U(k,i) b_k) / U(i,i), the sum taken in increasing k for every i
	for (int k = 0; k < N; k++) {
		if (tid == 0) bbd[k] = bbd[k] / ABD(k, k);
		__syncthreads();
		const real_t bk = bbd[k];
		for (int i = k + 1 + tid; i < N; i += nt) bbd[i] = bbd[i] - ABD(k, i) * bk;
		__syncthreads();
	}
	for (int k = N - 1; k >= 0; k--) {
		if (tid == 0 && bbd[k] != 0.0) bbd[k] = bbd[k] / ABD(k, k);
		__syncthreads();
		const real_t bk = bbd[k];
		if (bk != 0.0)
			for (int i = tid; i < k; i += nt) bbd[i] = bbd[i] - bk * ABD(i, k);
		__syncthreads();
	}
	__shared__ real_t cshift;
	if (tid == 0) {
		real_t cint = 0.0, qint = 0.0;
		for (int r = 0; r < N; r++) {
			qint = qint + bbd[r];
			cint = cint + 1;
		}
		cshift = -qint / cint;
	}
	__syncthreads();
	for (int r = tid; r < N; r += nt) q[XOF(r)] = bbd[r] + cshift;
	__syncthreads();
#undef XOF
	const size_t P = (size_t)II * JJ;
	if (pd.x)
		for (int t = tid; t < JJ * KK; t += nt) {
			real_t *row = q + (size_t)II * t;
			row[0] = row[II - 2];
			row[II - 1] = row[1];
		}
	__syncthreads();
	if (pd.y)
		for (int t = tid; t < II * KK; t += nt) {
			real_t *p = q + P * (size_t)(t / II) + (t % II);
			p[0] = p[(size_t)II * (JJ - 2)];
			p[(size_t)II * (JJ - 1)] = p[II];
		}
	__syncthreads();
	if (pd.z)
		for (int t = tid; t < II * JJ; t += nt) {
			q[t] = q[t + P * (size_t)(KK - 2)];
			q[t + P * (size_t)(KK - 1)] = q[t + P];
		}
}
#undef ABD

// bbd: bt.n segments of (II-2)(JJ-2)(KK-2) doubles
void solve_cg3_per_many(real_t *q, const real_t *qf, int II, int JJ, int KK, const real_t *abd, real_t *bbd, int nabd1, int ipn,
                        hipStream_t st, Batch bt)
{
	if (bt.n < 1) return;
	hipLaunchKernelGGL(solve_cg3_per_many_kernel, dim3(bt.n), dim3(1024), 0, st, q, qf, II, JJ, KK, abd, bbd, nabd1, per_dirs(3, ipn),
	                   bt.stride);
}

} // namespace cedar_amd
