// The 3D solve-phase kernels on a batch of right-hand sides that share ONE operator (common.h Batch; solver.cpp
// cedar_amd_solver_*_many).  Every level-0 kernel of the 3D cycle is bound by HBM bytes and most of them are the operator
// (27-point sweep: 26 of ~29 doubles per point), so a workgroup task fetches its operator entries -- the C27 coefficient
// sets and 1/diag of a lane's point pair, the 26 CI entries of a coarse point, the diagonal -- into registers ONCE and then
// walks the items doing only the vector part.  Item m of a vector starts m * stride doubles into the array.
//
// Arithmetic: per item exactly the expressions of the single-vector kernels (relax3d.hip, residual.hip, transfer.hip) in
// the reference's term order, -ffp-contract=off: item m's result has the bits of the single-vector reference-order
// computation on item m alone.  No partial sums here (relax3d_psum.hip re-associates; with the operator amortised over
// the items it would buy little).
#include "common.h"
#include "relax27_dev.h"
#include "transfer_dev.h"
#include <type_traits>

namespace cedar_amd {

// ------------------------------------------------------------------ 27-point sweep
// relax27_row_task for a batch: lane p relaxes the pair (2p+1, 2p+2) of row (j,k) of every item, both i-colours.  The
// coefficients and reciprocals stay in registers across the item loop, the q windows are per item.  xch: two LDS rows
// of BS+2 doubles used in turn, so that an item's first-colour values are not overwritten while a slower wave still
// reads the previous item's (one __syncthreads per item; every wave of the workgroup must call this).
// OP: the operator view, Op3 or the single-precision Op3f (common.h; entries promoted to double by the pair loads, so
// the items see the FP64 sweep of the operator rounded to float).
// PERX: the x-ghost refresh of relax27_row_task<.., PERX> (relax27_dev.h) per item, for the periodic batch
// (periodic_many3d.hip): the row has an EVEN number of points; the last point of the second i-colour takes the fresh first
// point of the row from LDS (EFIRST; the other order: the first point takes the fresh last one), and the two ghost cells
// of the row are written.  Everything an item reads from its LDS row (x[p+1], x[0], x[(II-2)/2]) is read between its own
// barrier and the next item's, and the row is next written two items later: one __syncthreads per item is still enough.
template <int BS, bool EFIRST, bool NT, bool PERX = false, typename OP = Op3>
__device__ __forceinline__ void relax27_row_task_many(const OP &A, const real_t *__restrict__ qf, real_t *__restrict__ q,
                                                      int II, size_t sj, size_t sk, size_t j, size_t k, real_t (*xch)[BS + 2],
                                                      int nitems, size_t stride)
{
	const size_t row = j * sj + k * sk, rowA = j * A.SJ + k * A.SK;
	const int p = threadIdx.x;
	const int ie = 2 * p + 1, io = 2 * p + 2;
	const bool e_ok = ie <= II - 2, o_ok = io <= II - 2;
	const bool two = io + 1 <= II - 1;

	C27 ce, co;
	real_t sre = 0, sro = 0;
	if (e_ok) {
		load_coef27<NT, NT, NT>(A, rowA, ie, io, two, ce, co);
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
				if (io + 1 <= II - 2) qo[1][1][2] = x[p + 1]; // next pair's fresh e (else ghost: old value)
				else if (PERX) qo[1][1][2] = x[0];            // periodic: the ghost was refreshed with the row's first point
				o_new = offdiag27(qfo, co, qo) * sro;
			}
			if (PERX && o_ok && io == II - 2) { // the two ghost cells: left = last point, right = first point
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
				if (p > 0) qe[1][1][0] = x[p]; // previous pair's fresh o (p == 0: ghost column)
				else if (PERX) qe[1][1][0] = x[(II - 2) / 2]; // periodic: the ghost was refreshed with the row's last point
				if (o_ok) qe[1][1][2] = o_new;
				e_new = offdiag27(qfe, ce, qe) * sre;
			}
			if (PERX && p == 0 && e_ok) {
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

// one workgroup = one grid row of the class (jb,kb), all items (relax27_rows of relax3d.hip)
template <int BS, bool EFIRST, bool NT, bool PERX = false, typename OP = Op3>
__global__ __launch_bounds__(BS) void relax27_rows_many(const OP A, const real_t *__restrict__ qf, real_t *__restrict__ q,
                                                         int II, int JJ, int KK, int jb, int kb, int nrj, int nrk, TileShape ts,
                                                         int nitems, size_t stride)
{
	__shared__ real_t xch[2][BS + 2];
	const unsigned nblk = tile_blocks((unsigned)nrj, (unsigned)nrk, ts);
	const unsigned L = xcd_remap(blockIdx.x, nblk);
	unsigned jr, kr;
	if (L >= nblk || !tile_rows(L, (unsigned)nrj, (unsigned)nrk, ts, jr, kr)) return; // whole workgroup leaves together
	const size_t j = (size_t)(1 + jb + 2 * (int)jr), k = (size_t)(1 + kb + 2 * (int)kr);
	relax27_row_task_many<BS, EFIRST, NT, PERX>(A, qf, q, II, (size_t)II, (size_t)II * JJ, j, k, xch, nitems, stride);
}

template <int BS, bool PERX = false, typename OP = Op3>
static void launch_rows_many(bool efirst, const OP &A, const real_t *qf, real_t *q, int II, int JJ, int KK, int jb, int kb,
                             hipStream_t st, Batch bt)
{
	const int nrj = (JJ - 2 - jb + 1) / 2, nrk = (KK - 2 - kb + 1) / 2;
	if (nrj <= 0 || nrk <= 0) return;
	const TileShape ts = tile_shape_relax();
	const unsigned grid = xcd_grid(tile_blocks((unsigned)nrj, (unsigned)nrk, ts));
	// operator rows are read by exactly one task of a launch: streamed past the caches as in the single-vector sweep
	if (efirst) hipLaunchKernelGGL((relax27_rows_many<BS, true, true, PERX, OP>), dim3(grid), dim3(BS), 0, st, A, qf, q, II, JJ, KK, jb, kb, nrj, nrk, ts, bt.n, bt.stride);
	else hipLaunchKernelGGL((relax27_rows_many<BS, false, true, PERX, OP>), dim3(grid), dim3(BS), 0, st, A, qf, q, II, JJ, KK, jb, kb, nrj, nrk, ts, bt.n, bt.stride);
}

// the row kernels' block size for rows of npairs <= 512 point pairs: f(BS) with BS() = 64, 128, 256 or 512
template <class F>
static void with_row_bs(int npairs, F &&f)
{
	if (npairs <= 64) f(std::integral_constant<int, 64>());
	else if (npairs <= 128) f(std::integral_constant<int, 128>());
	else if (npairs <= 256) f(std::integral_constant<int, 256>());
	else f(std::integral_constant<int, 512>());
}

template <typename OP = Op3>
static void relax3_gs27_many_t(const OP &A, const real_t *qf, real_t *q, int II, int JJ, int KK, int updown, hipStream_t st, Batch bt)
{
	if (II < 3 || JJ < 3 || KK < 3 || bt.n < 1) return;
	const bool up = (updown == BMG_UP);
	const int npairs = (II - 2 + 1) / 2;
	if (npairs > 512) { // rows too long for the row kernel: the single-vector colour kernels item by item (reference order)
		// (those kernels have no single-precision twin: a level with such rows never takes the float copy, solver.cpp, and
		// cedar_amd_relax3_gs_many_op32 refuses it)
		if constexpr (std::is_same<OP, Op3>::value)
			for (int m = 0; m < bt.n; m++) relax3_gs27_op(A, qf + m * bt.stride, q + m * bt.stride, II, JJ, KK, updown, st);
		return;
	}
	// colour pairs in sweep order: UP (j,k) parities 00,10,01,11 with even-i first; DOWN the reverse
	for (int c = 0; c < 4; c++) {
		const int cc = up ? c : 3 - c, jb = cc & 1, kb = cc >> 1;
		with_row_bs(npairs, [&](auto BS) { launch_rows_many<BS()>(up, A, qf, q, II, JJ, KK, jb, kb, st, bt); });
	}
}

void relax3_gs27_many(const Op3 &A, const real_t *qf, real_t *q, int II, int JJ, int KK, int updown, hipStream_t st, Batch bt)
{
	relax3_gs27_many_t(A, qf, q, II, JJ, KK, updown, st, bt);
}

// one row class (jb,kb) of that sweep on its own, rows of at most 512 pairs: the periodic batch refreshes ghosts between
// the classes (periodic_many3d.hip); perx: the row task does the x refresh (an even number of points per row)
void relax3_class27_many(const Op3 &A, const real_t *qf, real_t *q, int II, int JJ, int KK, int jb, int kb, bool efirst,
                         hipStream_t st, Batch bt, bool perx)
{
	with_row_bs((II - 2 + 1) / 2, [&](auto BS) {
		if (perx) launch_rows_many<BS(), true>(efirst, A, qf, q, II, JJ, KK, jb, kb, st, bt);
		else launch_rows_many<BS()>(efirst, A, qf, q, II, JJ, KK, jb, kb, st, bt);
	});
}

void relax3_gs27_many(const Op3f &A, const real_t *qf, real_t *q, int II, int JJ, int KK, int updown, hipStream_t st, Batch bt)
{
	relax3_gs27_many_t(A, qf, q, II, JJ, KK, updown, st, bt);
}

// ------------------------------------------------------------------ 27-point residual
// residual27_rows of relax3d.hip with the item loop inside: coefficients and diagonal of the pair once
template <int BS, typename OP = Op3>
__global__ __launch_bounds__(BS) void residual27_rows_many(const OP A, const real_t *__restrict__ qf, const real_t *__restrict__ q,
                                                            real_t *__restrict__ res, int II, int JJ, int KK, unsigned nblk,
                                                            TileShape ts, int nitems, size_t stride)
{
	const unsigned L = xcd_remap(blockIdx.x, nblk);
	unsigned jr, kr;
	if (L >= nblk || !tile_rows(L, (unsigned)(JJ - 2), (unsigned)(KK - 2), ts, jr, kr)) return;
	const size_t j = (size_t)jr + 1, k = (size_t)kr + 1;
	const size_t sj = (size_t)II, sk = (size_t)II * JJ;
	const size_t row = j * sj + k * sk, rowA = j * A.SJ + k * A.SK;
	for (int p = threadIdx.x; 2 * p + 1 <= II - 2; p += BS) {
		const int ie = 2 * p + 1, io = 2 * p + 2;
		const bool o_ok = io <= II - 2, two = io + 1 <= II - 1;
		C27 ce, co;
		real_t de, dn;
		load_coef27<false, false, false>(A, rowA, ie, io, two, ce, co);
		ldpair(A.so + rowA + ie, true, de, dn); // KP plane
#pragma unroll 1
		for (int m = 0; m < nitems; m++) {
			const size_t off = (size_t)m * stride;
			real_t qe[3][3][3], qo[3][3][3], qfe, qfo;
			load_vec27<0>(qf + off, q + off, row, sj, sk, ie, io, two, qe, qo, qfe, qfo);
			const real_t re = offdiag27(qfe, ce, qe) - de * qe[1][1][1];
			if (o_ok) {
				const real_t ro = offdiag27(qfo, co, qo) - dn * qo[1][1][1];
				d2u v; v.x = re; v.y = ro;
				*reinterpret_cast<d2u *>(res + off + row + ie) = v;
			} else
				res[off + row + ie] = re;
		}
	}
}

template <typename OP = Op3>
static void residual27_many_t(const OP &A, const real_t *qf, const real_t *q, real_t *res, int II, int JJ, int KK, hipStream_t st, Batch bt)
{
	if (II < 3 || JJ < 3 || KK < 3 || bt.n < 1) return;
	const TileShape ts = tile_shape_resid();
	const unsigned nrows = tile_blocks((unsigned)(JJ - 2), (unsigned)(KK - 2), ts);
	const int npairs = (II - 2 + 1) / 2;
	if (npairs <= 64) hipLaunchKernelGGL((residual27_rows_many<64, OP>), dim3(xcd_grid(nrows)), dim3(64), 0, st, A, qf, q, res, II, JJ, KK, nrows, ts, bt.n, bt.stride);
	else if (npairs <= 128) hipLaunchKernelGGL((residual27_rows_many<128, OP>), dim3(xcd_grid(nrows)), dim3(128), 0, st, A, qf, q, res, II, JJ, KK, nrows, ts, bt.n, bt.stride);
	else hipLaunchKernelGGL((residual27_rows_many<256, OP>), dim3(xcd_grid(nrows)), dim3(256), 0, st, A, qf, q, res, II, JJ, KK, nrows, ts, bt.n, bt.stride);
}

void residual27_many(const Op3 &A, const real_t *qf, const real_t *q, real_t *res, int II, int JJ, int KK, hipStream_t st, Batch bt)
{
	residual27_many_t(A, qf, q, res, II, JJ, KK, st, bt);
}

void residual27_many(const Op3f &A, const real_t *qf, const real_t *q, real_t *res, int II, int JJ, int KK, hipStream_t st, Batch bt)
{
	residual27_many_t(A, qf, q, res, II, JJ, KK, st, bt);
}

// ------------------------------------------------------------------ 7-point sweep and residual
// relax7_colour (relax3d.hip) / residual3_kernel (residual.hip): the six coefficients and 1/diag (the diagonal) of a
// point once, the items inside
__global__ void relax7_colour_many(const real_t *__restrict__ so, const real_t *__restrict__ qf, real_t *__restrict__ q,
                                   const real_t *__restrict__ sor, int II, int JJ, int KK, int pts, int nitems, size_t stride)
{
	const int nxh = (II - 2 + 1) / 2; // max points of one colour in a row
	const size_t n = (size_t)nxh * (JJ - 2) * (KK - 2);
	const size_t sj = II, sk = (size_t)II * JJ, PS = sk * KK;
	for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < n; t += (size_t)gridDim.x * blockDim.x) {
		const int a = (int)(t % nxh);
		const size_t r = t / nxh;
		const int j1 = 2 + (int)(r % (JJ - 2)), k1 = 2 + (int)(r / (JJ - 2)); // 1-based
		const int i1 = (j1 + k1 + pts) % 2 + 2 + 2 * a;
		if (i1 > II - 1) continue;
		const size_t x = (size_t)(i1 - 1) + sj * (size_t)(j1 - 1) + sk * (size_t)(k1 - 1);
		const real_t cw = so[KPW * PS + x], cn = so[KPS * PS + x + sj], ce = so[KPW * PS + x + 1], cs = so[KPS * PS + x];
		const real_t cb = so[KB * PS + x], ct = so[KB * PS + x + sk], rd = sor[PS + x];
		for (int m = 0; m < nitems; m++) {
			real_t *qm = q + (size_t)m * stride;
			real_t s = qf[(size_t)m * stride + x];
			s = s + cw * qm[x - 1];
			s = s + cn * qm[x + sj];
			s = s + ce * qm[x + 1];
			s = s + cs * qm[x - sj];
			s = s + cb * qm[x - sk];
			s = s + ct * qm[x + sk];
			qm[x] = s * rd;
		}
	}
}

static inline unsigned cap_grid(size_t n, unsigned bs)
{
	size_t g = (n + bs - 1) / bs;
	if (g > 16384) g = 16384;
	if (g < 1) g = 1;
	return (unsigned)g;
}

void relax3_gs7_many(const real_t *so, const real_t *qf, real_t *q, const real_t *sor, int II, int JJ, int KK, int updown,
                     hipStream_t st, Batch bt)
{
	if (II < 3 || JJ < 3 || KK < 3 || bt.n < 1) return;
	// UP = colours 0,1; DOWN = 1,0
	for (int c = 0; c < 2; c++) {
		const int pts = (updown == BMG_UP) ? c : 1 - c;
		const size_t n = (size_t)((II - 2 + 1) / 2) * (JJ - 2) * (KK - 2);
		hipLaunchKernelGGL(relax7_colour_many, dim3(cap_grid(n, 256)), dim3(256), 0, st, so, qf, q, sor, II, JJ, KK, pts, bt.n, bt.stride);
	}
}

// one colour of that sweep on its own (periodic_many3d.hip refreshes ghosts between the colours)
void relax3_colour7_many(const real_t *so, const real_t *qf, real_t *q, const real_t *sor, int II, int JJ, int KK, int pts,
                         hipStream_t st, Batch bt)
{
	const size_t n = (size_t)((II - 2 + 1) / 2) * (JJ - 2) * (KK - 2);
	hipLaunchKernelGGL(relax7_colour_many, dim3(cap_grid(n, 256)), dim3(256), 0, st, so, qf, q, sor, II, JJ, KK, pts, bt.n, bt.stride);
}

__global__ __launch_bounds__(256) void residual7_many_kernel(const real_t *__restrict__ so, const real_t *__restrict__ qf,
                                                              const real_t *__restrict__ q, real_t *__restrict__ res,
                                                              int II, int JJ, int KK, unsigned nrows, int nitems, size_t stride)
{
	const unsigned L = xcd_remap(blockIdx.x, nrows);
	if (L >= nrows) return;
	const int j = (int)(L % (unsigned)(JJ - 2)) + 1, k = (int)(L / (unsigned)(JJ - 2)) + 1;
	const size_t sj = II, sk = (size_t)II * JJ, PS = sk * KK;
	for (int i = threadIdx.x + 1; i <= II - 2; i += blockDim.x) {
		const size_t x = (size_t)i + sj * (size_t)j + sk * (size_t)k;
		const real_t cw = so[KPW * PS + x], cn = so[KPS * PS + x + sj], ce = so[KPW * PS + x + 1], cs = so[KPS * PS + x];
		const real_t cb = so[KB * PS + x], ct = so[KB * PS + x + sk], cp = so[KP * PS + x];
		for (int m = 0; m < nitems; m++) {
			const real_t *qm = q + (size_t)m * stride;
			real_t s = qf[(size_t)m * stride + x];
			s = s + cw * qm[x - 1];
			s = s + cn * qm[x + sj];
			s = s + ce * qm[x + 1];
			s = s + cs * qm[x - sj];
			s = s + cb * qm[x - sk];
			s = s + ct * qm[x + sk];
			s = s - cp * qm[x];
			res[(size_t)m * stride + x] = s;
		}
	}
}

void residual7_many(const real_t *so, const real_t *qf, const real_t *q, real_t *res, int II, int JJ, int KK, hipStream_t st, Batch bt)
{
	if (II < 3 || JJ < 3 || KK < 3 || bt.n < 1) return;
	const unsigned nrows = (unsigned)(JJ - 2) * (unsigned)(KK - 2);
	const int bs = II - 2 >= 256 ? 256 : (II - 2 > 64 ? 128 : 64);
	hipLaunchKernelGGL(residual7_many_kernel, dim3(xcd_grid(nrows)), dim3(bs), 0, st, so, qf, q, res, II, JJ, KK, nrows, bt.n, bt.stride);
}

// ------------------------------------------------------------------ restriction, interpolation and add
// restrict3_kernel / interp_add3_kernel with the CI entries of a lane's point or pair (and interp_add's two diagonal
// entries) in registers across the item loop: the device bodies of transfer_dev.h on the Cedar layout (transferf.hip: on the
// single-precision copy)
void restrict3_many(const real_t *q, real_t *qc, const real_t *ci, int II, int JJ, int KK, int IIC, int JJC, int KKC,
                    hipStream_t st, Batch bf, Batch bc)
{
	if (IIC < 3 || JJC < 3 || KKC < 3 || bf.n < 1) return;
	dim3 grid((IIC - 2 + 127) / 128, JJC - 2, KKC - 2);
	hipLaunchKernelGGL(restrict3_many_kernel<real_t>, grid, dim3(128), 0, st, q, qc, ci_cedar(ci, IIC, JJC, KKC), II, JJ, KK, IIC,
	                   JJC, KKC, bf.n, bf.stride, bc.stride);
}

void interp_add3_many(real_t *q, const real_t *qc, const real_t *so, real_t *res, const real_t *ci,
                      int IIC, int JJC, int KKC, int IIF, int JJF, int KKF, hipStream_t st, Batch bf, Batch bc)
{
	if (IIF < 3 || JJF < 3 || KKF < 3 || bf.n < 1) return;
	const InterpRanges3 r = interp_ranges3(IIC, JJC, KKC, IIF, JJF, KKF);
	hipLaunchKernelGGL(interp_add3_many_kernel<real_t>, dim3(xcd_grid(r.nrows)), dim3(r.bs), 0, st, q, qc, so /* KP plane */, res,
	                   ci_cedar(ci, IIC, JJC, KKC), IIC, JJC, KKC, IIF, JJF, KKF, r.imax_e, r.imax_all, r.jmax, r.kmax_e, r.kmax_o,
	                   r.nrows, bf.n, bf.stride, bc.stride);
}

} // namespace cedar_amd
