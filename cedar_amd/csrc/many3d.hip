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
#include <type_traits>

namespace cedar_amd {

// ------------------------------------------------------------------ 27-point sweep
// relax27_row_task for a batch: lane p relaxes the pair (2p+1, 2p+2) of row (j,k) of every item, both i-colours.  The
// coefficients and reciprocals stay in registers across the item loop, the q windows are per item.  xch: two LDS rows
// of BS+2 doubles used in turn, so that an item's first-colour values are not overwritten while a slower wave still
// reads the previous item's (one __syncthreads per item; every wave of the workgroup must call this).
// OP: the operator view, Op3 or the single-precision Op3f (common.h; entries promoted to double by the pair loads, so
// the items see the FP64 sweep of the operator rounded to float).
template <int BS, bool EFIRST, bool NT, typename OP = Op3>
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
				o_new = offdiag27(qfo, co, qo) * sro;
			}
		} else {
			if (o_ok) {
				o_new = offdiag27(qfo, co, qo) * sro;
				x[p + 1] = o_new;
			}
			__syncthreads();
			if (e_ok) {
				if (p > 0) qe[1][1][0] = x[p]; // previous pair's fresh o (p == 0: ghost column)
				if (o_ok) qe[1][1][2] = o_new;
				e_new = offdiag27(qfe, ce, qe) * sre;
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
template <int BS, bool EFIRST, bool NT, typename OP = Op3>
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
	relax27_row_task_many<BS, EFIRST, NT>(A, qf, q, II, (size_t)II, (size_t)II * JJ, j, k, xch, nitems, stride);
}

template <int BS, typename OP = Op3>
static void launch_rows_many(bool efirst, const OP &A, const real_t *qf, real_t *q, int II, int JJ, int KK, int jb, int kb,
                             hipStream_t st, Batch bt)
{
	const int nrj = (JJ - 2 - jb + 1) / 2, nrk = (KK - 2 - kb + 1) / 2;
	if (nrj <= 0 || nrk <= 0) return;
	const TileShape ts = tile_shape_relax();
	const unsigned grid = xcd_grid(tile_blocks((unsigned)nrj, (unsigned)nrk, ts));
	// operator rows are read by exactly one task of a launch: streamed past the caches as in the single-vector sweep
	if (efirst) hipLaunchKernelGGL((relax27_rows_many<BS, true, true, OP>), dim3(grid), dim3(BS), 0, st, A, qf, q, II, JJ, KK, jb, kb, nrj, nrk, ts, bt.n, bt.stride);
	else hipLaunchKernelGGL((relax27_rows_many<BS, false, true, OP>), dim3(grid), dim3(BS), 0, st, A, qf, q, II, JJ, KK, jb, kb, nrj, nrk, ts, bt.n, bt.stride);
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
		if (npairs <= 64) launch_rows_many<64>(up, A, qf, q, II, JJ, KK, jb, kb, st, bt);
		else if (npairs <= 128) launch_rows_many<128>(up, A, qf, q, II, JJ, KK, jb, kb, st, bt);
		else if (npairs <= 256) launch_rows_many<256>(up, A, qf, q, II, JJ, KK, jb, kb, st, bt);
		else launch_rows_many<512>(up, A, qf, q, II, JJ, KK, jb, kb, st, bt);
	}
}

void relax3_gs27_many(const Op3 &A, const real_t *qf, real_t *q, int II, int JJ, int KK, int updown, hipStream_t st, Batch bt)
{
	relax3_gs27_many_t(A, qf, q, II, JJ, KK, updown, st, bt);
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

// ------------------------------------------------------------------ restriction
// restrict3_kernel (transfer.hip): the 26 CI entries of a coarse point once, the items inside
__global__ __launch_bounds__(128) void restrict3_many_kernel(const real_t *__restrict__ q, real_t *__restrict__ qc,
                                                              const real_t *__restrict__ ci, int II, int JJ, int KK,
                                                              int IIC, int JJC, int KKC, int nitems, size_t bsf, size_t bsc)
{
	const int ic = blockIdx.x * blockDim.x + threadIdx.x + 1;
	const int jc = blockIdx.y + 1, kc = blockIdx.z + 1;
	if (ic > IIC - 2) return;
	const size_t sc = IIC, tc = (size_t)IIC * JJC, PC = tc * KKC;
	const size_t sf = II, tf = (size_t)II * JJ;
	const size_t c = (size_t)ic + sc * jc + tc * kc;
	const size_t f = (size_t)(2 * ic - 1) + sf * (size_t)(2 * jc - 1) + tf * (size_t)(2 * kc - 1);
#define CIv(slot, off) ci[(size_t)(slot)*PC + c + (off)]
	const real_t xyne = CIv(LXYNE, 0), xya = CIv(LXYA, 0), xynw = CIv(LXYNW, 1), xyr = CIv(LXYR, 0), xyl = CIv(LXYL, 1);
	const real_t xyse = CIv(LXYSE, sc), xyb = CIv(LXYB, sc), xysw = CIv(LXYSW, 1 + sc);
	const real_t tne = CIv(LTNE, 0), yznw = CIv(LYZNW, 0), tnw = CIv(LTNW, 1), xzne = CIv(LXZNE, 0), xza = CIv(LXZA, 0);
	const real_t xznw = CIv(LXZNW, 1), tse = CIv(LTSE, sc), yzne = CIv(LYZNE, sc), tsw = CIv(LTSW, 1 + sc);
	const real_t bne = CIv(LBNE, tc), yzsw = CIv(LYZSW, tc), bnw = CIv(LBNW, 1 + tc), xzse = CIv(LXZSE, tc), xzb = CIv(LXZB, tc);
	const real_t xzsw = CIv(LXZSW, 1 + tc), bse = CIv(LBSE, sc + tc), yzse = CIv(LYZSE, sc + tc), bsw = CIv(LBSW, 1 + sc + tc);
#undef CIv
	for (int m = 0; m < nitems; m++) {
		const real_t *qm = q + (size_t)m * bsf;
		real_t s = xyne * qm[f - 1 - sf];
		s = s + xya * qm[f - sf];
		s = s + xynw * qm[f + 1 - sf];
		s = s + xyr * qm[f - 1];
		s = s + qm[f];
		s = s + xyl * qm[f + 1];
		s = s + xyse * qm[f - 1 + sf];
		s = s + xyb * qm[f + sf];
		s = s + xysw * qm[f + 1 + sf];
		s = s + tne * qm[f - 1 - sf - tf];
		s = s + yznw * qm[f - sf - tf];
		s = s + tnw * qm[f + 1 - sf - tf];
		s = s + xzne * qm[f - 1 - tf];
		s = s + xza * qm[f - tf];
		s = s + xznw * qm[f + 1 - tf];
		s = s + tse * qm[f - 1 + sf - tf];
		s = s + yzne * qm[f + sf - tf];
		s = s + tsw * qm[f + 1 + sf - tf];
		s = s + bne * qm[f - 1 - sf + tf];
		s = s + yzsw * qm[f - sf + tf];
		s = s + bnw * qm[f + 1 - sf + tf];
		s = s + xzse * qm[f - 1 + tf];
		s = s + xzb * qm[f + tf];
		s = s + xzsw * qm[f + 1 + tf];
		s = s + bse * qm[f - 1 + sf + tf];
		s = s + yzse * qm[f + sf + tf];
		s = s + bsw * qm[f + 1 + sf + tf];
		qc[(size_t)m * bsc + c] = s;
	}
}

void restrict3_many(const real_t *q, real_t *qc, const real_t *ci, int II, int JJ, int KK, int IIC, int JJC, int KKC,
                    hipStream_t st, Batch bf, Batch bc)
{
	if (IIC < 3 || JJC < 3 || KKC < 3 || bf.n < 1) return;
	dim3 grid((IIC - 2 + 127) / 128, JJC - 2, KKC - 2);
	hipLaunchKernelGGL(restrict3_many_kernel, grid, dim3(128), 0, st, q, qc, ci, II, JJ, KK, IIC, JJC, KKC, bf.n, bf.stride, bc.stride);
}

// ------------------------------------------------------------------ interpolation and add
// interp_add3_kernel (transfer.hip) with the CI entries of a lane's pair (up to 4 for the even column, 8 for the odd one,
// by the (j,k) parity of the row) and the two diagonal entries in registers across the item loop.  The expressions of
// interp_add3_pair, in its order.
struct InterpCoef {
	real_t e[4], o[8];
};

template <bool KO, bool JO>
__device__ __forceinline__ void interp_coef3(InterpCoef &w, bool upd_e, bool upd_o, const real_t *__restrict__ ci, size_t ce, size_t PC)
{
	const size_t co = ce + 1;
#define CIe(slot) ci[(size_t)(slot)*PC + ce]
#define CIo(slot) ci[(size_t)(slot)*PC + co]
	if (!KO) {
		if (!JO) {
			if (upd_o) { w.o[0] = CIo(LXYR); w.o[1] = CIo(LXYL); }
		} else {
			if (upd_e) { w.e[0] = CIe(LXYA); w.e[1] = CIe(LXYB); }
			if (upd_o) { w.o[0] = CIo(LXYSW); w.o[1] = CIo(LXYNW); w.o[2] = CIo(LXYNE); w.o[3] = CIo(LXYSE); }
		}
	} else {
		if (!JO) {
			if (upd_e) { w.e[0] = CIe(LXZA); w.e[1] = CIe(LXZB); }
			if (upd_o) { w.o[0] = CIo(LXZNW); w.o[1] = CIo(LXZNE); w.o[2] = CIo(LXZSW); w.o[3] = CIo(LXZSE); }
		} else {
			if (upd_e) { w.e[0] = CIe(LYZNW); w.e[1] = CIe(LYZNE); w.e[2] = CIe(LYZSW); w.e[3] = CIe(LYZSE); }
			if (upd_o) {
				w.o[0] = CIo(LTNW); w.o[1] = CIo(LTNE); w.o[2] = CIo(LTSW); w.o[3] = CIo(LTSE);
				w.o[4] = CIo(LBNW); w.o[5] = CIo(LBNE); w.o[6] = CIo(LBSW); w.o[7] = CIo(LBSE);
			}
		}
	}
#undef CIe
#undef CIo
}

template <bool KO, bool JO>
__device__ __forceinline__ void interp_apply3(const InterpCoef &w, real_t &ve, real_t &vo, real_t re, real_t ro, bool upd_e,
                                              bool upd_o, const real_t *__restrict__ qc, size_t ce, size_t sc, size_t tc)
{
	const size_t co = ce + 1;
	if (!KO) {
		if (!JO) {
			if (upd_e) ve = ve + qc[ce];
			if (upd_o) {
				real_t a = w.o[0] * qc[co] + w.o[1] * qc[co - 1];
				vo = vo + a + ro;
			}
		} else {
			if (upd_e) {
				real_t a = w.e[0] * qc[ce] + w.e[1] * qc[ce - sc];
				ve = ve + a + re;
			}
			if (upd_o) {
				real_t a = w.o[0] * qc[co - 1 - sc] + w.o[1] * qc[co - 1] + w.o[2] * qc[co] + w.o[3] * qc[co - sc];
				vo = vo + a + ro;
			}
		}
	} else {
		if (!JO) {
			if (upd_e) ve = ve + w.e[0] * qc[ce] + w.e[1] * qc[ce - tc] + re;
			if (upd_o)
				vo = vo + w.o[0] * qc[co - 1] + w.o[1] * qc[co] + w.o[2] * qc[co - 1 - tc] + w.o[3] * qc[co - tc] + ro;
		} else {
			if (upd_e)
				ve = ve + w.e[0] * qc[ce] + w.e[1] * qc[ce - sc] + w.e[2] * qc[ce - tc] + w.e[3] * qc[ce - sc - tc] + re;
			if (upd_o)
				vo = vo + w.o[0] * qc[co - 1] + w.o[1] * qc[co] + w.o[2] * qc[co - 1 - sc] + w.o[3] * qc[co - sc]
				     + w.o[4] * qc[co - 1 - tc] + w.o[5] * qc[co - tc] + w.o[6] * qc[co - 1 - sc - tc] + w.o[7] * qc[co - sc - tc] + ro;
		}
	}
}

template <bool KO, bool JO>
__device__ __forceinline__ void interp_add3_row_many(real_t *__restrict__ q, const real_t *__restrict__ qc,
                                                     const real_t *__restrict__ so_diag, real_t *__restrict__ res,
                                                     const real_t *__restrict__ ci, int IIF, size_t rowf, size_t rowc,
                                                     size_t sc, size_t tc, size_t PC, bool row_in_range, bool row_interior,
                                                     int imax_e, int imax_all, int nitems, size_t bsf, size_t bsc)
{
	for (int p = threadIdx.x; 2 * p + 2 <= IIF; p += blockDim.x) {
		const int ie = 2 * p + 2, io = ie + 1; // 1-based
		const bool have_o = io <= IIF;
		const size_t x = rowf + (size_t)(ie - 1);
		const bool int_e = row_interior && ie <= IIF - 1, int_o = row_interior && have_o && io <= IIF - 1;
		const bool upd_e = row_in_range && (KO ? ie <= imax_e : ie <= imax_all);
		const bool upd_o = row_in_range && have_o && (KO ? io <= imax_all - 1 : io <= imax_all);
		if (!(int_e || int_o || upd_e || upd_o)) continue;
		real_t de = 1.0, dn = 1.0;
		if (have_o) {
			d2u t = *reinterpret_cast<const d2u *>(so_diag + x); de = t.x; dn = t.y;
		} else
			de = so_diag[x];
		const size_t ce = rowc + (size_t)(ie / 2); // 0-based: ic-1 = i/2
		InterpCoef w;
		interp_coef3<KO, JO>(w, upd_e, upd_o, ci, ce, PC);
		for (int m = 0; m < nitems; m++) {
			real_t *qm = q + (size_t)m * bsf, *rm = res + (size_t)m * bsf;
			real_t re = 0.0, ro = 0.0, ve = 0.0, vo = 0.0;
			if (have_o) {
				d2u t = *reinterpret_cast<const d2u *>(rm + x); re = t.x; ro = t.y;
				t = *reinterpret_cast<const d2u *>(qm + x); ve = t.x; vo = t.y;
			} else {
				re = rm[x]; ve = qm[x];
			}
			if (int_e) re = re / de;
			if (int_o) ro = ro / dn;
			if (int_e && int_o) {
				d2u t; t.x = re; t.y = ro;
				*reinterpret_cast<d2u *>(rm + x) = t;
			} else {
				if (int_e) rm[x] = re;
				if (int_o) rm[x + 1] = ro;
			}
			if (!(upd_e || upd_o)) continue;
			interp_apply3<KO, JO>(w, ve, vo, re, ro, upd_e, upd_o, qc + (size_t)m * bsc, ce, sc, tc);
			if (upd_e && upd_o) {
				d2u t; t.x = ve; t.y = vo;
				*reinterpret_cast<d2u *>(qm + x) = t;
			} else {
				if (upd_e) qm[x] = ve;
				if (upd_o) qm[x + 1] = vo;
			}
		}
	}
}

__global__ __launch_bounds__(256) void interp_add3_many_kernel(real_t *__restrict__ q, const real_t *__restrict__ qc,
                                                                const real_t *__restrict__ so_diag, real_t *__restrict__ res,
                                                                const real_t *__restrict__ ci,
                                                                int IIC, int JJC, int KKC, int IIF, int JJF, int KKF,
                                                                int imax_e, int imax_all, int jmax, int kmax_e, int kmax_o,
                                                                unsigned nrows, int nitems, size_t bsf, size_t bsc)
{
	const unsigned L = xcd_remap(blockIdx.x, nrows);
	if (L >= nrows) return;
	const int j = (int)(L % (unsigned)(JJF - 1)) + 2, k = (int)(L / (unsigned)(JJF - 1)) + 2; // 1-based, 2..JJF / 2..KKF
	const size_t sf = IIF, tf = (size_t)IIF * JJF;
	const size_t sc = IIC, tc = (size_t)IIC * JJC, PC = tc * KKC;
	const bool jo = j & 1, ko = k & 1;
	const int jc = jo ? (j + 1) / 2 + 1 : j / 2 + 1, kc = ko ? (k + 1) / 2 + 1 : k / 2 + 1;
	const bool row_in_range = j <= jmax && k <= (ko ? kmax_o : kmax_e);
	const bool row_interior = j <= JJF - 1 && k <= KKF - 1;
	const size_t rowf = sf * (size_t)(j - 1) + tf * (size_t)(k - 1);
	const size_t rowc = sc * (size_t)(jc - 1) + tc * (size_t)(kc - 1);
#define ROW(KOv, JOv)                                                                                                       \
	interp_add3_row_many<KOv, JOv>(q, qc, so_diag, res, ci, IIF, rowf, rowc, sc, tc, PC, row_in_range, row_interior, imax_e, \
	                               imax_all, nitems, bsf, bsc)
	if (ko) {
		if (jo) ROW(true, true);
		else ROW(true, false);
	} else {
		if (jo) ROW(false, true);
		else ROW(false, false);
	}
#undef ROW
}

void interp_add3_many(real_t *q, const real_t *qc, const real_t *so, real_t *res, const real_t *ci,
                      int IIC, int JJC, int KKC, int IIF, int JJF, int KKF, hipStream_t st, Batch bf, Batch bc)
{
	if (IIF < 3 || JJF < 3 || KKF < 3 || bf.n < 1) return;
	const int iicf1 = (IIF - 2) / 2 + 2, jjcf1 = (JJF - 2) / 2 + 2, kkcf1 = (KKF - 2) / 2 + 2;
	const int imax_all = 2 * (iicf1 - 1);
	const int imax_e = 2 * (IIC - 2);
	const int jmax = 2 * (jjcf1 - 1);
	const int kmax_e = 2 * (KKC - 2);
	const int kmax_o = 2 * (kkcf1 - 1) - 1;
	const unsigned nrows = (unsigned)(JJF - 1) * (unsigned)(KKF - 1);
	const int bs = IIF / 2 >= 256 ? 256 : (IIF / 2 > 64 ? 128 : 64); // one lane per column pair
	hipLaunchKernelGGL(interp_add3_many_kernel, dim3(xcd_grid(nrows)), dim3(bs), 0, st, q, qc, so /* KP plane */, res, ci,
	                   IIC, JJC, KKC, IIF, JJF, KKF, imax_e, imax_all, jmax, kmax_e, kmax_o, nrows, bf.n, bf.stride, bc.stride);
}

} // namespace cedar_amd
