// The 7-point sweep and residual on a single-precision copy of the operator (common.h Op7f), for
// one vector and for a batch of right-hand sides.  The copy is row-interleaved: the five slot-rows of grid row (j,k) --
// KPW, KPS, KB, the diagonal KP and 1/diag -- lie back to back, every slot-row on a 128-byte line.  The kernels promote
// an entry to double when they load it (exact) and keep vectors and arithmetic in FP64 with the reference's term order
// (-ffp-contract=off), so every result has the bits of relax7_colour (relax3d.hip) / residual3_kernel<false>
// (residual.hip) on the operator and 1/diag rounded to float.
//
// One workgroup per grid row, rows walked in the (j,k) tiles of the 27-point row kernels so that the KPS row of j+1 and
// the KB row of k+1, which two rows of a launch read, are found in the XCD's L2; the lanes loop over the row, so a row
// may have any length.
#include "common.h"

namespace cedar_amd {

// build: one workgroup per grid row (ghost rows included), unit stride both ways, round to nearest even.  A finite entry
// that leaves float's range raises *overflow (an ordinary store of 1: every writer stores the same value).
__global__ __launch_bounds__(256) void op7f_build_kernel(const real_t *__restrict__ so, const real_t *__restrict__ sor,
                                                          float *__restrict__ out, int II, int JJ, int KK, size_t RS,
                                                          int *__restrict__ overflow)
{
	const size_t row = blockIdx.x; // j + JJ*k
	const size_t PS = (size_t)II * JJ * KK;
	float *dst = out + row * (size_t)NS7 * RS;
	bool bad = false;
	for (int s = 0; s < NS7; s++) {
		const real_t *from = s == O7_PW ? so + KPW * PS : s == O7_PS ? so + KPS * PS : s == O7_B ? so + KB * PS
		                     : s == O7_P ? so + KP * PS : sor;
		from += row * (size_t)II;
		for (size_t i = threadIdx.x; i < RS; i += 256) {
			const real_t v = i < (size_t)II ? from[i] : 0.0;
			const float f = (float)v; // v_cvt_f32_f64: round to nearest even
			bad = bad || (isinf(f) && !isinf(v));
			dst[(size_t)s * RS + i] = f;
		}
	}
	if (bad) *overflow = 1;
}

void op7f_build(const real_t *so, const real_t *sor_msor, float *out, int II, int JJ, int KK, int *overflow, hipStream_t st)
{
	hipLaunchKernelGGL(op7f_build_kernel, dim3((unsigned)((size_t)JJ * KK)), dim3(256), 0, st, so, sor_msor, out, II, JJ, KK,
	                   ilv32_row_stride(II), overflow);
}

// the six off-diagonal coefficients of point i of the grid row whose block starts at r
struct C7 {
	real_t cw, cn, ce, cs, cb, ct;
};
__device__ __forceinline__ C7 load_c7(const Op7f &A, const float *__restrict__ r, int i)
{
	C7 c;
	const f2u we = *reinterpret_cast<const f2u *>(r + O7_PW * A.RS + i); // KPW at i and i + 1
	c.cw = (real_t)we.x;
	c.ce = (real_t)we.y;
	c.cs = (real_t)r[O7_PS * A.RS + i];
	c.cn = (real_t)r[A.SJ + O7_PS * A.RS + i];
	c.cb = (real_t)r[O7_B * A.RS + i];
	c.ct = (real_t)r[A.SK + O7_B * A.RS + i];
	return c;
}
// qf + the six off-diagonal terms in the order of BMG3_SymStd_relax_GS.f90:155-184 / BMG3_SymStd_residual.f90
__device__ __forceinline__ real_t offdiag7(const C7 &c, const real_t *__restrict__ qf, const real_t *__restrict__ q, size_t x,
                                           size_t sj, size_t sk)
{
	real_t s = qf[x];
	s = s + c.cw * q[x - 1];
	s = s + c.cn * q[x + sj];
	s = s + c.ce * q[x + 1];
	s = s + c.cs * q[x - sj];
	s = s + c.cb * q[x - sk];
	s = s + c.ct * q[x + sk];
	return s;
}

// the grid row (j,k) of this workgroup; false: none (the whole workgroup leaves together)
__device__ __forceinline__ bool row_of_block(int JJ, int KK, unsigned nblk, TileShape ts, size_t &j, size_t &k)
{
	const unsigned L = xcd_remap(blockIdx.x, nblk);
	unsigned jr, kr;
	if (L >= nblk || !tile_rows(L, (unsigned)(JJ - 2), (unsigned)(KK - 2), ts, jr, kr)) return false;
	j = (size_t)jr + 1;
	k = (size_t)kr + 1;
	return true;
}

// ------------------------------------------------------------------ sweep: one colour, colour = mod(i+j+k+pts,2) 1-based
__global__ __launch_bounds__(256) void relax7f_colour(const Op7f A, const real_t *__restrict__ qf, real_t *__restrict__ q,
                                                       int II, int JJ, int KK, int pts, unsigned nblk, TileShape ts)
{
	size_t j, k;
	if (!row_of_block(JJ, KK, nblk, ts, j, k)) return;
	const size_t sj = (size_t)II, sk = (size_t)II * JJ, row = j * sj + k * sk;
	const float *__restrict__ r = A.a + j * A.SJ + k * A.SK;
	const int i0 = (int)((j + k + (size_t)pts) & 1) + 1; // 0-based first point of the colour
	for (int i = i0 + 2 * (int)threadIdx.x; i <= II - 2; i += 2 * (int)blockDim.x) {
		const C7 c = load_c7(A, r, i);
		const real_t rd = (real_t)r[O7_RD * A.RS + i];
		q[row + i] = offdiag7(c, qf, q, row + i, sj, sk) * rd;
	}
}

// the same on a batch: the coefficients and 1/diag of a point once, the items inside
__global__ __launch_bounds__(256) void relax7f_colour_many(const Op7f A, const real_t *__restrict__ qf, real_t *__restrict__ q,
                                                            int II, int JJ, int KK, int pts, unsigned nblk, TileShape ts,
                                                            int nitems, size_t stride)
{
	size_t j, k;
	if (!row_of_block(JJ, KK, nblk, ts, j, k)) return;
	const size_t sj = (size_t)II, sk = (size_t)II * JJ, row = j * sj + k * sk;
	const float *__restrict__ r = A.a + j * A.SJ + k * A.SK;
	const int i0 = (int)((j + k + (size_t)pts) & 1) + 1;
	for (int i = i0 + 2 * (int)threadIdx.x; i <= II - 2; i += 2 * (int)blockDim.x) {
		const C7 c = load_c7(A, r, i);
		const real_t rd = (real_t)r[O7_RD * A.RS + i];
		for (int m = 0; m < nitems; m++) {
			real_t *qm = q + (size_t)m * stride;
			qm[row + i] = offdiag7(c, qf + (size_t)m * stride, qm, row + i, sj, sk) * rd;
		}
	}
}

// ------------------------------------------------------------------ residual (residual3_kernel<false>'s order)
__global__ __launch_bounds__(256) void residual7f_rows(const Op7f A, const real_t *__restrict__ qf, const real_t *__restrict__ q,
                                                        real_t *__restrict__ res, int II, int JJ, int KK, unsigned nblk,
                                                        TileShape ts)
{
	size_t j, k;
	if (!row_of_block(JJ, KK, nblk, ts, j, k)) return;
	const size_t sj = (size_t)II, sk = (size_t)II * JJ, row = j * sj + k * sk;
	const float *__restrict__ r = A.a + j * A.SJ + k * A.SK;
	for (int i = (int)threadIdx.x + 1; i <= II - 2; i += (int)blockDim.x) {
		const C7 c = load_c7(A, r, i);
		const real_t cp = (real_t)r[O7_P * A.RS + i];
		real_t s = offdiag7(c, qf, q, row + i, sj, sk);
		s = s - cp * q[row + i];
		res[row + i] = s;
	}
}

__global__ __launch_bounds__(256) void residual7f_rows_many(const Op7f A, const real_t *__restrict__ qf,
                                                             const real_t *__restrict__ q, real_t *__restrict__ res, int II,
                                                             int JJ, int KK, unsigned nblk, TileShape ts, int nitems,
                                                             size_t stride)
{
	size_t j, k;
	if (!row_of_block(JJ, KK, nblk, ts, j, k)) return;
	const size_t sj = (size_t)II, sk = (size_t)II * JJ, row = j * sj + k * sk;
	const float *__restrict__ r = A.a + j * A.SJ + k * A.SK;
	for (int i = (int)threadIdx.x + 1; i <= II - 2; i += (int)blockDim.x) {
		const C7 c = load_c7(A, r, i);
		const real_t cp = (real_t)r[O7_P * A.RS + i];
		for (int m = 0; m < nitems; m++) {
			const real_t *qm = q + (size_t)m * stride;
			real_t s = offdiag7(c, qf + (size_t)m * stride, qm, row + i, sj, sk);
			s = s - cp * qm[row + i];
			res[(size_t)m * stride + row + i] = s;
		}
	}
}

// ------------------------------------------------------------------ launchers
// workgroup size for a row of n lane tasks: 64 up to 64, 128 up to 128, else 256 with the lane loop
static inline int row_block(int n) { return n <= 64 ? 64 : n <= 128 ? 128 : 256; }

// 7-point: UP = colours 0,1; DOWN = 1,0 (BMG3_SymStd_relax_GS.f90:144-153); many: the batched kernel (any bt.n >= 1)
static void relax7f_launch(bool many, const Op7f &A, const real_t *qf, real_t *q, int II, int JJ, int KK, int updown,
                           hipStream_t st, Batch bt)
{
	if (II < 3 || JJ < 3 || KK < 3 || bt.n < 1) return;
	const TileShape ts = tile_shape_relax();
	const unsigned nblk = tile_blocks((unsigned)(JJ - 2), (unsigned)(KK - 2), ts);
	const int bs = row_block((II - 2 + 1) / 2);
	for (int c = 0; c < 2; c++) {
		const int pts = (updown == BMG_UP) ? c : 1 - c;
		if (!many)
			hipLaunchKernelGGL(relax7f_colour, dim3(xcd_grid(nblk)), dim3(bs), 0, st, A, qf, q, II, JJ, KK, pts, nblk, ts);
		else
			hipLaunchKernelGGL(relax7f_colour_many, dim3(xcd_grid(nblk)), dim3(bs), 0, st, A, qf, q, II, JJ, KK, pts, nblk, ts,
			                   bt.n, bt.stride);
	}
}

static void residual7f_launch(bool many, const Op7f &A, const real_t *qf, const real_t *q, real_t *res, int II, int JJ, int KK,
                              hipStream_t st, Batch bt)
{
	if (II < 3 || JJ < 3 || KK < 3 || bt.n < 1) return;
	const TileShape ts = tile_shape_resid();
	const unsigned nblk = tile_blocks((unsigned)(JJ - 2), (unsigned)(KK - 2), ts);
	const int bs = row_block(II - 2);
	if (!many)
		hipLaunchKernelGGL(residual7f_rows, dim3(xcd_grid(nblk)), dim3(bs), 0, st, A, qf, q, res, II, JJ, KK, nblk, ts);
	else
		hipLaunchKernelGGL(residual7f_rows_many, dim3(xcd_grid(nblk)), dim3(bs), 0, st, A, qf, q, res, II, JJ, KK, nblk, ts,
		                   bt.n, bt.stride);
}

void relax3_gs7_op(const Op7f &A, const real_t *qf, real_t *q, int II, int JJ, int KK, int updown, hipStream_t st)
{
	relax7f_launch(false, A, qf, q, II, JJ, KK, updown, st, Batch());
}

void relax3_gs7_many(const Op7f &A, const real_t *qf, real_t *q, int II, int JJ, int KK, int updown, hipStream_t st, Batch bt)
{
	relax7f_launch(true, A, qf, q, II, JJ, KK, updown, st, bt);
}

void residual7_op(const Op7f &A, const real_t *qf, const real_t *q, real_t *res, int II, int JJ, int KK, hipStream_t st)
{
	residual7f_launch(false, A, qf, q, res, II, JJ, KK, st, Batch());
}

void residual7_many(const Op7f &A, const real_t *qf, const real_t *q, real_t *res, int II, int JJ, int KK, hipStream_t st, Batch bt)
{
	residual7f_launch(true, A, qf, q, res, II, JJ, KK, st, bt);
}

} // namespace cedar_amd
