// The 2D point sweeps and residuals on a single-precision copy of the operator (common.h Op2f),
// for one vector and, through the launch grid, for a batch of right-hand sides.  The copy is row-interleaved: the slot-rows
// of grid row j -- KW, KS, [KSW, KNW,] KO, 1/diag -- lie back to back, every slot-row on a 128-byte line.  The device bodies
// are those of the FP64 kernels (relax2_dev.h), instantiated on this view: an entry is promoted to double when it is
// loaded (exact), vectors and arithmetic stay FP64 in the reference's term order (-ffp-contract=off), so every result has
// the bits of the kernel of relax2d.hip / residual.hip on the operator and 1/diag rounded to float -- the partial-sum
// sweep included, at the same run length.
#include "common.h"
#include "relax2_dev.h"

namespace cedar_amd {

// build: one workgroup per grid row (ghost rows included), unit stride both ways, round to nearest even; the lead and
// the tail of every slot-row are zero.  A finite entry that leaves float's range raises *overflow (an ordinary store of
// 1: every writer stores the same value).
__global__ __launch_bounds__(256) void op2f_build_kernel(const real_t *__restrict__ so, const real_t *__restrict__ sor,
                                                          float *__restrict__ out, int II, int JJ, int ns, size_t RS,
                                                          int *__restrict__ overflow)
{
	const size_t j = blockIdx.x;
	const size_t PS = (size_t)II * JJ;
	float *dst = out + j * (size_t)ns * RS;
	bool bad = false;
	for (int s = 0; s < ns; s++) {
		// nine-point: KW, KS, KSW, KNW, KO, 1/diag; five-point: KW, KS, KO, 1/diag
		// (sor == nullptr: a line-relaxed level has no 1/diag plane, its slot-row is zeros)
		const real_t *from = s == ns - 1 ? sor : s == ns - 2 ? so + KO * PS : so + (size_t)(s + 1) * PS;
		if (from) from += j * (size_t)II;
		for (size_t o = threadIdx.x; o < RS; o += 256) {
			const real_t v = (from && o >= 1 && o <= (size_t)II) ? from[o - 1] : 0.0;
			const float f = (float)v; // v_cvt_f32_f64: round to nearest even
			bad = bad || (isinf(f) && !isinf(v));
			dst[(size_t)s * RS + o] = f;
		}
	}
	if (bad) *overflow = 1;
}

void op2f_build(const real_t *so, const real_t *sor_msor, float *out, int II, int JJ, int nstncl, int *overflow, hipStream_t st)
{
	hipLaunchKernelGGL(op2f_build_kernel, dim3((unsigned)JJ), dim3(256), 0, st, so, sor_msor, out, II, JJ, op2f_slots(nstncl),
	                   op2f_row_stride(II), overflow);
}

// ------------------------------------------------------------------ nine-point kernels (the arguments of relax2d.hip's, the
// operator as a view)
template <int BS, bool EFIRST>
__global__ __launch_bounds__(BS) void relax9f_rows(const Op2f A, const real_t *__restrict__ qf, real_t *__restrict__ q, int II,
                                                    int j0, int jstep, int nrows, size_t bstride)
{
	__shared__ real_t xch[BS + 2];
	__shared__ real_t carry_s;
	const unsigned L = xcd_remap(blockIdx.x, (unsigned)nrows);
	if (L >= (unsigned)nrows) return;
	qf += bstride * blockIdx.y; q += bstride * blockIdx.y; // batch item (common.h Batch)
	relax9_row_task<BS, EFIRST>(A, qf, q, II, (size_t)(j0 + jstep * (int)L), xch, &carry_s);
}

template <int BS, bool EFIRST>
__global__ __launch_bounds__(BS) void relax9f_band(const Op2f A, const real_t *__restrict__ qf, real_t *__restrict__ q, int II,
                                                    int JJ, int jbF, int frun, int nrun, size_t bstride)
{
	__shared__ real_t xch[BS + 2];
	__shared__ real_t carry_s;
	const unsigned run = xcd_remap(blockIdx.x, (unsigned)nrun);
	if (run >= (unsigned)nrun) return;
	qf += bstride * blockIdx.y; q += bstride * blockIdx.y;
	relax9_band_body<BS, EFIRST>(A, qf, q, II, JJ, jbF, frun, (int)run, xch, &carry_s);
}

template <int BS, bool EFIRST>
__global__ __launch_bounds__(BS) void relax9f_band_psum(const Op2f A, const real_t *__restrict__ qf, real_t *__restrict__ q,
                                                         int II, int JJ, int jbF, int frun, int nrun, size_t bstride)
{
	extern __shared__ real_t lds_band_f[];
	const int IIp = (II + 1) & ~1;
	real_t *T0 = lds_band_f, *T1 = lds_band_f + IIp, *xch = lds_band_f + 2 * IIp, *carry_s = xch + BS + 2;
	const unsigned run = xcd_remap(blockIdx.x, (unsigned)nrun);
	if (run >= (unsigned)nrun) return;
	qf += bstride * blockIdx.y; q += bstride * blockIdx.y;
	relax9_band_psum_body<BS, EFIRST>(A, qf, q, II, JJ, jbF, frun, (int)run, T0, T1, xch, carry_s);
}

__global__ __launch_bounds__(256) void residual9f_rows(const Op2f A, const real_t *__restrict__ qf, const real_t *__restrict__ q,
                                                        real_t *__restrict__ res, int II, unsigned nrows, size_t bstride)
{
	const unsigned L = xcd_remap(blockIdx.x, nrows);
	if (L >= nrows) return;
	qf += bstride * blockIdx.y; q += bstride * blockIdx.y; res += bstride * blockIdx.y;
	residual9_row_body(A, qf, q, res, II, (size_t)(L + 1));
}

// ------------------------------------------------------------------ five-point kernels (relax5_colour / residual2_kernel<false>)
__global__ __launch_bounds__(256) void relax5f_colour(const Op2f A, const real_t *__restrict__ qf, real_t *__restrict__ q, int II,
                                                       int jo, size_t bstride)
{
	qf += bstride * blockIdx.z; q += bstride * blockIdx.z;
	const int j1 = blockIdx.y + 2; // 1-based
	const int a = blockIdx.x * blockDim.x + threadIdx.x;
	const int i1 = (j1 + jo) % 2 + 2 + 2 * a;
	if (i1 > II - 1) return;
	const size_t sj = II, j = (size_t)(j1 - 1);
	const size_t x = (size_t)(i1 - 1) + sj * j;
	q[x] = offdiag5(A, qf, q, i1 - 1, j, x, sj) * (real_t)A.rd(j)[i1 - 1];
}

__global__ __launch_bounds__(256) void residual5f_kernel(const Op2f A, const real_t *__restrict__ qf, const real_t *__restrict__ q,
                                                          real_t *__restrict__ res, int II, size_t bstride)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x + 1; // 0-based incl. ghost
	const size_t j = (size_t)blockIdx.y + 1;
	if (i > II - 2) return;
	qf += bstride * blockIdx.z; q += bstride * blockIdx.z; res += bstride * blockIdx.z;
	const size_t sj = II, x = (size_t)i + sj * j;
	real_t s = offdiag5(A, qf, q, i, j, x, sj);
	s = s - (real_t)A.row(KO, j)[i] * q[x];
	res[x] = s;
}

// ------------------------------------------------------------------ launchers: the geometry of relax2d.hip's, step for step
template <int BS>
static void launch_rows9f(bool efirst, const Op2f &A, const real_t *qf, real_t *q, int II, int j0, int jstep, int nrows,
                          hipStream_t st, Batch bt)
{
	if (nrows <= 0) return;
	const dim3 grid(xcd_grid((unsigned)nrows), bt.n);
	if (efirst) hipLaunchKernelGGL((relax9f_rows<BS, true>), grid, dim3(BS), 0, st, A, qf, q, II, j0, jstep, nrows, bt.stride);
	else hipLaunchKernelGGL((relax9f_rows<BS, false>), grid, dim3(BS), 0, st, A, qf, q, II, j0, jstep, nrows, bt.stride);
}

// whole nine-point sweep in the reference order: band-fused where band_frun says so, else one launch per row class
static void sweep9f(const Op2f &A, const real_t *qf, real_t *q, int II, int JJ, bool down, hipStream_t st, Batch bt)
{
	const int frun = band_frun(II, JJ);
	if (frun == 0 || (II - 2 + 1) / 2 <= 64) {
		for (int c = 0; c < 2; c++) { // DOWN: rows J=2,4,.. first (LSTART=2), even 1-based i first
			const int jb = down ? c : 1 - c, nrows = (JJ - 2 - jb + 1) / 2;
			if ((II - 2 + 1) / 2 <= 64) launch_rows9f<64>(down, A, qf, q, II, 1 + jb, 2, nrows, st, bt);
			else launch_rows9f<256>(down, A, qf, q, II, 1 + jb, 2, nrows, st, bt);
		}
		return;
	}
	const int jbF = down ? 0 : 1;
	const int nF = (JJ - 2 - jbF + 1) / 2, nrun = (nF + frun - 1) / frun;
	const dim3 grid(xcd_grid((unsigned)nrun), bt.n);
	if (down) hipLaunchKernelGGL((relax9f_band<256, true>), grid, dim3(256), 0, st, A, qf, q, II, JJ, jbF, frun, nrun, bt.stride);
	else hipLaunchKernelGGL((relax9f_band<256, false>), grid, dim3(256), 0, st, A, qf, q, II, JJ, jbF, frun, nrun, bt.stride);
	// S rows between runs: jbF = 0: j = 2 frun (r+1); jbF = 1: j = 1 + 2 frun (r+1), r = 0 .. nrun-2
	launch_rows9f<256>(down, A, qf, q, II, (jbF ? 1 : 0) + 2 * frun, 2 * frun, nrun - 1, st, bt);
}

void relax2_gs9_psum_op(const Op2f &A, const real_t *qf, real_t *q, int II, int JJ, int updown, hipStream_t st, Batch bt)
{
	if (II < 3 || JJ < 3) return;
	const bool down = updown == BMG_DOWN;
	const int frun = band_psum_frun(II, JJ);
	if (frun == 0) {
		sweep9f(A, qf, q, II, JJ, down, st, bt);
		return;
	}
	const int jbF = down ? 0 : 1;
	const int nF = (JJ - 2 - jbF + 1) / 2, nrun = (nF + frun - 1) / frun;
	const size_t shm = ((size_t)((II + 1) & ~1) * 2 + 256 + 2 + 2) * sizeof(real_t);
	static bool attr_dev[64] = {false};
	int dev_ = 0;
	(void)hipGetDevice(&dev_);
	if (!attr_dev[dev_ & 63]) {
		CEDAR_HIP_CHECK(hipFuncSetAttribute((const void *)relax9f_band_psum<256, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 72 * 1024));
		CEDAR_HIP_CHECK(hipFuncSetAttribute((const void *)relax9f_band_psum<256, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 72 * 1024));
		attr_dev[dev_ & 63] = true;
	}
	const dim3 grid(xcd_grid((unsigned)nrun), bt.n);
	if (down) hipLaunchKernelGGL((relax9f_band_psum<256, true>), grid, dim3(256), shm, st, A, qf, q, II, JJ, jbF, frun, nrun, bt.stride);
	else hipLaunchKernelGGL((relax9f_band_psum<256, false>), grid, dim3(256), shm, st, A, qf, q, II, JJ, jbF, frun, nrun, bt.stride);
	launch_rows9f<256>(down, A, qf, q, II, (jbF ? 1 : 0) + 2 * frun, 2 * frun, nrun - 1, st, bt);
}

void relax2_gs_op(const Op2f &A, const real_t *qf, real_t *q, int II, int JJ, int nstncl, int updown, hipStream_t st, Batch bt)
{
	if (II < 3 || JJ < 3) return;
	const bool down = (updown == BMG_DOWN);
	if (nstncl == 5) {
		sweep9f(A, qf, q, II, JJ, down, st, bt);
		return;
	}
	const dim3 grid(((II - 2 + 1) / 2 + 255) / 256, JJ - 2, bt.n);
	for (int c = 0; c < 2; c++) // colour = mod(i+j+jo,2) (1-based), jo = LSTART..LEND
		hipLaunchKernelGGL(relax5f_colour, grid, dim3(256), 0, st, A, qf, q, II, down ? 2 + c : 3 - c, bt.stride);
}

void residual2_op(const Op2f &A, const real_t *qf, const real_t *q, real_t *res, int II, int JJ, int nstncl, hipStream_t st, Batch bt)
{
	if (II < 3 || JJ < 3) return;
	if (nstncl == 5) {
		const unsigned nrows = (unsigned)(JJ - 2);
		hipLaunchKernelGGL(residual9f_rows, dim3(xcd_grid(nrows), bt.n), dim3((II - 2) / 2 >= 256 ? 256 : 64), 0, st, A, qf, q, res,
		                   II, nrows, bt.stride);
		return;
	}
	const dim3 grid((II - 2 + 255) / 256, JJ - 2, bt.n);
	hipLaunchKernelGGL(residual5f_kernel, grid, dim3(256), 0, st, A, qf, q, res, II, bt.stride);
}

} // namespace cedar_amd
