// The inter-grid transfers on a single-precision copy of the interpolation weights (common.h Ci3f / Ci2f; DESIGN.md section
// 18; cedar_amd_solver_use_fp32_interpolation).  The copy keeps the slots in planes, every coarse row padded to a multiple
// of 32 floats with one float of lead, so every row of every slot starts on a 128-byte line and the pair (ic, ic + 1) of an
// odd ic sits on an 8-byte boundary.  The device bodies are those of the FP64 kernels (transfer_dev.h) instantiated on this
// view: a weight is promoted to double when it is used (exact), vectors, the diagonal and all arithmetic stay FP64 in the
// reference's term order (-ffp-contract=off), so every result has the bits of the kernel of transfer.hip / many3d.hip on
// the weights rounded to float.
//   restrictions: a lane owns two adjacent coarse points and moves their weights as aligned pairs (8-byte loads instead of
//   4-byte ones); one kernel serves one vector and a batch (the weights stay in registers across the items).
//   interp_add: lane ownership of the FP64 kernels (3D: a lane's fine pair reads different slots at its two coarse
//   columns, so its weights stay single loads).
#include "common.h"
#include "transfer_dev.h"

namespace cedar_amd {

// build: one workgroup per (slot, coarse row), unit stride both ways, round to nearest even; the lead and the tail of every
// row are zero.  A finite weight that leaves float's range raises *overflow (an ordinary store of 1: every writer stores
// the same value).
__global__ __launch_bounds__(256) void ci32_build_kernel(const real_t *__restrict__ ci, float *__restrict__ out, int IIC, size_t RS,
                                                          int *__restrict__ overflow)
{
	const size_t row = blockIdx.x; // slot-major, then kc, jc: the order of both arrays
	const real_t *from = ci + row * (size_t)IIC;
	float *dst = out + row * RS;
	bool bad = false;
	for (size_t o = threadIdx.x; o < RS; o += 256) {
		const real_t v = (o >= 1 && o <= (size_t)IIC) ? from[o - 1] : 0.0;
		const float f = (float)v; // v_cvt_f32_f64: round to nearest even
		bad = bad || (isinf(f) && !isinf(v));
		dst[o] = f;
	}
	if (bad) *overflow = 1;
}

void ci32_build(const real_t *ci, float *out, int IIC, int JJC, int KKC, int nslots, int *overflow, hipStream_t st)
{
	const size_t rows = (size_t)JJC * KKC * nslots;
	hipLaunchKernelGGL(ci32_build_kernel, dim3((unsigned)rows), dim3(256), 0, st, ci, out, IIC, ci32_row_stride(IIC), overflow);
}

// lanes of a restriction workgroup for a coarse row of npairs pairs
static inline int pairs_block(int npairs, int most) { return npairs <= 64 ? 64 : npairs <= 128 || most == 128 ? 128 : 256; }

void restrict2_ci(const Ci2f &W, const real_t *q, real_t *qc, int II, int JJ, int IIC, int JJC, hipStream_t st, Batch bf, Batch bc)
{
	if (IIC < 3 || JJC < 3) return;
	const int npairs = (IIC - 2 + 1) / 2, bs = pairs_block(npairs, 256);
	dim3 grid((npairs + bs - 1) / bs, JJC - 2, bf.n);
	hipLaunchKernelGGL(restrict2_pairs_kernel<float>, grid, dim3(bs), 0, st, q, qc, W, II, JJ, IIC, JJC, bf.stride, bc.stride);
}

void interp_add2_ci(const Ci2f &W, real_t *q, const real_t *qc, real_t *res, const real_t *so, int IIC, int JJC, int IIF, int JJF,
                    hipStream_t st, Batch bf, Batch bc)
{
	if (IIF < 3 || JJF < 3) return;
	const int imax = 2 * ((IIF - 2) / 2 + 2 - 1), jmax = 2 * ((JJF - 2) / 2 + 2 - 1);
	dim3 grid((IIF - 1 + 255) / 256, JJF - 1, bf.n);
	hipLaunchKernelGGL(interp_add2_kernel<float>, grid, dim3(256), 0, st, q, qc, res, so /* KO plane */, W, IIC, JJC, IIF, JJF, imax,
	                   jmax, bf.stride, bc.stride);
}

void restrict3_ci(const Ci3f &W, const real_t *q, real_t *qc, int II, int JJ, int KK, int IIC, int JJC, int KKC, hipStream_t st,
                  Batch bf, Batch bc)
{
	if (IIC < 3 || JJC < 3 || KKC < 3 || bf.n < 1) return;
	const int npairs = (IIC - 2 + 1) / 2, bs = pairs_block(npairs, 128);
	dim3 grid((npairs + bs - 1) / bs, JJC - 2, KKC - 2);
	hipLaunchKernelGGL(restrict3_pairs_kernel<float>, grid, dim3(bs), 0, st, q, qc, W, II, JJ, KK, IIC, JJC, KKC, bf.n, bf.stride,
	                   bc.stride);
}

void interp_add3_ci(const Ci3f &W, real_t *q, const real_t *qc, const real_t *so, real_t *res, int IIC, int JJC, int KKC,
                    int IIF, int JJF, int KKF, hipStream_t st, Batch bf, Batch bc)
{
	if (IIF < 3 || JJF < 3 || KKF < 3 || bf.n < 1) return;
	const InterpRanges3 r = interp_ranges3(IIC, JJC, KKC, IIF, JJF, KKF);
	if (bf.n == 1)
		hipLaunchKernelGGL(interp_add3_kernel<float>, dim3(xcd_grid(r.nrows)), dim3(r.bs), 0, st, q, qc, so /* KP plane */, res, W,
		                   IIC, JJC, KKC, IIF, JJF, KKF, r.imax_e, r.imax_all, r.jmax, r.kmax_e, r.kmax_o, r.nrows);
	else
		hipLaunchKernelGGL(interp_add3_many_kernel<float>, dim3(xcd_grid(r.nrows)), dim3(r.bs), 0, st, q, qc, so /* KP plane */, res,
		                   W, IIC, JJC, KKC, IIF, JJF, KKF, r.imax_e, r.imax_all, r.jmax, r.kmax_e, r.kmax_o, r.nrows, bf.n,
		                   bf.stride, bc.stride);
}

} // namespace cedar_amd
