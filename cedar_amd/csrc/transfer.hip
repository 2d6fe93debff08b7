// Inter-grid transfers: restriction b_c = P^T r and interpolate-and-add
// x += P x_c (+ r/diag at F points).
// Replace BMG2_SymStd_restrict (src/2d/ftn/BMG2_SymStd_restrict.f90:73-92),
// BMG3_SymStd_restrict (src/3d/ftn/BMG3_SymStd_restrict.f90:115-150),
// BMG2_SymStd_interp_add (src/2d/ftn/BMG2_SymStd_interp_add.f90:88-137) and
// BMG3_SymStd_interp_add (src/3d/ftn/BMG3_SymStd_interp_add.f90:88-240).
//
// restrict: one lane per coarse point (gather, unit stride in the coarse row).
// interp_add: the reference scatters from coarse cells; every fine point is
// written exactly once, so the device kernel is one lane per *fine* point that
// picks its formula from its (i,j,k) parity -- a pure gather, no atomics, and
// the in-place RES /= diag pass is fused in (each RES entry is only consumed by
// its own point).  The reference's index ranges are kept exactly, including
// the ghost column/row it touches for even extents (IICF1 = (IIF-2)/2+2).
// Term order = reference, no contraction => bit-identical results.
#include "common.h"
#include "transfer_dev.h"

namespace cedar_amd {

// The device bodies live in transfer_dev.h, written on a view of the weights; this unit instantiates them on the Cedar
// layout (FP64), transferf.hip on the single-precision copy.
// ------------------------------------------------------------------ restrict
void restrict2(const real_t *q, real_t *qc, const real_t *ci, int II, int JJ, int IIC, int JJC, hipStream_t st, Batch bf, Batch bc)
{
	if (IIC < 3 || JJC < 3) return;
	dim3 grid((IIC - 2 + 255) / 256, JJC - 2, bf.n);
	hipLaunchKernelGGL(restrict2_kernel<real_t>, grid, dim3(256), 0, st, q, qc, ci_cedar(ci, IIC, JJC), II, JJ, IIC, JJC,
	                   bf.stride, bc.stride);
}

void restrict3(const real_t *q, real_t *qc, const real_t *ci, int II, int JJ, int KK,
               int IIC, int JJC, int KKC, hipStream_t st)
{
	if (IIC < 3 || JJC < 3 || KKC < 3) return;
	dim3 grid((IIC - 2 + 127) / 128, JJC - 2, KKC - 2);
	hipLaunchKernelGGL(restrict3_kernel<real_t>, grid, dim3(128), 0, st, q, qc, ci_cedar(ci, IIC, JJC, KKC), II, JJ, KK, IIC, JJC,
	                   KKC);
}

// ------------------------------------------------------------------ interp_add
void interp_add2(real_t *q, const real_t *qc, real_t *res, const real_t *so, const real_t *ci,
                 int IIC, int JJC, int IIF, int JJF, hipStream_t st, Batch bf, Batch bc)
{
	if (IIF < 3 || JJF < 3) return;
	const int imax = 2 * ((IIF - 2) / 2 + 2 - 1), jmax = 2 * ((JJF - 2) / 2 + 2 - 1);
	dim3 grid((IIF - 1 + 255) / 256, JJF - 1, bf.n);
	hipLaunchKernelGGL(interp_add2_kernel<real_t>, grid, dim3(256), 0, st, q, qc, res, so /* KO plane */, ci_cedar(ci, IIC, JJC),
	                   IIC, JJC, IIF, JJF, imax, jmax, bf.stride, bc.stride);
}

void interp_add3(real_t *q, const real_t *qc, const real_t *so, real_t *res, const real_t *ci,
                 int IIC, int JJC, int KKC, int IIF, int JJF, int KKF, hipStream_t st)
{
	if (IIF < 3 || JJF < 3 || KKF < 3) return;
	const InterpRanges3 r = interp_ranges3(IIC, JJC, KKC, IIF, JJF, KKF);
	hipLaunchKernelGGL(interp_add3_kernel<real_t>, dim3(xcd_grid(r.nrows)), dim3(r.bs), 0, st, q, qc, so /* KP plane */, res,
	                   ci_cedar(ci, IIC, JJC, KKC), IIC, JJC, KKC, IIF, JJF, KKF, r.imax_e, r.imax_all, r.jmax, r.kmax_e, r.kmax_o,
	                   r.nrows);
}

// ------------------------------------------------------------------ halo pack / unpack
// Copies up to 26 sub-boxes of a (planes x KK x JJ x II) array to / from one contiguous buffer in a
// single launch (blockIdx.y = box): the pack and unpack steps of the ghost-layer exchange that
// replaces the MSG gather/scatter index lists of the reference (src/2d/ftn/mpi/mpi_msg.F:483-550).
struct BoxTable {
	int n;
	int i0[26], j0[26], k0[26], ni[26], nj[26], nk[26];
	int sj[26], sk[26]; // step between the rows / planes of a box (1: dense; 2: one row class / one k-parity)
	unsigned long long off[26]; // offset of the box (first plane) in the buffer, in doubles
};

__global__ __launch_bounds__(256) void box_copy_kernel(real_t *__restrict__ arr, int II, int JJ, int KK, int nplanes,
                                                        BoxTable tab, real_t *__restrict__ buf, int unpack)
{
	const int bx = blockIdx.y;
	const int ni = tab.ni[bx], nj = tab.nj[bx], nk = tab.nk[bx];
	const size_t nbox = (size_t)ni * nj * nk, ntot = nbox * (size_t)nplanes;
	const size_t PS = (size_t)II * JJ * KK;
	for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < ntot; t += (size_t)gridDim.x * blockDim.x) {
		const size_t pl = t / nbox, r = t % nbox;
		const int i = (int)(r % ni), j = (int)((r / ni) % nj), k = (int)(r / ((size_t)ni * nj));
		const size_t a = pl * PS + (size_t)(tab.i0[bx] + i) +
		                 (size_t)II * ((size_t)(tab.j0[bx] + j * tab.sj[bx]) + (size_t)JJ * (size_t)(tab.k0[bx] + k * tab.sk[bx]));
		const size_t b = tab.off[bx] * (size_t)nplanes + t;
		if (unpack) arr[a] = buf[b];
		else buf[b] = arr[a];
	}
}

void box_copy(real_t *arr, int II, int JJ, int KK, int nplanes, int nboxes, const int *boxes /* 6 (8: + row step, plane step) per box */,
              const unsigned long long *offsets, real_t *buf, int unpack, hipStream_t st, int strided)
{
	if (nboxes <= 0) return;
	BoxTable tab;
	tab.n = nboxes;
	size_t maxn = 1;
	const int w = strided ? 8 : 6;
	for (int b = 0; b < nboxes && b < 26; b++) {
		tab.i0[b] = boxes[w * b]; tab.j0[b] = boxes[w * b + 1]; tab.k0[b] = boxes[w * b + 2];
		tab.ni[b] = boxes[w * b + 3]; tab.nj[b] = boxes[w * b + 4]; tab.nk[b] = boxes[w * b + 5];
		tab.sj[b] = strided ? boxes[w * b + 6] : 1; tab.sk[b] = strided ? boxes[w * b + 7] : 1;
		tab.off[b] = offsets[b];
		size_t n = (size_t)tab.ni[b] * tab.nj[b] * tab.nk[b] * nplanes;
		if (n > maxn) maxn = n;
	}
	unsigned gx = (unsigned)((maxn + 255) / 256);
	if (gx > 2048) gx = 2048;
	hipLaunchKernelGGL(box_copy_kernel, dim3(gx, nboxes), dim3(256), 0, st, arr, II, JJ, KK, nplanes, tab, buf, unpack);
}

} // namespace cedar_amd
