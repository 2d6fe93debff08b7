// Zebra line relaxation on single-precision copies of the operator and of the line factors
// (cedar_amd_solver_use_fp32_operator_lines).  The device bodies are those of the FP64 kernels
// (lines_dev.h), instantiated on the row-interleaved float copy (common.h Op2f) and on float factors: an entry is
// promoted to double when it is loaded (exact), vectors, LDS, the scan and all arithmetic stay FP64 in the same term
// order and chunking (-ffp-contract=off), so a sweep has the bits of relax_lines_x / relax_lines_yt (lines.hip) on the
// operator and the factor arrays each rounded to float.  Dirichlet lines only; batches through the launch grid.
#include "common.h"
#include "lines_dev.h"

namespace cedar_amd {

// plain float image of the two SOR planes (round to nearest even); *overflow as for op2f_build
__global__ __launch_bounds__(256) void linesf_image_kernel(const real_t *__restrict__ sor, float *__restrict__ out, size_t n,
                                                            int *__restrict__ overflow)
{
	bool bad = false;
	for (size_t x = (size_t)blockIdx.x * 256 + threadIdx.x; x < n; x += (size_t)gridDim.x * 256) {
		const real_t v = sor[x];
		const float f = (float)v;
		bad = bad || (isinf(f) && !isinf(v));
		out[x] = f;
	}
	if (bad) *overflow = 1;
}

void linesf_image(const real_t *sor, float *out, int II, int JJ, int *overflow, hipStream_t st)
{
	const size_t n = (size_t)II * JJ * 2;
	const size_t nb = (n + 255) / 256;
	hipLaunchKernelGGL(linesf_image_kernel, dim3((unsigned)(nb < 65536 ? nb : 65536)), dim3(256), 0, st, sor, out, n, overflow);
}

void linesf_permute(const real_t *sor, float *pf, int n, int ld, int nlines, size_t PS, int *overflow, hipStream_t st)
{
	lines_permute_t<float>(sor, pf, n, ld, nlines, PS, overflow, st);
}

void relax_lines_x_op(const Op2f &A, const real_t *qf, real_t *q, const float *sorf, int II, int JJ, int nstncl, int updown,
                      hipStream_t st, const float *pff, Batch bt)
{
	if (II < 3 || JJ < 3) return;
	if (!lds_ok(II - 2, "relax_lines_x")) return;
	for (int c = 0; c < 2; c++) {
		const int jb = (updown == BMG_DOWN) ? 1 - c : c; // DOWN: lines J = 3,5,.. first, as relax_lines_x
		launch_x(A, qf, q, sorf, II, JJ, nstncl, jb, st, false, false, pff, bt);
	}
}

// At: the copy of the transposed planes (the grid JJ fast, II rows); the transposes of q around the sweep are
// relax_lines_yt's
void relax_lines_yt_op(const Op2f &At, const real_t *qft, real_t *q, real_t *qt, const float *sorf, int II, int JJ, int nstncl,
                       int updown, hipStream_t st, const float *pff, Batch bt)
{
	if (II < 3 || JJ < 3) return;
	if (!lds_ok(JJ - 2, "relax_lines_y")) return;
	transpose2(q, qt, II, JJ, st, bt);
	for (int c = 0; c < 2; c++) {
		const int ib = (updown == BMG_DOWN) ? 1 - c : c; // DOWN: I = 3,5,.. first
		const int nlines = (II - 2 - ib + 1) / 2;
		if (nlines <= 0) continue;
		launch_x(At, qft, qt, sorf, JJ, II, nstncl, ib, st, false, true, pff, bt);
	}
	transpose2(qt, q, JJ, II, st, bt);
}

} // namespace cedar_amd
