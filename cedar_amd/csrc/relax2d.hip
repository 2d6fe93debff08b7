// 2D point relaxation: 9-point 4-colour and 5-point red-black Gauss-Seidel.
// Replaces BMG2_SymStd_relax_GS (reference src/2d/ftn/BMG2_SymStd_relax_GS.f90:76-137).
//
// 9-point: the reference's loop nest visits, for each row parity, row by row,
// the even-i then the odd-i points (DOWN; reversed for UP).  Rows of equal
// parity do not couple, and the second i-colour of a row only needs the first
// i-colour *of the same row*, so a workgroup that owns whole rows relaxes both
// i-colours in one pass: 2 launches per sweep, unit-stride row streams
// (64 algorithmic B/DOF), any row length.
// Bit-identical to the reference CPU build (term order kept, no contraction).
#include "common.h"
#include "relax2_dev.h"
#include "relax3_psum.h"

namespace cedar_amd {

__device__ __forceinline__ real_t gs9_mem(const real_t *__restrict__ so, const real_t *__restrict__ qf,
                                          const real_t *__restrict__ q, size_t sj, size_t PS, size_t x)
{
	real_t s = qf[x];
	s = s + so[KW * PS + x] * q[x - 1];
	s = s + so[KW * PS + x + 1] * q[x + 1];
	s = s + so[KS * PS + x] * q[x - sj];
	s = s + so[KS * PS + x + sj] * q[x + sj];
	s = s + so[KSW * PS + x] * q[x - 1 - sj];
	s = s + so[KNW * PS + x + 1] * q[x + 1 - sj];
	s = s + so[KNW * PS + x + sj] * q[x - 1 + sj];
	s = s + so[KSW * PS + x + 1 + sj] * q[x + 1 + sj];
	return s;
}

// The device bodies (row task, band walk, partial-sum F / S tasks, residual row) live in relax2_dev.h, written on a view
// of the operator; the kernels here give them the FP64 Cedar planes, op2f.hip the single-precision copy.

// rows j = j0 + jstep * L (0-based incl. ghost), L < nrows; the row classes use j0 = 1 + jb, jstep = 2
template <int BS, bool EFIRST>
__global__ __launch_bounds__(BS) void relax9_rows(const real_t *__restrict__ so, const real_t *__restrict__ qf,
                                                   real_t *__restrict__ q, const real_t *__restrict__ sor,
                                                   int II, int JJ, int j0, int jstep, int nrows, size_t bstride)
{
	__shared__ real_t xch[BS + 2];
	__shared__ real_t carry_s;
	const unsigned L = xcd_remap(blockIdx.x, (unsigned)nrows);
	if (L >= (unsigned)nrows) return;
	qf += bstride * blockIdx.y; q += bstride * blockIdx.y; // batch item (common.h Batch)
	relax9_row_task<BS, EFIRST>(op2_cedar(so, sor, II, JJ), qf, q, II, (size_t)(j0 + jstep * (int)L), xch, &carry_s);
}

// band-fused sweep: both row classes in one launch, a workgroup per run of frun F rows (relax2_dev.h relax9_band_body)
template <int BS, bool EFIRST>
__global__ __launch_bounds__(BS) void relax9_band(const real_t *__restrict__ so, const real_t *__restrict__ qf,
                                                   real_t *__restrict__ q, const real_t *__restrict__ sor,
                                                   int II, int JJ, int jbF, int frun, int nrun, size_t bstride)
{
	__shared__ real_t xch[BS + 2];
	__shared__ real_t carry_s;
	const unsigned run = xcd_remap(blockIdx.x, (unsigned)nrun);
	if (run >= (unsigned)nrun) return;
	qf += bstride * blockIdx.y; q += bstride * blockIdx.y; // batch item (common.h Batch)
	relax9_band_body<BS, EFIRST>(op2_cedar(so, sor, II, JJ), qf, q, II, JJ, jbF, frun, (int)run, xch, &carry_s);
}

// band-fused sweep with inter-row partial sums in LDS (relax2_dev.h relax9_band_psum_body)
template <int BS, bool EFIRST>
__global__ __launch_bounds__(BS) void relax9_band_psum(const real_t *__restrict__ so, const real_t *__restrict__ qf,
                                                        real_t *__restrict__ q, const real_t *__restrict__ sor,
                                                        int II, int JJ, int jbF, int frun, int nrun, size_t bstride)
{
	extern __shared__ real_t lds_band[];
	const int IIp = (II + 1) & ~1;
	real_t *T0 = lds_band, *T1 = lds_band + IIp, *xch = lds_band + 2 * IIp, *carry_s = xch + BS + 2;
	const unsigned run = xcd_remap(blockIdx.x, (unsigned)nrun);
	if (run >= (unsigned)nrun) return;
	qf += bstride * blockIdx.y; q += bstride * blockIdx.y; // batch item (common.h Batch)
	relax9_band_psum_body<BS, EFIRST>(op2_cedar(so, sor, II, JJ), qf, q, II, JJ, jbF, frun, (int)run, T0, T1, xch, carry_s);
}

// 9-point residual, pair per lane, 16-byte loads (BMG2_SymStd_residual.f90:88-99)
__global__ __launch_bounds__(256) void residual9_rows(const real_t *__restrict__ so, const real_t *__restrict__ qf,
                                                       const real_t *__restrict__ q, real_t *__restrict__ res,
                                                       int II, int JJ, unsigned nrows, size_t bstride)
{
	const unsigned L = xcd_remap(blockIdx.x, nrows);
	if (L >= nrows) return;
	qf += bstride * blockIdx.y; q += bstride * blockIdx.y; res += bstride * blockIdx.y; // batch item (common.h Batch)
	residual9_row_body(op2_cedar(so, nullptr, II, JJ), qf, q, res, II, (size_t)(L + 1));
}

void residual9_fast(const real_t *so, const real_t *qf, const real_t *q, real_t *res, int II, int JJ, hipStream_t st, Batch bt)
{
	unsigned nrows = (unsigned)(JJ - 2);
	hipLaunchKernelGGL(residual9_rows, dim3(xcd_grid(nrows), bt.n), dim3((II - 2) / 2 >= 256 ? 256 : 64), 0, st, so, qf, q, res, II, JJ,
	                   nrows, bt.stride);
}

// 5-point red-black, one colour per launch (relax_GS.f90:120-135): colour = mod(j+jo,2)
__global__ __launch_bounds__(256) void relax5_colour(const real_t *__restrict__ so, const real_t *__restrict__ qf,
                                                      real_t *__restrict__ q, const real_t *__restrict__ sor,
                                                      int II, int JJ, int jo, size_t bstride)
{
	qf += bstride * blockIdx.z; q += bstride * blockIdx.z; // batch item (common.h Batch)
	const int j1 = blockIdx.y + 2; // 1-based
	const int a = blockIdx.x * blockDim.x + threadIdx.x;
	const int i1 = (j1 + jo) % 2 + 2 + 2 * a;
	if (i1 > II - 1) return;
	const size_t sj = II;
	const size_t x = (size_t)(i1 - 1) + sj * (size_t)(j1 - 1);
	const Op2c A = op2_cedar(so, sor, II, JJ);
	q[x] = offdiag5(A, qf, q, i1 - 1, (size_t)(j1 - 1), x, sj) * A.rd((size_t)(j1 - 1))[i1 - 1];
}

// one row class (jb = parity of the 0-based row minus 1) of the nine-point sweep, both i-colours;
// efirst: even 1-based i first (the DOWN order of the 2D sweep).  Domain-decomposed runs exchange
// halos between row classes.
template <int BS>
static void launch_rows9(bool efirst, const real_t *so, const real_t *qf, real_t *q, const real_t *sor, int II, int JJ,
                         int j0, int jstep, int nrows, hipStream_t st, Batch bt = Batch())
{
	if (nrows <= 0) return;
	const dim3 grid(xcd_grid((unsigned)nrows), bt.n);
	if (efirst) hipLaunchKernelGGL((relax9_rows<BS, true>), grid, dim3(BS), 0, st, so, qf, q, sor, II, JJ, j0, jstep, nrows, bt.stride);
	else hipLaunchKernelGGL((relax9_rows<BS, false>), grid, dim3(BS), 0, st, so, qf, q, sor, II, JJ, j0, jstep, nrows, bt.stride);
}

static void pass9(const real_t *so, const real_t *qf, real_t *q, const real_t *sor, int II, int JJ, int jb, bool efirst,
                  hipStream_t st, Batch bt)
{
	const int nrows = (JJ - 2 - jb + 1) / 2;
	if ((II - 2 + 1) / 2 <= 64) launch_rows9<64>(efirst, so, qf, q, sor, II, JJ, 1 + jb, 2, nrows, st, bt);
	else launch_rows9<256>(efirst, so, qf, q, sor, II, JJ, 1 + jb, 2, nrows, st, bt);
}

void relax2_pass9(const real_t *so, const real_t *qf, real_t *q, const real_t *sor,
                  int II, int JJ, int jb, int efirst, hipStream_t st)
{
	pass9(so, qf, q, sor, II, JJ, jb, efirst != 0, st, Batch());
}

// F rows per workgroup of the band-fused sweep; 0 = two launches per sweep (one per row class).
// CEDAR_AMD_FRUN2 overrides (0 = never; n = runs of n rows wherever the grid has >= 4 runs per class).
int band_frun(int II, int JJ)
{
	const char *e = getenv("CEDAR_AMD_FRUN2"); // read per call: the tests switch it between cases
	const int ny = JJ - 2;
	if (e) {
		const int frun = atoi(e);
		return (frun <= 0 || ny < 8 * frun) ? 0 : frun;
	}
	// measured (profiles/r02_experiment_band_fused_relax9.log): 4096^2 -4.5 % at runs of 4, slower from 8 on (a 2D grid has
	// only ny/2 row tasks per class: long runs leave compute units idle), slower at 2048^2 and below at any run length
	return (ny >= 4096 && II - 2 >= 2048) ? 4 : 0;
}

// whole nine-point sweep
static void relax2_sweep9(const real_t *so, const real_t *qf, real_t *q, const real_t *sor, int II, int JJ, bool down, hipStream_t st,
                          Batch bt)
{
	const int frun = band_frun(II, JJ);
	if (frun == 0 || (II - 2 + 1) / 2 <= 64) {
		for (int c = 0; c < 2; c++) // DOWN: rows J=2,4,.. first (LSTART=2), even 1-based i first
			pass9(so, qf, q, sor, II, JJ, down ? c : 1 - c, down, st, bt);
		return;
	}
	const int jbF = down ? 0 : 1;
	const int nF = (JJ - 2 - jbF + 1) / 2, nrun = (nF + frun - 1) / frun;
	const dim3 grid(xcd_grid((unsigned)nrun), bt.n);
	if (down) hipLaunchKernelGGL((relax9_band<256, true>), grid, dim3(256), 0, st, so, qf, q, sor, II, JJ, jbF, frun, nrun, bt.stride);
	else hipLaunchKernelGGL((relax9_band<256, false>), grid, dim3(256), 0, st, so, qf, q, sor, II, JJ, jbF, frun, nrun, bt.stride);
	// S rows between runs: jbF = 0: j = 2 frun (r+1); jbF = 1: j = 1 + 2 frun (r+1), r = 0 .. nrun-2
	launch_rows9<256>(down, so, qf, q, sor, II, JJ, (jbF ? 1 : 0) + 2 * frun, 2 * frun, nrun - 1, st, bt);
}

// The sweep with inter-row partial sums (relax9_band_psum): rows of at most 4098 doubles (two T rows of LDS beside a second
// workgroup), at least 8 runs.  CEDAR_AMD_FRUN2 gives the run length as for the band-fused sweep.
int band_psum_frun(int II, int JJ)
{
	const char *e = getenv("CEDAR_AMD_FRUN2");
	const int ny = JJ - 2;
	if ((II - 2 + 1) / 2 <= 64 || (size_t)II * 2 * sizeof(real_t) > 68 * 1024) return 0;
	if (e) {
		const int frun = atoi(e);
		return (frun < 2 || ny < 8 * frun) ? 0 : frun;
	}
	// measured (profiles/r03_psum2d_run_length.log): 4096^2 0.310 -> 0.299 / 0.260 / 0.320 ms per sweep for runs of 2 / 4 / 8 rows
	// (a 2D grid has only ny/2 F rows: runs of 8 leave half the compute units idle), 2048^2 and 1024^2 slower than the two
	// row-class launches at every run length => the finest level of config 2 only
	return (ny >= 4096 && II - 2 >= 2048) ? 4 : 0;
}

bool relax2_psum_wanted(int II, int JJ)
{
	const char *e = getenv("CEDAR_AMD_PSUM");
	if (e && atoi(e) == 0) return false;
	return band_psum_frun(II, JJ) > 0;
}

void relax2_gs9_psum(const real_t *so, const real_t *qf, real_t *q, const real_t *sor, int II, int JJ, int updown, hipStream_t st,
                     Batch bt)
{
	const bool down = updown == BMG_DOWN;
	const int frun = band_psum_frun(II, JJ);
	if (frun == 0) {
		relax2_sweep9(so, qf, q, sor, II, JJ, down, st, bt);
		return;
	}
	const int jbF = down ? 0 : 1;
	const int nF = (JJ - 2 - jbF + 1) / 2, nrun = (nF + frun - 1) / frun;
	const size_t shm = ((size_t)((II + 1) & ~1) * 2 + 256 + 2 + 2) * sizeof(real_t);
	static bool attr_dev[64] = {false};
	int dev_ = 0;
	(void)hipGetDevice(&dev_);
	if (!attr_dev[dev_ & 63]) {
		CEDAR_HIP_CHECK(hipFuncSetAttribute((const void *)relax9_band_psum<256, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 72 * 1024));
		CEDAR_HIP_CHECK(hipFuncSetAttribute((const void *)relax9_band_psum<256, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 72 * 1024));
		attr_dev[dev_ & 63] = true;
	}
	const dim3 grid(xcd_grid((unsigned)nrun), bt.n);
	if (down) hipLaunchKernelGGL((relax9_band_psum<256, true>), grid, dim3(256), shm, st, so, qf, q, sor, II, JJ, jbF, frun, nrun, bt.stride);
	else hipLaunchKernelGGL((relax9_band_psum<256, false>), grid, dim3(256), shm, st, so, qf, q, sor, II, JJ, jbF, frun, nrun, bt.stride);
	launch_rows9<256>(down, so, qf, q, sor, II, JJ, (jbF ? 1 : 0) + 2 * frun, 2 * frun, nrun - 1, st, bt);
}

// recompute the points of column icol (0-based incl. ghost) on the rows of class jb: used after the
// x-neighbour's fresh first colour arrived (the update of a point does not read its own old value)
__global__ void relax9_column(const real_t *__restrict__ so, const real_t *__restrict__ qf,
                              real_t *__restrict__ q, const real_t *__restrict__ sor,
                              int II, int JJ, int icol, int jb)
{
	const int nrows = (JJ - 2 - jb + 1) / 2;
	const int t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= nrows) return;
	const size_t sj = II, PS = (size_t)II * JJ;
	const size_t x = (size_t)icol + sj * (size_t)(1 + jb + 2 * t);
	real_t s = qf[x];
	s = s + so[KW * PS + x] * q[x - 1];
	s = s + so[KW * PS + x + 1] * q[x + 1];
	s = s + so[KS * PS + x] * q[x - sj];
	s = s + so[KS * PS + x + sj] * q[x + sj];
	s = s + so[KSW * PS + x] * q[x - 1 - sj];
	s = s + so[KNW * PS + x + 1] * q[x + 1 - sj];
	s = s + so[KNW * PS + x + sj] * q[x - 1 + sj];
	s = s + so[KSW * PS + x + 1 + sj] * q[x + 1 + sj];
	q[x] = s * sor[PS + x];
}

void relax2_fixup9(const real_t *so, const real_t *qf, real_t *q, const real_t *sor,
                   int II, int JJ, int icol, int jb, hipStream_t st)
{
	const int nrows = (JJ - 2 - jb + 1) / 2;
	if (nrows <= 0) return;
	hipLaunchKernelGGL(relax9_column, dim3((nrows + 127) / 128), dim3(128), 0, st, so, qf, q, sor, II, JJ, icol, jb);
}

// one colour of the five-point red-black sweep: jo in {2,3}, points with mod(i+j+jo,2) == 0 (1-based)
static void colour5(const real_t *so, const real_t *qf, real_t *q, const real_t *sor, int II, int JJ, int jo, hipStream_t st, Batch bt)
{
	if (II < 3 || JJ < 3) return;
	dim3 grid(((II - 2 + 1) / 2 + 255) / 256, JJ - 2, bt.n);
	hipLaunchKernelGGL(relax5_colour, grid, dim3(256), 0, st, so, qf, q, sor, II, JJ, jo, bt.stride);
}

void relax2_colour5(const real_t *so, const real_t *qf, real_t *q, const real_t *sor,
                    int II, int JJ, int jo, hipStream_t st)
{
	colour5(so, qf, q, sor, II, JJ, jo, st, Batch());
}

void relax2_gs(const real_t *so, const real_t *qf, real_t *q, const real_t *sor,
               int II, int JJ, int nstncl, int updown, hipStream_t st, Batch bt)
{
	if (II < 3 || JJ < 3) return;
	const bool down = (updown == BMG_DOWN);
	if (nstncl == 5) {
		relax2_sweep9(so, qf, q, sor, II, JJ, down, st, bt);
	} else {
		for (int c = 0; c < 2; c++)
			colour5(so, qf, q, sor, II, JJ, down ? 2 + c : 3 - c /* LSTART..LEND */, st, bt);
	}
}

} // namespace cedar_amd
